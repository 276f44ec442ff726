// Connected components of a mask held as 64-bit column words (word x*HW64 + j = rows 64j .. 64j+63 of column x, padding bits
// beyond H clear: the layout of the RLE planes), for the clean-up of encoded sets (csrc/rle_clean.hip: hgl_rle_clean_device).
// The rule is remove_small_regions' (utils/amg.py:267-291), as csrc/sam_ccl.hip applies it to bytes.  The unit is a column
// SEGMENT: a maximal vertical stretch [y0, y1] of pixels of the working colour inside one column (foreground for islands, the
// complement for holes; padding bits are neither).  Two segments of one column never touch; segments of neighbouring columns
// belong to one 8-connected component iff their row ranges, one of them widened by a row at either end, meet.  A segment's id
// is its rank in (x, y0) order, which is the order the words' start bits come in.
//
// Every step stands alone: plain functions that compile under g++ (the harness tests/native/rle_clean_sanitize.cpp walks whole
// masks with them and a serial union-find) and as __device__ code (rle_clean.hip).  Nothing here needs HIP when __HIPCC__ is
// absent.
#ifndef HGL_CCL_RUNS_H
#define HGL_CCL_RUNS_H
#include <stdint.h>

#ifdef __HIPCC__
#define CCL_FN static __host__ __device__ inline
#else
#define CCL_FN static inline
#endif

// the rows of word j of a column of H rows that exist
CCL_FN unsigned long long ccl_valid(int H, int j) {
  const int nb = H - 64 * j < 64 ? H - 64 * j : 64;
  return nb == 64 ? ~0ull : ((1ull << nb) - 1ull);
}

// the pixels of the working colour in a plane word c
CCL_FN unsigned long long ccl_work(unsigned long long c, unsigned long long valid, bool holes) { return (holes ? ~c : c) & valid; }

// the working word j of a column (col: the column's HW64 plane words)
CCL_FN unsigned long long ccl_work_word(const unsigned long long* col, int H, int j, bool holes) {
  return ccl_work(col[j], ccl_valid(H, j), holes);
}

// the bits of working word d at which a segment starts; above: the working word over it in the same column, 0 for the first
// (a column's first pixel has no predecessor: segments do not continue across columns, unlike the runs of the RLE)
CCL_FN unsigned long long ccl_seg_starts(unsigned long long d, unsigned long long above) { return d & ~((d << 1) | (above >> 63)); }

// the starts of word j of a column
CCL_FN unsigned long long ccl_word_starts(const unsigned long long* col, int H, int j, bool holes) {
  return ccl_seg_starts(ccl_work_word(col, H, j, holes), j > 0 ? ccl_work_word(col, H, j - 1, holes) : 0ull);
}

// the last row of the segment that starts at bit b of word j of a column of HW64 words: it runs on through whole words
CCL_FN int ccl_seg_end(const unsigned long long* col, int H, int HW64, bool holes, int j, int b) {
  for (;;) {
    const unsigned long long valid = ccl_valid(H, j);
    const unsigned long long stop = ~ccl_work(col[j], valid, holes) & valid & (~0ull << b);      // rows at or below b of the other colour
    if (stop) return 64 * j + (int)__builtin_ctzll(stop) - 1;
    if (j + 1 >= HW64) return H - 1;      // a word with padding is the column's last
    ++j;
    b = 0;
  }
}

// segments [a0, a1] and [b0, b1] of neighbouring columns touch (8-connectivity: a diagonal step counts)
CCL_FN bool ccl_touch(int a0, int a1, int b0, int b1) { return a0 <= b1 + 1 && b0 <= a1 + 1; }
// the two-pointer walk over the sorted segments of two columns: after a pair is looked at, the one that ends first moves on (its
// successor starts two rows further down at least, so nothing the other can still touch is passed over)
CCL_FN bool ccl_first_moves(int a1, int b1) { return a1 <= b1; }

// a component's place in raster (row-major) order: that of its first pixel.  The minimum over the component's segments of
// y0 * W + x; < H*W < 2^31
CCL_FN unsigned ccl_key(int y0, int x, int W) { return (unsigned)y0 * (unsigned)W + (unsigned)x; }

// small: the component is filled (holes) or removed (islands) -- strictly below the threshold
CCL_FN bool ccl_small(unsigned area, int thresh) { return area < (unsigned)thresh; }

// the order by which islands mode picks its survivor when every component is small: the largest area, the first in raster order
// among equals.  The maximum of this number over the components.
CCL_FN unsigned long long ccl_rank(unsigned area, unsigned key) { return ((unsigned long long)area << 32) | (unsigned long long)(0xffffffffu - key); }

// the decision for one component once the whole mask is known: does its colour flip?  any_large: some component is not small;
// best: the maximum of ccl_rank over all components
CCL_FN bool ccl_flips(bool holes, unsigned area, unsigned key, int thresh, bool any_large, unsigned long long best) {
  if (!ccl_small(area, thresh)) return false;
  return holes || any_large || ccl_rank(area, key) != best;
}

// the rows of segment [y0, y1] that lie in word j, as bits of that word (0: none)
CCL_FN unsigned long long ccl_seg_bits(int y0, int y1, int j) {
  const int lo = y0 > 64 * j ? y0 - 64 * j : 0, hi = y1 < 64 * j + 63 ? y1 - 64 * j : 63;
  if (lo > hi) return 0ull;
  const int n = hi - lo + 1;
  return (n == 64 ? ~0ull : ((1ull << n) - 1ull)) << lo;
}

// the most segments of one colour an H x W mask can have: every other row of every column
CCL_FN long long ccl_seg_bound(long long H, long long W) { return W * ((H + 1) / 2); }

#endif  // HGL_CCL_RUNS_H
