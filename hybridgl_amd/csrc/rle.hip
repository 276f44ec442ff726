// Run-length encoding of device masks, selected by a DEVICE index tensor (hgl_rle_encode_device).
//
// The records the mask generator hands out in its RLE modes and the evaluator's winning masks are column-major run
// lengths (utils/amg.py:107-136 mask_to_rle_pytorch, refer/external/maskApi.c rleEncode): runs over p = x*H + y, the first
// count = leading zeros (0 when pixel (0,0) is set), runs continue across column boundaries, the last count ends at H*W.
// hgl_rle_encode_mask (gtmask.cpp) is the host form of the same arithmetic; here the masks never leave the device as
// pixels -- only runs (or, for a mask with more runs than its slot holds, one bit per pixel) cross to the host.
//
// Two launches, no atomics, no host synchronisation; every selected entry owns its slot and its table row.
//
//   1. rle_columns_kernel   the masks are row-major, the runs column-major.  Lane x of a wave walks 64 rows of column x: every
//      row is read coalesced across the lanes (1 or 4 bytes per lane) and sets one bit of the lane's own 64-bit column word.
//      The column words, every column padded to whole 64-bit words, go to the workspace in run order: word x*HW64 + j holds
//      the pixels y = 64j .. 64j+63 of column x (bits beyond H are 0).  No LDS transpose, no strided byte walk.
//   2. rle_runs_kernel      one workgroup per selected mask.  A pixel starts a run where it differs from its predecessor in run
//      order: T = C ^ ((C << 1) | carry_in), masked to the valid bits of the word; carry_in is the last valid pixel of the
//      previous word (0 before the first pixel, so a mask that starts with foreground has a transition at p = 0 and
//      counts[0] = 0).  A first sweep pop-counts T (the number of counts is transitions + 1) and C (the area) and so decides
//      what the slot holds; the second sweep takes the words 256 at a time: an exclusive sum-scan of the pop-counts gives the
//      rank of every word's first transition, an exclusive max-scan of "position of my last transition" the position of the
//      last earlier one, both carried from chunk to chunk, and every transition writes its own counts[k] = p_k - p_(k-1)
//      (rle_counts_chunk in rle_scan.h: the polygon rasteriser of rle_poly.hip ends in the same scan).  Both sweeps are
//      rle_write_runs, a device function over any column plane: the merge kernel further down ends in it too.
//
// Slot forms (table row = n_counts, form, area, 0): 0 = the n_counts counts (whenever they fit), 1 = the column-major bit
// plane (bit p % 32 of word p / 32; whenever the counts do not fit but ceil(H*W/32) words do), 2 = neither fits, nothing
// written, 3 = the index is outside [0, N), nothing read or written.  Words beyond what the form defines keep their bytes.
#include "hgl_common.h"
#include "rle_group.h"      // RleTiles, RleGroup, RleOne, RleSet and the rle_*_plan functions: plain C++, shared with the sanitizer harnesses
#include "rle_scan.h"       // RLE_THREADS, the block reductions, rle_group_find, rle_counts_chunk, rle_write_runs, rle_stage_ws: shared with rle_poly.hip, rle_clean.hip
#include "nms_walk.h"       // nms_before, nms_resolve_block, nms_emit_block: shared with sam_nms.hip

namespace {

// the mask of entry s, or -1 when its index is outside [0, N) (the host never sees the indices)
__device__ __forceinline__ long long rle_pick(const long long* sel, int s, int N) {
  const long long n = sel ? sel[s] : (long long)s;
  return (n < 0 || n >= (long long)N) ? -1 : n;
}

// V columns per lane (4: one aligned 32-bit load per row when W % 4 == 0), 64 rows per wave, 4 waves = 4 row tiles per block
template <int V>
__global__ __launch_bounds__(RLE_THREADS) void rle_columns_kernel(const uint8_t* __restrict__ masks, int N, int H, int W,
                                                                  const long long* __restrict__ sel, int HW64, int col_tiles,
                                                                  int row_tiles, unsigned long long* __restrict__ plane) {
  const unsigned tile = blockIdx.x;
  const int s = (int)(tile / (unsigned)(col_tiles * row_tiles));
  const int rem = (int)(tile % (unsigned)(col_tiles * row_tiles));
  const long long n = rle_pick(sel, s, N);
  if (n < 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = (rem / col_tiles) * 4 + wave;
  const int x = ((rem % col_tiles) * 64 + lane) * V;
  if (j >= HW64 || x >= W) return;      // no barrier and no cross-lane operation below
  const int y0 = j * 64;
  const int rows = H - y0 < 64 ? H - y0 : 64;
  const uint8_t* src = masks + (size_t)n * H * W + (size_t)y0 * W + x;
  unsigned long long c[V];
#pragma unroll
  for (int k = 0; k < V; ++k) c[k] = 0;
#pragma unroll 8
  for (int r = 0; r < rows; ++r) {
    if (V == 4) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(src + (size_t)r * W);
#pragma unroll
      for (int k = 0; k < V; ++k) c[k] |= (unsigned long long)(((v >> (8 * k)) & 0xffu) != 0) << r;
    } else {
      c[0] |= (unsigned long long)(src[(size_t)r * W] != 0) << r;
    }
  }
  unsigned long long* dst = plane + (size_t)s * W * HW64 + (size_t)x * HW64 + j;
#pragma unroll
  for (int k = 0; k < V; ++k) dst[(size_t)k * HW64] = c[k];      // x + k < W: W % 4 == 0 on the 4-column path
}

__global__ __launch_bounds__(RLE_THREADS) void rle_runs_kernel(const unsigned long long* __restrict__ plane, int N, int H, int W,
                                                               const long long* __restrict__ sel, int HW64,
                                                               uint32_t* __restrict__ slots, long long slot_words,
                                                               int32_t* __restrict__ table) {
  __shared__ unsigned red[4];
  __shared__ unsigned wsum[4], wmax[4];
  const int s = blockIdx.x, t = threadIdx.x;
  int32_t* row = table + (size_t)s * 4;
  if (rle_pick(sel, s, N) < 0) {
    if (t == 0) { row[0] = 0; row[1] = 3; row[2] = 0; row[3] = 0; }
    return;
  }
  rle_write_runs(plane + (size_t)s * W * HW64, H, W, HW64, slots + (size_t)s * (size_t)slot_words, slot_words, row, red, wsum, wmax);
}

// ---- the way back: slots + table -> masks (hgl_rle_decode_device, hgl_rle_decode_group_device) and intersection / union of two
// encoded sets (hgl_rle_iou_device).  ONE decoder: the S entries of a call belong to G <= 64 images of their own sizes, and a
// single-size set is a group of one.  The geometry rides in the kernel arguments, by value (no descriptor memory, nothing to keep
// alive), in one of two shapes the kernels are compiled for: RleGroup, in which a block finds its image by a search of <= 6
// steps over <= 64 rows of the arguments, uniform over the block; RleOne (a call of one image that starts at `masks`): H and W,
// no search, nothing else to load.  The mirror image of the launches above, two per decode call whatever G is:
//
//   A. rle_starts_kernel<BOX>   one workgroup per entry decides what the slot holds (the status code) and, for form 0, sum-scans
//      the counts 256 at a time with a 64-bit carry into run starts E_k (E_0 = 0, saturated at H*W, so a count of 0xFFFFFFFF
//      cannot wrap).  The area is the clipped length of the odd runs (form 0) or the pop-count of the plane's valid bits (form 1).
//      BOX: the mask's box is read off the same runs / plane words (the group entry); without it no box is kept and none written.
//   B. rle_plane_word      any 64-bit column word -- rows 64j .. 64j+63 of column x, the encoder's own layout -- from its
//      entry alone.  Form 0: an upper-bound search in E finds the last run that starts at or before the word's first pixel,
//      then the runs that touch the word are walked: no atomics, no scatter, O(words * log n + n) over an entry.  Form 1: the
//      32-bit run-order words are re-packed (the inverse of the encoder's form-1 branch).  An entry of code 2 gives 0.
//   C. rle_rows_kernel<V>  the inverse of rle_columns_kernel: (image, entry, tile) of a block from the host's tile prefix sums;
//      lane x forms the column word(s) of its 64 rows with B and every row is one coalesced store across the lanes (rle_rows_tile:
//      1 or 4 bytes per lane).  V = 4 / 1: every image of the call takes that store path (a single image always does);
//      V = 0: each image its own, a branch uniform over the block.  Every byte of every entry is written exactly once; the
//      decoder keeps no plane anywhere.
//   D. rle_plane_kernel<GEO> / rle_iou_kernel   for the IoU the words of both sets go to the workspace, one thread per word, and
//      one workgroup per entry pop-counts a & b and a | b: padding bits are 0 on both sides, no mask is expanded to bytes.  GEO:
//      RlePlaneOne (the pairwise IoU: one size) or RleSet (the match below: the block finds its image by a search).

// the slot of an entry holds a mask (include/hybridgl.h: anything else is code 2)
__device__ __forceinline__ bool rle_entry_usable(int n, int form, long long slot_words, unsigned plane_words) {
  if (n < 0) return false;
  if (form == 0) return (long long)n <= slot_words;
  if (form == 1) return (long long)plane_words <= slot_words;      // a plane that the slot cannot hold is never read
  return false;
}

// rows 64j .. 64j+63 of column x of an entry that holds a mask (bits beyond H are 0); Es: the entry's run starts (form 0)
__device__ __forceinline__ unsigned long long rle_plane_word(const uint32_t* __restrict__ slot, int form, int n,
                                                             const uint32_t* __restrict__ Es, unsigned plane_words, int H, int x,
                                                             int j) {
  const int nb = H - 64 * j < 64 ? H - 64 * j : 64;
  const unsigned p0 = (unsigned)x * (unsigned)H + 64u * (unsigned)j, p1 = p0 + (unsigned)nb;      // p1 <= H*W
  unsigned long long c = 0;
  if (form == 1) {
    // the nb <= 64 bits from p0 on live in at most three 32-bit words
    const unsigned w = p0 >> 5, o = p0 & 31u;
    const unsigned long long w0 = slot[w];
    const unsigned long long w1 = w + 1 < plane_words ? slot[w + 1] : 0u;
    const unsigned long long w2 = w + 2 < plane_words ? slot[w + 2] : 0u;
    c = (w0 | (w1 << 32)) >> o;
    if (o) c |= w2 << (64 - o);
    if (nb < 64) c &= (1ull << nb) - 1ull;
  } else if (n > 0) {
    unsigned lo = 0, hi = (unsigned)n - 1u;      // the last run k in [0, n) with E[k] <= p0 (E[0] = 0)
    while (lo < hi) {
      const unsigned mid = (lo + hi + 1u) >> 1;
      if (Es[mid] <= p0) lo = mid; else hi = mid - 1u;
    }
    unsigned k = lo, pos = p0;
    while (pos < p1 && k < (unsigned)n) {
      const unsigned e = Es[k + 1];
      const unsigned end = e < p1 ? e : p1;
      if (end > pos) {
        if (k & 1u) {
          const unsigned len = end - pos;      // 1 .. 64
          c |= (len == 64u ? ~0ull : ((1ull << len) - 1ull)) << (pos - p0);
        }
        pos = end;
      }
      ++k;
    }
  }
  return c;
}

// The box of the pixels [a, b) of run order (a < b <= H*W) joined into (x0, y0, x1, y1): x in [a / H, (b-1) / H]; within one
// column y in [a % H, (b-1) % H], and a stretch that crosses a column boundary holds a pixel of row H-1 and one of row 0.
__device__ __forceinline__ void rle_box_join(unsigned a, unsigned b, unsigned H, unsigned& x0, unsigned& y0, unsigned& x1,
                                             unsigned& y1) {
  const unsigned xa = a / H, xb = (b - 1u) / H;
  unsigned ya = a - xa * H, yb = (b - 1u) - xb * H;
  if (xa != xb) { ya = 0; yb = H - 1u; }
  x0 = x0 < xa ? x0 : xa;
  x1 = x1 > xb ? x1 : xb;
  y0 = y0 < ya ? y0 : ya;
  y1 = y1 > yb ? y1 : yb;
}

// The size of the image that owns entry s: looked up in a group, the image itself in a call of one.
template <class GRP>      // RleGroup or RleSet
__device__ __forceinline__ void rle_entry_size(const GRP& grp, int s, int& H, int& W) {
  const int g = rle_group_find(grp.first, grp.G, s);
  H = grp.H[g], W = grp.W[g];
}
__device__ __forceinline__ void rle_entry_size(const RleOne& one, int, int& H, int& W) { H = one.H, W = one.W; }
__device__ __forceinline__ void rle_entry_size(const RlePick& pick, int t, int& H, int& W) { rle_entry_size(pick.pos, t, H, W); }

// The entry whose table row and slot staged row s reads: s itself -- except under RlePick (the paint list), where row t reads the
// entry its list position names, or nothing (-1, status code 3) when order[t] is outside the image's entries.
template <class GEO>
__device__ __forceinline__ int rle_entry_source(const GEO&, int s) { return s; }
__device__ __forceinline__ int rle_entry_source(const RlePick& pick, int t) {
  const int g = rle_group_find(pick.pos.first, pick.pos.G, t);
  const int o = pick.order[t];
  return (o >= 0 && o < pick.entries[g]) ? pick.entry0[g] + o : -1;
}

// What a block of the rows kernel needs of the image that owns its tile: size and tiling (rle_tiles' arithmetic; a call of one
// brings the host's), first entry and tile, byte offset of the first entry, store path (V = 0: the image's own, else V's).
struct RleImage {
  int H, W, HW64, col_tiles, row_tiles, first;
  unsigned tile0;
  long long off;
  bool wide;
};
template <int V>
__device__ __forceinline__ RleImage rle_tile_image(const RleGroup& grp, unsigned tile) {
  const int g = rle_group_find(grp.tile0, grp.G, tile);
  const bool wide = V == 0 ? (bool)((grp.wide >> g) & 1ull) : V == 4;
  const int H = grp.H[g], W = grp.W[g], HW64 = (H + 63) / 64;
  return {H, W, HW64, (W + (wide ? 255 : 63)) / (wide ? 256 : 64), (HW64 + 3) / 4, grp.first[g], grp.tile0[g], grp.off[g], wide};
}
template <int V>
__device__ __forceinline__ RleImage rle_tile_image(const RleOne& one, unsigned) {
  return {one.H, one.W, one.HW64, one.col_tiles, one.row_tiles, 0, 0u, 0ll, V == 4};
}

// boxes [S,4] (BOX only) receives the inclusive XYXY box of the mask the entry decodes to (batched_mask_to_box,
// utils/amg.py:303-346; zeros for an empty mask and for code 2), read off the runs (form 0) or the plane words (form 1) in the
// pass that scans them.  GEO: RleGroup, RleSet or RleOne.
template <bool BOX, class GEO>
__global__ __launch_bounds__(RLE_THREADS) void rle_starts_kernel(const uint32_t* __restrict__ slots, long long slot_words,
                                                                 const int32_t* __restrict__ table, const GEO geo,
                                                                 uint32_t* __restrict__ E, long long e_stride,
                                                                 int32_t* __restrict__ status, int32_t* __restrict__ boxes) {
  __shared__ unsigned red[4];
  __shared__ unsigned long long wtot[4];
  const int s = blockIdx.x;
  int H, W;
  rle_entry_size(geo, s, H, W);
  int32_t* box = BOX ? boxes + (size_t)s * 4 : nullptr;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  int32_t* row = status + (size_t)s * 4;
  const int src = rle_entry_source(geo, s);
  if (src < 0) {      // uniform over the workgroup; RlePick alone
    if (t == 0) {
      row[0] = 3; row[1] = 0; row[2] = 0; row[3] = 0;
      if (BOX) { box[0] = 0; box[1] = 0; box[2] = 0; box[3] = 0; }
    }
    return;
  }
  const int n = table[(size_t)src * 4], form = table[(size_t)src * 4 + 1];
  const unsigned HW = (unsigned)H * (unsigned)W;      // < 2^31 (checked by the host entry)
  const unsigned plane_words = (HW + 31u) / 32u;
  if (!rle_entry_usable(n, form, slot_words, plane_words)) {      // uniform over the workgroup
    if (t == 0) {
      row[0] = 2; row[1] = 0; row[2] = 0; row[3] = 0;
      if (BOX) { box[0] = 0; box[1] = 0; box[2] = 0; box[3] = 0; }
    }
    return;
  }
  const uint32_t* slot = slots + (size_t)src * (size_t)slot_words;
  unsigned area = 0;
  unsigned bx0 = 0x7fffffffu, by0 = 0x7fffffffu, bx1 = 0, by1 = 0;      // the box of this thread's pixels
  int code = 0;
  if (form == 1) {
    const unsigned tail = HW - 32u * (plane_words - 1u);      // 1 .. 32 valid bits in the last word
    for (unsigned w = t; w < plane_words; w += RLE_THREADS) {
      uint32_t v = slot[w];
      if (w == plane_words - 1u && tail < 32u) v &= (1u << tail) - 1u;
      area += __popc(v);
      if (BOX && v) {
        // the word's set pixels column by column (a word spans several columns when H < 32)
        const unsigned p = 32u * w;
        unsigned x = p / (unsigned)H, y = p - x * (unsigned)H, filled = 0;
        while (filled < 32u && x < (unsigned)W) {
          const unsigned m = 32u - filled < (unsigned)H - y ? 32u - filled : (unsigned)H - y;
          const uint32_t seg = (v >> filled) & (m == 32u ? 0xffffffffu : ((1u << m) - 1u));
          if (seg) {
            const unsigned ya = y + (unsigned)__builtin_ctz(seg), yb = y + 31u - (unsigned)__builtin_clz(seg);
            bx0 = bx0 < x ? bx0 : x;
            bx1 = bx1 > x ? bx1 : x;
            by0 = by0 < ya ? by0 : ya;
            by1 = by1 > yb ? by1 : yb;
          }
          filled += m;
          y += m;
          if (y == (unsigned)H) { y = 0; ++x; }
        }
      }
    }
  } else {
    uint32_t* Es = E + (size_t)s * (size_t)e_stride;      // n + 1 <= slot_words + 1 <= e_stride entries
    // E[k] = min(H*W, counts[0] + .. + counts[k-1]); the sums are exact in 64 bits (n < 2^31 counts < 2^32)
    unsigned long long carry = 0;
    if (t == 0) Es[0] = 0;
    for (unsigned base = 0; base < (unsigned)n; base += RLE_THREADS) {
      const unsigned i = base + t;
      const unsigned long long own = i < (unsigned)n ? (unsigned long long)slot[i] : 0ull;
      unsigned long long v = own;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long a = __shfl_up(v, d, 64);
        if (lane >= d) v += a;
      }
      __syncthreads();      // the previous chunk's reads of wtot are over
      if (lane == 63) wtot[wave] = v;
      __syncthreads();
      unsigned long long sum = carry + v, tot = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (w < wave) sum += wtot[w];
        tot += wtot[w];
      }
      if (i < (unsigned)n) {
        const unsigned end = sum < (unsigned long long)HW ? (unsigned)sum : HW;
        const unsigned start = sum - own < (unsigned long long)HW ? (unsigned)(sum - own) : HW;
        Es[i + 1] = end;
        if (i & 1u) area += end - start;
        if (BOX && (i & 1u) && end > start) rle_box_join(start, end, (unsigned)H, bx0, by0, bx1, by1);
      }
      carry += tot;
    }
    code = carry == (unsigned long long)HW ? 0 : 1;
  }
  area = rle_block_sum(area, red);
  if (t == 0) { row[0] = code; row[1] = (int32_t)area; row[2] = 0; row[3] = 0; }
  if (!BOX) return;
  // minima as maxima of the complement; an empty mask keeps the zeros of batched_mask_to_box
  bx0 = 0x7fffffffu - rle_block_max(0x7fffffffu - bx0, red);
  by0 = 0x7fffffffu - rle_block_max(0x7fffffffu - by0, red);
  bx1 = rle_block_max(bx1, red);
  by1 = rle_block_max(by1, red);
  if (t == 0) {
    box[0] = area ? (int32_t)bx0 : 0;
    box[1] = area ? (int32_t)by0 : 0;
    box[2] = area ? (int32_t)bx1 : 0;
    box[3] = area ? (int32_t)by1 : 0;
  }
}

// rows 64j .. 64j+63 of columns x .. x+V-1 of entry s (j < HW64, x < W) into the entry's mask at dst [H,W]; V columns per lane
// (4: one aligned 32-bit store per row when W % 4 == 0 and dst is 4-byte aligned).  No barrier, no cross-lane operation.
template <int V>
__device__ __forceinline__ void rle_rows_tile(const uint32_t* __restrict__ slots, long long slot_words,
                                              const int32_t* __restrict__ table, const uint32_t* __restrict__ E, long long e_stride,
                                              const int32_t* __restrict__ status, int s, int H, int W, int j, int x,
                                              uint8_t* __restrict__ dst) {
  const int y0 = j * 64;
  const int rows = H - y0 < 64 ? H - y0 : 64;
  unsigned long long c[V];
#pragma unroll
  for (int k = 0; k < V; ++k) c[k] = 0;
  if (status[(size_t)s * 4] != 2) {
    const int n = table[(size_t)s * 4], form = table[(size_t)s * 4 + 1];
    const unsigned plane_words = ((unsigned)H * (unsigned)W + 31u) / 32u;
#pragma unroll
    for (int k = 0; k < V; ++k)      // x + k < W: W % 4 == 0 on the 4-column path
      c[k] = rle_plane_word(slots + (size_t)s * (size_t)slot_words, form, n, E + (size_t)s * (size_t)e_stride, plane_words, H, x + k, j);
  }
  dst = dst + (size_t)y0 * W + x;      // (y0 + r) * W + x (+ 3) < H * W
#pragma unroll 8
  for (int r = 0; r < rows; ++r) {
    if (V == 4) {
      uint32_t v = 0;
#pragma unroll
      for (int k = 0; k < V; ++k) v |= (uint32_t)((c[k] >> r) & 1ull) << (8 * k);
      *reinterpret_cast<uint32_t*>(dst + (size_t)r * W) = v;
    } else {
      dst[(size_t)r * W] = (uint8_t)((c[0] >> r) & 1ull);
    }
  }
}

// 64 rows per wave, 4 waves = 4 row tiles per block; V as under C above, GEO: RleGroup or RleOne.  Waves per SIMD are asked for
// (8 with one store path, 5 with both): left alone, the register allocator spreads V = 4 over a group over 94 VGPRs, occupancy 5.
template <int V, class GEO>
__global__ __launch_bounds__(RLE_THREADS, V ? 8 : 5) void rle_rows_kernel(const uint32_t* __restrict__ slots, long long slot_words,
                                                                          const int32_t* __restrict__ table,
                                                                          const uint32_t* __restrict__ E, long long e_stride,
                                                                          const int32_t* __restrict__ status, const GEO geo,
                                                                          uint8_t* __restrict__ masks) {
  const unsigned tile = blockIdx.x;
  const RleImage im = rle_tile_image<V>(geo, tile);
  const int H = im.H, W = im.W, HW64 = im.HW64, col_tiles = im.col_tiles, row_tiles = im.row_tiles;
  const bool wide = im.wide;      // a constant unless V == 0: one store path is compiled
  const unsigned local = tile - im.tile0;
  const int k = (int)(local / (unsigned)(col_tiles * row_tiles));      // the entry within its image
  const int rem = (int)(local % (unsigned)(col_tiles * row_tiles));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = (rem / col_tiles) * 4 + wave;
  uint8_t* dst = masks + im.off + (size_t)k * H * W;
  const int s = im.first + k;
  const int x = ((rem % col_tiles) * 64 + lane) * (wide ? 4 : 1);
  if (j >= HW64 || x >= W) return;
  if (wide)
    rle_rows_tile<4>(slots, slot_words, table, E, e_stride, status, s, H, W, j, x, dst);
  else
    rle_rows_tile<1>(slots, slot_words, table, E, e_stride, status, s, H, W, j, x, dst);
}

// The entry and the size of the image that own block `blk` of the plane kernel, the block's rank among the entry's q_tiles
// blocks and the plane word the entry starts at: looked up in a group, plain arithmetic in a call of one.
struct RlePlaneBlock {
  int s, H, W, HW64;
  unsigned tile;
  size_t word0;
};
__device__ __forceinline__ RlePlaneBlock rle_plane_block(const RlePlaneOne& one, unsigned blk) {
  const int s = (int)(blk / (unsigned)one.q_tiles);
  return {s, one.H, one.W, one.HW64, blk % (unsigned)one.q_tiles, (size_t)s * (size_t)one.W * (size_t)one.HW64};
}
__device__ __forceinline__ RlePlaneBlock rle_plane_block(const RleSet& grp, unsigned blk) {
  const int g = rle_group_find(grp.blk0, grp.G, blk);
  const int H = grp.H[g], W = grp.W[g], HW64 = (H + 63) / 64;
  const unsigned Q = (unsigned)W * (unsigned)HW64, q_tiles = (Q + RLE_THREADS - 1) / RLE_THREADS;
  const unsigned local = blk - grp.blk0[g], k = local / q_tiles;
  return {grp.first[g] + (int)k, H, W, HW64, local % q_tiles, (size_t)grp.word0[g] + (size_t)k * Q};
}

__device__ __forceinline__ RlePlaneBlock rle_plane_block(const RlePick& pick, unsigned blk) { return rle_plane_block(pick.pos, blk); }

// one thread per plane word: word q = x*HW64 + j of an entry, ceil(Q / 256) workgroups per entry.  GEO: RlePlaneOne, RleSet or
// RlePick (a row of the list: status, run starts and plane are the row's, table row and slot the named entry's).
template <class GEO>
__global__ __launch_bounds__(RLE_THREADS) void rle_plane_kernel(const uint32_t* __restrict__ slots, long long slot_words,
                                                                const int32_t* __restrict__ table, const uint32_t* __restrict__ E,
                                                                long long e_stride, const int32_t* __restrict__ status, const GEO geo,
                                                                unsigned long long* __restrict__ plane) {
  const RlePlaneBlock b = rle_plane_block(geo, blockIdx.x);
  const int s = b.s, H = b.H, W = b.W, HW64 = b.HW64;
  const unsigned q = b.tile * RLE_THREADS + threadIdx.x;
  const unsigned Q = (unsigned)W * (unsigned)HW64;
  if (q >= Q) return;
  unsigned long long c = 0;
  const int src = rle_entry_source(geo, s);
  if (src >= 0 && status[(size_t)s * 4] != 2) {
    const unsigned plane_words = ((unsigned)H * (unsigned)W + 31u) / 32u;
    c = rle_plane_word(slots + (size_t)src * (size_t)slot_words, table[(size_t)src * 4 + 1], table[(size_t)src * 4],
                       E + (size_t)s * (size_t)e_stride, plane_words, H, (int)(q / (unsigned)HW64), (int)(q % (unsigned)HW64));
  }
  plane[b.word0 + q] = c;
}

__global__ __launch_bounds__(RLE_THREADS) void rle_iou_kernel(const unsigned long long* __restrict__ pa,
                                                              const unsigned long long* __restrict__ pb,
                                                              const int32_t* __restrict__ sa, const int32_t* __restrict__ sb,
                                                              unsigned Q, long long* __restrict__ iu) {
  __shared__ unsigned red[4];
  const int s = blockIdx.x, t = threadIdx.x;
  if (sa[(size_t)s * 4] == 2 || sb[(size_t)s * 4] == 2) {      // uniform over the workgroup
    if (t == 0) { iu[(size_t)s * 2] = -1; iu[(size_t)s * 2 + 1] = -1; }
    return;
  }
  const unsigned long long* A = pa + (size_t)s * Q;
  const unsigned long long* B = pb + (size_t)s * Q;
  unsigned inter = 0, uni = 0;      // <= H*W < 2^31
  for (unsigned q = t; q < Q; q += RLE_THREADS) {
    const unsigned long long a = A[q], b = B[q];
    inter += __popcll(a & b);
    uni += __popcll(a | b);
  }
  inter = rle_block_sum(inter, red);
  uni = rle_block_sum(uni, red);
  if (t == 0) { iu[(size_t)s * 2] = (long long)inter; iu[(size_t)s * 2 + 1] = (long long)uni; }
}

// ---- new masks out of encoded masks (hgl_rle_merge_device): output entry s is a vote over k_s source entries of its own image,
// a pixel is set iff lo_s <= (members that cover it) <= hi_s -- rleMerge (refer/external/maskApi.c:49-70) is lo = 1 (union) or
// lo = k (intersection) with hi = k.  Three launches whatever G, S, M and the sizes are: A and D above put the source set's column
// words into the workspace; then
//
//   G. rle_merge_kernel   one workgroup per output entry.  It checks the entry's members (a block-wide maximum of their codes),
//      then a thread owns plane word q = x*HW64 + j and walks the members: a member's word is one 8-byte load, coalesced over the
//      workgroup (the words of an entry are contiguous); the member index is the same for every thread (a scalar load).  The
//      count of every one of the word's 64 pixels is kept bit-sliced: slice b holds bit b of all 64 counts, ceil(log2(k+1)) <= 16
//      slices, and a member is added by a ripple of AND / XOR through them (count <= k never carries out of the top slice).
//      lo <= count and count <= hi are two bit-serial comparisons from the top slice down (hi clamped to k; lo > k sets nothing).
//      All loop bounds are uniform over the workgroup; no pixel is ever a byte.  The padding bits beyond H are masked (the rule
//      (0, 0) would set them).  The merged word goes to the entry's plane in the workspace -- materialised once: both sweeps of
//      the run writer read it, and a re-vote per sweep would read k words for each -- and after a barrier the workgroup runs
//      rle_write_runs on it: the encoder's own slot and table row.
// One plane word of a vote: the counts of its 64 pixels over the k members mem[0 .. k) (absolute source indices; the word of
// member m lies at P[(m - src_lo) * Q]), bit-sliced into NB slices (k < 2^NB), and the pixels whose count lies in [lo, hi]
// (0 <= lo, hi <= k).  All loop bounds are uniform over the workgroup.
template <int NB>
__device__ __forceinline__ unsigned long long rle_vote_word(const unsigned long long* __restrict__ P, unsigned Q,
                                                            const int32_t* __restrict__ mem, int k, int src_lo, int lo, int hi) {
  unsigned long long c[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) c[b] = 0;
#pragma unroll 4
  for (int i = 0; i < k; ++i) {
    unsigned long long carry = P[(size_t)(mem[i] - src_lo) * Q];
#pragma unroll
    for (int b = 0; b < NB; ++b) {      // a ripple add of one bit per pixel; count <= k never carries out of the top slice
      const unsigned long long both = c[b] & carry;
      c[b] ^= carry;
      carry = both;
    }
  }
  unsigned long long gt = 0, lt = 0, eq_lo = ~0ull, eq_hi = ~0ull;      // count > lo, count < hi, equal so far
#pragma unroll
  for (int b = NB - 1; b >= 0; --b) {
    const unsigned long long lb = ((lo >> b) & 1) ? ~0ull : 0ull, hb = ((hi >> b) & 1) ? ~0ull : 0ull;
    gt |= eq_lo & c[b] & ~lb;
    eq_lo &= ~(c[b] ^ lb);
    lt |= eq_hi & ~c[b] & hb;
    eq_hi &= ~(c[b] ^ hb);
  }
  return (gt | eq_lo) & (lt | eq_hi);
}

__global__ __launch_bounds__(RLE_THREADS) void rle_merge_kernel(const unsigned long long* __restrict__ src_plane,
                                                                const int32_t* __restrict__ src_status, const RleMerge geo,
                                                                const int32_t* __restrict__ members, int M,
                                                                const int32_t* __restrict__ member_offsets,
                                                                const int32_t* __restrict__ bounds, unsigned long long* merged,
                                                                uint32_t* __restrict__ slots, long long slot_words,
                                                                int32_t* __restrict__ table, int32_t* __restrict__ status) {
  __shared__ unsigned red[4];
  __shared__ unsigned wsum[4], wmax[4];
  const int s = blockIdx.x, t = threadIdx.x;
  const int g = rle_group_find(geo.first_out, geo.G, s);
  const int H = geo.H[g], W = geo.W[g], HW64 = (H + 63) / 64;
  const unsigned Q = (unsigned)W * (unsigned)HW64;
  const int src_lo = geo.first_src[g], src_hi = geo.first_src[g + 1];
  const long long o0 = member_offsets[s], o1 = member_offsets[s + 1];
  const int lo = bounds[(size_t)s * 2], hi = bounds[(size_t)s * 2 + 1];
  int32_t* row = table + (size_t)s * 4;
  int32_t* st = status + (size_t)s * 4;
  // everything up to the vote is uniform over the workgroup
  bool ok = o0 >= 0 && o0 <= o1 && o1 <= (long long)M;
  const int k = ok ? (int)(o1 - o0) : 0;
  ok = ok && k <= 65535 && lo >= 0 && lo <= hi;
  unsigned worst = 0;      // the largest code among the members; 2 for a member outside the image's own source entries
  if (ok) {
    for (int i = t; i < k; i += RLE_THREADS) {
      const int m = members[o0 + i];
      unsigned code = 2;
      if (m >= src_lo && m < src_hi) {
        const int c = src_status[(size_t)m * 4];
        code = c == 0 ? 0u : (c == 1 ? 1u : 2u);
      }
      worst = worst > code ? worst : code;
    }
    worst = rle_block_max(worst, red);
  }
  if (!ok || worst == 2u) {
    if (t == 0) {
      row[0] = 0; row[1] = 3; row[2] = 0; row[3] = 0;
      st[0] = 2; st[1] = k; st[2] = 0; st[3] = 0;
    }
    return;
  }
  if (t == 0) { st[0] = (int32_t)worst; st[1] = k; st[2] = 0; st[3] = 0; }
  int nb = 0;      // slices: count <= k < 2^nb
  while ((k >> nb) != 0) ++nb;
  const int hic = hi < k ? hi : k;
  const bool none = lo > k;
  const unsigned long long* Ps = src_plane + (size_t)geo.word0_src[g];
  unsigned long long* Pm = merged + (size_t)geo.word0_out[g] + (size_t)(s - geo.first_out[g]) * Q;
  for (unsigned q = t; q < Q; q += RLE_THREADS) {
    unsigned long long in;      // lo <= count <= hi, 64 pixels at once; NB: nb rounded up, the slices above nb stay 0
    if (nb <= 2) in = rle_vote_word<2>(Ps + q, Q, members + o0, k, src_lo, lo, hic);
    else if (nb <= 4) in = rle_vote_word<4>(Ps + q, Q, members + o0, k, src_lo, lo, hic);
    else if (nb <= 8) in = rle_vote_word<8>(Ps + q, Q, members + o0, k, src_lo, lo, hic);
    else in = rle_vote_word<16>(Ps + q, Q, members + o0, k, src_lo, lo, hic);
    const int j = (int)(q % (unsigned)HW64);
    const int nv = H - 64 * j < 64 ? H - 64 * j : 64;
    const unsigned long long valid = nv == 64 ? ~0ull : ((1ull << nv) - 1ull);      // rle_transitions' valid bits
    Pm[q] = none ? 0ull : (in & valid);
  }
  __syncthreads();      // the workgroup's own plane words are written: every thread may read any of them
  rle_write_runs(Pm, H, W, HW64, slots + (size_t)s * (size_t)slot_words, slot_words, row, red, wsum, wmax);
}

// ---- every mask of one set against every mask of another, image by image (hgl_rle_match_device).
//
//   E. rle_match_tile_kernel   a workgroup owns TA x TB = 32 x 64 pairs of one image.  Both sets' planes are in the workspace
//      (A .. D above, the starts kernel with boxes); the tile's words are walked CHUNK = 32 at a time through LDS: As[32][32] and
//      Bs[64][34] 64-bit words.  Lane l of a wave owns B row l and the wave 8 A rows, two words per read (ds_read_b128): the B
//      rows are padded to a stride of 34 words = 68 banks, so the 16 lanes of every lane group of the read (their l mod 16 are all
//      different) start on 16 different 4-bank slots -- unpadded, every lane would start on bank 0 -- and the A words are one
//      address for the whole wave (a broadcast).  A plane word is read from memory once per tile; a pair costs two ANDs and two
//      pop-counts per word.  The columns outside the intersection of (the union of the tile's A boxes) and (the
//      union of its B boxes) are not walked: one side is all zeros there.
//      A call of few tiles (64 x 64 masks are 2) splits every tile's word range over `splits` workgroups, each with a plane of
//      partial counts of its own in the workspace: no atomics, and the sum below does not depend on who finished first.
//      `upper`: both sides are the same set and only the pairs a < b are wanted (G below): a tile that holds none returns at once.
//   F. rle_match_best_kernel   one wave per entry of either set walks its row / column of the image's matrix, sums the partial
//      counts, and keeps the partner with the largest I / D, ratios compared exactly (I1*D2 > I2*D1 in 64 bits), the lowest
//      index on a tie.  The waves of set A write the caller's matrix on the way, every element once.
struct RleBest {
  long long I, D;
  int idx;      // -1: none
};
__device__ __forceinline__ bool rle_best_better(const RleBest& a, const RleBest& b) {      // a takes b's place
  if (a.idx < 0) return false;
  if (b.idx < 0) return true;
  const long long l = a.I * b.D, r = b.I * a.D;      // I < 2^31, D < 2^32
  return l > r || (l == r && a.idx < b.idx);
}

__global__ __launch_bounds__(RLE_THREADS) void rle_match_tile_kernel(const unsigned long long* __restrict__ pa,
                                                                     const unsigned long long* __restrict__ pb,
                                                                     const int32_t* __restrict__ sa, const int32_t* __restrict__ sb,
                                                                     const int32_t* __restrict__ boxa, const int32_t* __restrict__ boxb,
                                                                     const RleMatch geo, int splits, long long pairs,
                                                                     int upper, int32_t* __restrict__ partial) {
  constexpr int TA = RLE_MATCH_TA, TB = RLE_MATCH_TB, CH = RLE_MATCH_CHUNK, PER = TA / 4;      // PER A rows per wave
  __shared__ alignas(16) unsigned long long As[TA][CH];
  __shared__ alignas(16) unsigned long long Bs[TB][CH + 2];      // + 2: rows stay 16-byte aligned and start 4 banks apart
  __shared__ int xr[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned tile = blockIdx.x / (unsigned)splits, z = blockIdx.x % (unsigned)splits;
  const int g = rle_group_find(geo.tile0, geo.G, tile);
  const int fa = geo.first_a[g], fb = geo.first_b[g];
  const int na = geo.first_a[g + 1] - fa, nb = geo.first_b[g + 1] - fb;
  const unsigned tiles_b = ((unsigned)nb + TB - 1) / TB, local = tile - geo.tile0[g];
  const int a0 = (int)(local / tiles_b) * TA, b0 = (int)(local % tiles_b) * TB;
  if (upper && a0 >= b0 + TB) return;      // a set against itself (the mask NMS): no pair a < b in this tile, its counts are never read
  const int HW64 = (geo.H[g] + 63) / 64;
  const unsigned Q = (unsigned)geo.W[g] * (unsigned)HW64;
  // the columns that hold a pixel of one of the tile's A masks and of one of its B masks
  if (wave < 2) {
    const int32_t* st = wave ? sb : sa;
    const int32_t* bx = wave ? boxb : boxa;
    const int e = wave ? b0 + lane : a0 + lane;
    const bool in = wave ? e < nb : (lane < TA && e < na);
    int x0 = 0x7fffffff, x1 = -1;
    if (in) {
      const size_t s = (size_t)(wave ? fb : fa) + e;
      if (st[s * 4] != 2 && st[s * 4 + 1] > 0) { x0 = bx[s * 4]; x1 = bx[s * 4 + 2]; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const int o0 = __shfl_xor(x0, d, 64), o1 = __shfl_xor(x1, d, 64);
      x0 = x0 < o0 ? x0 : o0;
      x1 = x1 > o1 ? x1 : o1;
    }
    if (lane == 0) { xr[2 * wave] = x0; xr[2 * wave + 1] = x1; }
  }
  __syncthreads();
  const int x0 = xr[0] > xr[2] ? xr[0] : xr[2], x1 = xr[1] < xr[3] ? xr[1] : xr[3];
  const unsigned c_lo = x0 <= x1 ? (unsigned)x0 * HW64 : 0u, c_hi = x0 <= x1 ? (unsigned)(x1 + 1) * HW64 : 0u;      // <= Q
  // this workgroup's share of them: whole chunks, the z-th of `splits` equal parts
  const unsigned per = (((c_hi - c_lo + CH - 1) / CH + (unsigned)splits - 1) / (unsigned)splits) * CH;
  const unsigned w_lo = c_lo + z * per < c_hi ? c_lo + z * per : c_hi, w_hi = c_hi - w_lo < per ? c_hi : w_lo + per;
  const unsigned long long* PA = pa + (size_t)geo.word0_a[g];
  const unsigned long long* PB = pb + (size_t)geo.word0_b[g];
  unsigned acc[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) acc[i] = 0;
  // Staging: 8 rows of 32 words per pass, a row is 256 contiguous bytes.  The twelve loads of a chunk go to registers at clamped
  // (always valid) addresses with nothing between them, so they are in flight together, and a chunk is loaded while the one
  // before it is pop-counted; what lies outside the tile or the word range becomes 0 afterwards.
  const int sr = t >> 5, sw = t & 31;
  unsigned long long ra[TA / 8], rb[TB / 8];
  auto fetch = [&](unsigned w0) {      // w0 < w_hi; a0 < na and b0 < nb: the tile exists
    const unsigned w = w0 + sw;
    const bool ok = w < w_hi;
    const unsigned wc = ok ? w : w_hi - 1u;
#pragma unroll
    for (int i = 0; i < TA / 8; ++i) {
      const int r = a0 + sr + 8 * i;
      ra[i] = PA[(size_t)(r < na ? r : a0) * Q + wc];
    }
#pragma unroll
    for (int i = 0; i < TB / 8; ++i) {
      const int r = b0 + sr + 8 * i;
      rb[i] = PB[(size_t)(r < nb ? r : b0) * Q + wc];
    }
  };
  // The values are pinned in their registers, all twelve at once, where they are needed (after the pop-count of the chunk before):
  // left to itself the compiler turns "outside ? 0 : load" back into a branch around every load and waits for each before it
  // issues the next.
  auto settle = [&](unsigned w0) {
    const bool ok = w0 + sw < w_hi;
#pragma unroll
    for (int i = 0; i < TA / 8; ++i) asm volatile("" : "+v"(ra[i]));
#pragma unroll
    for (int i = 0; i < TB / 8; ++i) asm volatile("" : "+v"(rb[i]));
#pragma unroll
    for (int i = 0; i < TA / 8; ++i) ra[i] = (ok && a0 + sr + 8 * i < na) ? ra[i] : 0ull;
#pragma unroll
    for (int i = 0; i < TB / 8; ++i) rb[i] = (ok && b0 + sr + 8 * i < nb) ? rb[i] : 0ull;
  };
  if (w_lo < w_hi) fetch(w_lo);
  for (unsigned w0 = w_lo; w0 < w_hi; w0 += CH) {
    settle(w0);
#pragma unroll
    for (int i = 0; i < TA / 8; ++i) As[sr + 8 * i][sw] = ra[i];
#pragma unroll
    for (int i = 0; i < TB / 8; ++i) Bs[sr + 8 * i][sw] = rb[i];
    __syncthreads();
    if (w0 + CH < w_hi) fetch(w0 + CH);      // uniform over the workgroup; settled and stored after the barrier below
#pragma unroll 4
    for (int k = 0; k < CH; ++k) {
      const unsigned long long b = Bs[lane][k];
#pragma unroll
      for (int i = 0; i < PER; ++i) acc[i] += __popcll(As[wave * PER + i][k] & b);
    }
    __syncthreads();      // the next chunk overwrites As / Bs
  }
  const int b = b0 + lane;
  if (b >= nb) return;
  int32_t* P = partial + (size_t)z * (size_t)pairs + geo.pair0[g];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int a = a0 + wave * PER + i;
    if (a < na) P[(size_t)a * nb + b] = (int32_t)acc[i];      // <= H*W < 2^31; every element of every plane is written
  }
}

// blocks 0 .. Sa-1: the entries of A over their rows; Sa .. Sa+Sb-1: the entries of B over their columns.  One wave each.
// inter: the caller's matrices (null: not wanted), written by the waves of A: -1 in the row / column of an entry of code 2.
__global__ __launch_bounds__(64) void rle_match_best_kernel(const int32_t* __restrict__ sa, const int32_t* __restrict__ sb,
                                                            const uint8_t* __restrict__ crowd_b, const RleMatch geo, int splits,
                                                            long long pairs, const int32_t* __restrict__ partial,
                                                            int32_t* __restrict__ inter, int32_t* __restrict__ match_a,
                                                            int32_t* __restrict__ match_b) {
  const int Sa = geo.first_a[geo.G], lane = threadIdx.x;
  const bool side_b = (int)blockIdx.x >= Sa;
  const int s = side_b ? (int)blockIdx.x - Sa : (int)blockIdx.x;
  const int g = rle_group_find(side_b ? geo.first_b : geo.first_a, geo.G, s);
  const int fa = geo.first_a[g], fb = geo.first_b[g];
  const int na = geo.first_a[g + 1] - fa, nb = geo.first_b[g + 1] - fb;
  const int32_t* self = (side_b ? sb : sa) + (size_t)s * 4;
  int32_t* out = (side_b ? match_b : match_a) + (size_t)s * 4;
  const int code = self[0], area = self[1];
  const int k = s - (side_b ? fb : fa), n = side_b ? na : nb;
  int32_t* row = (!side_b && inter) ? inter + geo.off[g] + (size_t)k * nb : nullptr;
  if (code == 2) {      // uniform over the wave
    if (row)
      for (int j = lane; j < n; j += 64) row[j] = -1;
    if (lane == 0) { out[0] = 2; out[1] = 0; out[2] = -1; out[3] = 0; }
    return;
  }
  const int32_t* P = partial + geo.pair0[g];
  const bool crowd_self = side_b && crowd_b && crowd_b[s];
  RleBest best = {0, 1, -1};
  for (int j = lane; j < n; j += 64) {
    const int32_t* other = side_b ? sa + (size_t)(fa + j) * 4 : sb + (size_t)(fb + j) * 4;
    const bool dead = other[0] == 2;
    const size_t e = side_b ? (size_t)j * nb + k : (size_t)k * nb + j;
    long long I = 0;
    for (int z = 0; z < splits; ++z) I += P[(size_t)z * (size_t)pairs + e];
    if (row) row[j] = dead ? -1 : (int32_t)I;
    if (dead || I <= 0) continue;      // a partner that holds no mask, or no common pixel
    const long long area_a = side_b ? other[1] : area, area_b = side_b ? area : other[1];
    const bool crowd = side_b ? crowd_self : (crowd_b && crowd_b[fb + j]);
    const RleBest c = {I, crowd ? area_a : area_a + area_b - I, j};
    if (rle_best_better(c, best)) best = c;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const RleBest o = {__shfl_xor(best.I, d, 64), __shfl_xor(best.D, d, 64), __shfl_xor(best.idx, d, 64)};
    if (rle_best_better(o, best)) best = o;
  }
  if (lane == 0) { out[0] = code; out[1] = area; out[2] = best.idx; out[3] = (int32_t)best.I; }
}

// ---- greedy suppression by mask overlap inside one set, image by image (hgl_rle_nms_device): rleNms of maskApi.c:98-107 on the
// planes, with the box NMS's order (nms_walk.h).  The set goes through A, B, D and E once (pa == pb, the tiles above the
// diagonal), then:
//
//   G. rle_nms_rank_kernel    one thread per entry counts the entries of its image that come before it (nms_before; without
//      scores every score is equal and the index decides: the given order).  An entry of code 2 takes a place behind every
//      entry that holds a mask, so order[] is a permutation of the image's list and nothing downstream reads an unwritten index.
//   H. rle_nms_words_kernel   one wave per suppression word: lane j decides column rank 64 w + j against row rank q from the
//      summed partial counts and the two areas, in double; the word is the wave's ballot.  Words left of a row's diagonal block
//      are neither written nor read.
//   I. rle_nms_walk_kernel    one workgroup per image walks the 64-row blocks: wave 0 resolves the diagonal block
//      (nms_resolve_block, nms_emit_block), then every later word of removed[] takes the OR of the block's kept rows, one wave per
//      word with a lane per kept row; the column's first suppressor is the lowest lane whose word names it.
struct RleNmsEntry {
  int g, f, n;      // image, its first entry, its entries
};
__device__ __forceinline__ RleNmsEntry rle_nms_image(const RleNms& geo, int g) { return {g, geo.first[g], geo.first[g + 1] - geo.first[g]}; }

__global__ __launch_bounds__(RLE_THREADS) void rle_nms_rank_kernel(const int32_t* __restrict__ status, const float* __restrict__ scores,
                                                                   const RleNms geo, int32_t* __restrict__ order,
                                                                   int32_t* __restrict__ result) {
  const int s = blockIdx.x * RLE_THREADS + threadIdx.x;
  if (s >= geo.first[geo.G]) return;
  const RleNmsEntry im = rle_nms_image(geo, rle_group_find(geo.first, geo.G, s));
  const int i = s - im.f;
  const int code = status[(size_t)s * 4], area = status[(size_t)s * 4 + 1];
  const float si = scores ? scores[s] : 0.f;
  int before = 0, valid = 0, dead_lower = 0;
  for (int j = 0; j < im.n; ++j) {
    const bool ok = status[(size_t)(im.f + j) * 4] != 2;
    const float sj = scores ? scores[im.f + j] : 0.f;
    valid += ok ? 1 : 0;
    before += (ok && nms_before(sj, j, si, i)) ? 1 : 0;
    dead_lower += (!ok && j < i) ? 1 : 0;
  }
  order[im.f + (code != 2 ? before : valid + dead_lower)] = i;
  int32_t* row = result + (size_t)s * 4;
  row[0] = code; row[1] = area; row[2] = code != 2 ? before : -1; row[3] = -1;
}

// does the pair of I common pixels and these areas (both > 0) exceed thr?  metric 0: I / union, 1: I / the smaller area
__device__ __forceinline__ bool rle_nms_exceeds(long long I, long long area_a, long long area_b, double thr, int metric) {
  const long long D = metric == 0 ? area_a + area_b - I : (area_a < area_b ? area_a : area_b);
  const double ratio = I == 0 ? 0.0 : (double)I / (double)D;
  return ratio > thr;
}

__global__ __launch_bounds__(RLE_THREADS) void rle_nms_words_kernel(const int32_t* __restrict__ status, const int32_t* __restrict__ order,
                                                                    const int32_t* __restrict__ partial, const RleNms geo, int splits,
                                                                    long long pairs, long long sup_words, double thr, int metric,
                                                                    unsigned long long* __restrict__ sup) {
  const int lane = threadIdx.x & 63;
  const long long u = (long long)blockIdx.x * (RLE_THREADS / 64) + (threadIdx.x >> 6);
  if (u >= sup_words) return;      // uniform over the wave, as everything up to the ballot
  const RleNmsEntry im = rle_nms_image(geo, rle_group_find(geo.sup0, geo.G, u));
  const int nw = (im.n + 63) >> 6;
  const long long local = u - geo.sup0[im.g];
  const int q = (int)(local / nw), w = (int)(local % nw);
  if (w < (q >> 6)) return;
  const int a = order[im.f + q];
  const int32_t* sa = status + (size_t)(im.f + a) * 4;
  const bool row_ok = sa[0] != 2 && sa[1] > 0;
  const int c = 64 * w + lane;
  bool bit = false;
  if (row_ok && c > q && c < im.n) {
    const int b = order[im.f + c];
    const int32_t* sb = status + (size_t)(im.f + b) * 4;
    if (sb[0] != 2 && sb[1] > 0) {
      const int lo = a < b ? a : b, hi = a < b ? b : a;      // the tile kernel counted the pairs lo < hi
      const int32_t* P = partial + geo.pair0[im.g] + (size_t)lo * im.n + hi;
      long long I = 0;
      for (int z = 0; z < splits; ++z) I += P[(size_t)z * (size_t)pairs];
      bit = rle_nms_exceeds(I, sa[1], sb[1], thr, metric);
    }
  }
  const unsigned long long word = __ballot(bit);
  if (lane == 0) sup[u] = word;
}

__global__ __launch_bounds__(RLE_THREADS) void rle_nms_walk_kernel(const int32_t* __restrict__ status, const int32_t* __restrict__ order,
                                                                   const unsigned long long* __restrict__ sup, const RleNms geo,
                                                                   int32_t* __restrict__ out_idx, int32_t* __restrict__ out_n,
                                                                   int32_t* __restrict__ result) {
  __shared__ int by_rank[RLE_NMS_MAX];                       // the rank of the column's first suppressor, -1: none
  __shared__ unsigned long long removed[RLE_NMS_MAX / 64];
  __shared__ unsigned long long kept_word;
  __shared__ int nkept_s;
  __shared__ int red[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const RleNmsEntry im = rle_nms_image(geo, (int)blockIdx.x);
  if (im.n == 0) {      // uniform over the workgroup
    if (t == 0) out_n[im.g] = 0;
    return;
  }
  // the entries that hold a mask take the ranks 0 .. nv-1
  int mine = 0;
  for (int j = t; j < im.n; j += RLE_THREADS) mine += status[(size_t)(im.f + j) * 4] != 2 ? 1 : 0;
  const int nv = rle_block_sum(mine, red);
  const int nw = (im.n + 63) >> 6, nblk = (nv + 63) >> 6;
  for (int c = t; c < im.n; c += RLE_THREADS) by_rank[c] = -1;
  if (t < nw) removed[t] = 0;
  if (t == 0) nkept_s = 0;
  __syncthreads();
  const int* ord = order + im.f;
  const unsigned long long* words = sup + geo.sup0[im.g];
  for (int rb = 0; rb < nblk; ++rb) {
    if (wave == 0) {
      const int a = rb * 64 + lane;
      const unsigned long long d = a < nv ? words[(size_t)a * nw + rb] : 0ull, rem = removed[rb];
      const unsigned long long km = nms_resolve_block(d, rem, rb, nv);
      nms_emit_block(km, rb, lane, ord, out_idx + im.f, nkept_s, kept_word);
      // a column of this block that falls here: the first kept row whose diagonal word names it
      int first = -1;
      for (int s2 = 0; s2 < 64; ++s2) {
        const unsigned lo = __shfl((unsigned)(d & 0xffffffffull), s2), hi = __shfl((unsigned)(d >> 32), s2);
        const unsigned long long row = ((unsigned long long)hi << 32) | lo;
        if (first < 0 && ((km >> s2) & 1ull) && ((row >> lane) & 1ull)) first = rb * 64 + s2;
      }
      if (a < nv && !((rem >> lane) & 1ull) && first >= 0) by_rank[a] = first;
    }
    __syncthreads();
    const unsigned long long km = kept_word;
    for (int w = rb + 1 + wave; w < nblk; w += RLE_THREADS / 64) {      // uniform over the wave
      const unsigned long long v = ((km >> lane) & 1ull) ? words[(size_t)(rb * 64 + lane) * nw + w] : 0ull;
      unsigned long long who = 0;      // lane j: the kept rows of the block that name column 64 w + j
      for (int j = 0; j < 64; ++j) {
        const unsigned long long b = __ballot((v >> j) & 1ull);
        if (lane == j) who = b;
      }
      const unsigned long long old = removed[w];
      if (who && !((old >> lane) & 1ull)) by_rank[64 * w + lane] = rb * 64 + (__ffsll((long long)who) - 1);
      const unsigned long long fresh = __ballot(who != 0);
      if (lane == 0) removed[w] = old | fresh;
    }
    __syncthreads();
  }
  for (int c = t; c < nv; c += RLE_THREADS)
    if (by_rank[c] >= 0) result[(size_t)(im.f + ord[c]) * 4 + 3] = ord[by_rank[c]];
  if (t == 0) out_n[im.g] = nkept_s;
}

// ---- the kept entries of a set, compacted image by image into a second set (hgl_rle_select_device).  Nothing is decoded: an
// entry moves as the words its table row defines.
//
//   J. rle_select_rank_kernel   one workgroup per image.  The image's entries are taken RLE_THREADS at a time in stored order:
//      a wave's ballot of the keep flags gives every lane the kept entries before it in the wave (a pop-count below the lane),
//      the four wave totals cross in LDS, the chunks' total is carried in a register.  A kept entry of rank r < max_keep writes
//      out_src[e + r] = its index; the positions from k = min(kept, max_keep) on receive -1, out_n[g] = k.
//   K. rle_select_move_kernel   one wave per (destination entry, chunk of RLE_SELECT_CHUNK slot words): the lanes share the
//      entry's words, 16 bytes a lane and pass where the plan found both buffers aligned (WIDE), 4 otherwise; chunk 0 also
//      carries the table row and the side columns.  A placeholder (out_src < 0) is the row (1, 0, 0, 0) and the one count H*W.
__device__ __forceinline__ bool rle_select_kept(const uint8_t* __restrict__ keep, const int32_t* __restrict__ nms, int s) {
  if (keep) return keep[s] != 0;
  const int32_t* r = nms + (size_t)s * 4;
  return (r[0] == 0 || r[0] == 1) && r[3] == -1;
}

__global__ __launch_bounds__(RLE_THREADS) void rle_select_rank_kernel(const uint8_t* __restrict__ keep, const int32_t* __restrict__ nms,
                                                                      const RleSelect geo, int32_t* __restrict__ out_src,
                                                                      int32_t* __restrict__ out_n) {
  __shared__ int wcnt[2][RLE_THREADS / 64];      // two sets: a chunk's totals are read while the next chunk's are written
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int g = (int)blockIdx.x, f = geo.first[g], n = geo.first[g + 1] - f, limit = geo.max_keep[g];
  int base = 0;      // kept entries of the chunks before this one: the same in every thread
  for (int c0 = 0, it = 0; c0 < n; c0 += RLE_THREADS, ++it) {      // uniform over the workgroup
    const int i = c0 + t;
    const bool k = i < n && rle_select_kept(keep, nms, f + i);
    const unsigned long long b = __ballot(k);
    if (lane == 0) wcnt[it & 1][wave] = __popcll(b);
    __syncthreads();
    int r = base + __popcll(b & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < RLE_THREADS / 64; ++w) {
      const int v = wcnt[it & 1][w];
      r += w < wave ? v : 0;
      total += v;
    }
    if (k && r < limit) out_src[f + r] = i;      // r < limit <= n
    base += total;
  }
  const int kept = base < limit ? base : limit;
  for (int p = kept + t; p < n; p += RLE_THREADS) out_src[f + p] = -1;
  if (t == 0) out_n[g] = kept;
}

template <bool WIDE>
__global__ __launch_bounds__(64 * RLE_SELECT_WAVES) void rle_select_move_kernel(
    const uint32_t* __restrict__ slots, long long slot_words, const int32_t* __restrict__ table, const uint32_t* __restrict__ cols, int C,
    const RleSelect geo, long long chunks, const int32_t* __restrict__ out_src, uint32_t* __restrict__ out_slots,
    int32_t* __restrict__ out_table, uint32_t* __restrict__ out_cols) {
  const int lane = threadIdx.x & 63, S = geo.first[geo.G];
  const long long blk = (long long)blockIdx.x;
  const int d = (int)(blk / chunks) * RLE_SELECT_WAVES + (int)(threadIdx.x >> 6);      // the destination entry: uniform over the wave
  const long long w0 = (blk % chunks) * RLE_SELECT_CHUNK;                               // the chunk's first word
  if (d >= S) return;
  const int g = rle_group_find(geo.first, geo.G, d);
  const int src = out_src[d];
  uint32_t* dst = out_slots + (size_t)d * (size_t)slot_words;
  if (src < 0) {      // a placeholder: an empty mask of the image's size
    if (w0 == 0 && lane == 0) {
      int32_t* row = out_table + (size_t)d * 4;
      row[0] = 1; row[1] = 0; row[2] = 0; row[3] = 0;
      dst[0] = (uint32_t)geo.H[g] * (uint32_t)geo.W[g];      // slot_words >= 1 (the plan)
    }
    if (w0 == 0 && lane < C) out_cols[(size_t)lane * S + d] = 0u;
    return;
  }
  const int s = geo.first[g] + src;      // src < n_g: the rank kernel wrote an index of the image's list
  const int32_t* row = table + (size_t)s * 4;
  const int n = row[0], form = row[1];
  if (w0 == 0) {
    if (lane < 4) out_table[(size_t)d * 4 + lane] = row[lane];
    if (lane < C) out_cols[(size_t)lane * S + d] = cols[(size_t)lane * S + s];
  }
  const unsigned plane_words = ((unsigned)geo.H[g] * (unsigned)geo.W[g] + 31u) / 32u;
  if (!rle_entry_usable(n, form, slot_words, plane_words)) return;      // the row describes no mask: no slot word moves
  const long long words = form == 0 ? (long long)n : (long long)plane_words;      // <= slot_words
  const long long w1 = words < w0 + RLE_SELECT_CHUNK ? words : w0 + RLE_SELECT_CHUNK;      // this chunk: [w0, w1)
  const uint32_t* from = slots + (size_t)s * (size_t)slot_words;
  long long w = w0;
  if (WIDE) {      // both rows start 16-byte aligned and so does the chunk (RLE_SELECT_CHUNK % 4 == 0)
    const long long quads = w1 > w0 ? (w1 - w0) / 4 : 0;
    const uint4* from4 = reinterpret_cast<const uint4*>(from + w0);
    uint4* dst4 = reinterpret_cast<uint4*>(dst + w0);
    for (long long q = lane; q < quads; q += 64) dst4[q] = from4[q];
    w = w0 + 4 * quads;      // up to 3 words remain
  }
  for (long long q = w + lane; q < w1; q += 64) dst[q] = from[q];
}

// the staged set's arrays; the two launches that fill them when the set has an entry (`blocks`: the plane kernel's grid).  SG is
// the starts kernel's geometry and PG the plane kernel's: RleSet for both, or RleOne and RlePlaneOne.
struct RleStaged {
  uint32_t* E;
  int32_t *status, *boxes;      // boxes: null when the carve has none
  unsigned long long* plane;
};
template <class SG, class PG>
RleStaged rle_stage_launch(const uint32_t* slots, long long slot_words, const int32_t* table, int S, long long blocks, const SG& sgeo,
                           const PG& pgeo, char* base, const RleStageWs& w, hipStream_t st) {
  const RleStaged d = {(uint32_t*)(base + w.E), (int32_t*)(base + w.status), w.boxes != RLE_NO_BOXES ? (int32_t*)(base + w.boxes) : nullptr,
                       (unsigned long long*)(base + w.plane)};
  if (S == 0) return d;
  auto starts = d.boxes ? rle_starts_kernel<true, SG> : rle_starts_kernel<false, SG>;
  hipLaunchKernelGGL(starts, dim3((unsigned)S), dim3(RLE_THREADS), 0, st, slots, slot_words, table, sgeo, d.E, slot_words + 1, d.status,
                     d.boxes);
  hipLaunchKernelGGL(rle_plane_kernel<PG>, dim3((unsigned)blocks), dim3(RLE_THREADS), 0, st, slots, slot_words, table,
                     (const uint32_t*)d.E, slot_words + 1, (const int32_t*)d.status, pgeo, d.plane);
  return d;
}

// the workspace of a pairwise IoU: either side, S entries of one size, staged without boxes
struct RleIouWs {
  RleStageWs side[2];
  size_t total;
};
RleIouWs rle_iou_ws(int S, int H, int W, long long swa, long long swb) {
  RleIouWs w;
  const long long words = (long long)S * W * ((H + 63) / 64);      // <= S*H*W
  w.total = 0;
  w.side[0] = rle_stage_ws(&w.total, S, swa, words, false);
  w.side[1] = rle_stage_ws(&w.total, S, swb, words, false);
  return w;
}

// the workspace of a match: either side staged with boxes; the planes of partial counts, one per split
struct RleMatchWs {
  RleStageWs side[2];
  size_t partial, total;
};
size_t rle_partial_bytes(const RlePairs& p) { return hgl_align_up((size_t)p.splits * (size_t)p.pairs * sizeof(int32_t), 256); }
RleMatchWs rle_match_ws(const RleMatchPlan& plan, int Sa, long long swa, int Sb, long long swb) {
  RleMatchWs w;
  size_t p = 0;
  w.side[0] = rle_stage_ws(&p, Sa, swa, plan.a.words, true);
  w.side[1] = rle_stage_ws(&p, Sb, swb, plan.b.words, true);
  w.partial = p;
  w.total = p + rle_partial_bytes(plan.p);
  return w;
}

// the workspace of a mask NMS: the one set staged with boxes; the planes of partial counts; order; suppression words
struct RleNmsWs {
  RleStageWs set;
  size_t partial, order, sup, total;
};
RleNmsWs rle_nms_ws(const RleNmsPlan& plan, int S, long long sw) {
  RleNmsWs w;
  size_t p = 0;
  w.set = rle_stage_ws(&p, S, sw, plan.set.words, true);
  w.partial = p;
  p += rle_partial_bytes(plan.p);
  w.order = p;
  p += hgl_align_up((size_t)S * sizeof(int32_t), 256);
  w.sup = p;
  w.total = p + hgl_align_up((size_t)plan.sup_words * sizeof(unsigned long long), 256);
  return w;
}

// the workspace of a merge: the source set staged without boxes, then the merged planes
struct RleMergeWs {
  RleStageWs src;
  size_t merged, total;
};
RleMergeWs rle_merge_ws(const RleMergePlan& plan, int Ssrc, long long sw) {
  RleMergeWs w;
  size_t p = 0;
  w.src = rle_stage_ws(&p, Ssrc, sw, plan.src.words, false);
  w.merged = p;
  w.total = p + hgl_align_up((size_t)plan.words_out * sizeof(unsigned long long), 256);
  return w;
}

// the one decode: plan the images' geometry (-1), check the workspace (-3), two launches; boxes: null for none
int rle_decode_launch(const char* name, const uint32_t* slots, long long slot_words, const int32_t* table, int S,
                      const int64_t* images, int G, uint8_t* masks, long long masks_bytes, int32_t* boxes, int32_t* status, void* ws,
                      size_t ws_bytes, void* stream) {
  RleGroup grp;
  long long tiles = 0;
  char why[200];
  if (rle_group_plan(images, G, S, (uintptr_t)masks, masks_bytes, &grp, &tiles, why, sizeof(why)) != 0) {
    hgl_set_error("%s: %s", name, why);
    return HGL_EINVAL;
  }
  if (!ws || ws_bytes < rle_starts_bytes(S, slot_words)) {
    hgl_set_error("%s: workspace too small", name);
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  uint32_t* E = (uint32_t*)ws;
  const long long e_stride = slot_words + 1;
  const unsigned long long all = G == RLE_GROUP_MAX ? ~0ull : (1ull << G) - 1ull;
  // V: one store path for all G images -> the kernel that holds only that path; the choice per image otherwise
  auto launch = [&](auto geo, uint8_t* base) {
    using GEO = decltype(geo);
    auto starts = boxes ? rle_starts_kernel<true, GEO> : rle_starts_kernel<false, GEO>;
    hipLaunchKernelGGL(starts, dim3((unsigned)S), dim3(RLE_THREADS), 0, st, slots, slot_words, table, geo, E, e_stride, status, boxes);
    auto rows = grp.wide == all ? rle_rows_kernel<4, GEO> : rle_rows_kernel<1, GEO>;
    if constexpr (std::is_same<GEO, RleGroup>::value)
      if (grp.wide != all && grp.wide != 0) rows = rle_rows_kernel<0, GEO>;
    hipLaunchKernelGGL(rows, dim3((unsigned)tiles), dim3(RLE_THREADS), 0, st, slots, slot_words, table, (const uint32_t*)E, e_stride,
                       (const int32_t*)status, geo, base);
  };
  const RleTiles one = rle_tiles(grp.H[0], grp.W[0], (uintptr_t)masks + (uintptr_t)grp.off[0]);
  if (G == 1)
    launch(RleOne{grp.H[0], grp.W[0], one.HW64, one.col_tiles, one.row_tiles}, masks + grp.off[0]);
  else
    launch(grp, masks);
  return hgl_check_launch(name);
}

}  // namespace

// rle_scan.h: the staging of a set for a caller in another file (rle_clean.hip): rle_stage_launch on a carve without boxes,
// its offsets taken from E
void rle_stage_set(const uint32_t* slots, long long slot_words, const int32_t* table, int S, const RleSet& set, uint32_t* E,
                   int32_t* status, unsigned long long* plane, void* stream) {
  char* base = (char*)E;
  const RleStageWs w = {0, (size_t)((char*)status - base), RLE_NO_BOXES, (size_t)((char*)plane - base)};
  rle_stage_launch(slots, slot_words, table, S, set.blocks, set, set, base, w, (hipStream_t)stream);
}

// rle_scan.h: the staging of a paint list for rle_paint.hip: the starts kernel without boxes and the plane kernel over the K list
// positions, each reading the entry it names; status is the caller's own [K,4].  K > 0.
void rle_stage_picked(const uint32_t* slots, long long slot_words, const int32_t* table, int K, const RlePick& pick, uint32_t* E,
                      int32_t* status, unsigned long long* plane, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((rle_starts_kernel<false, RlePick>), dim3((unsigned)K), dim3(RLE_THREADS), 0, st, slots, slot_words, table, pick, E,
                     slot_words + 1, status, (int32_t*)nullptr);
  hipLaunchKernelGGL(rle_plane_kernel<RlePick>, dim3((unsigned)pick.pos.blocks), dim3(RLE_THREADS), 0, st, slots, slot_words, table,
                     (const uint32_t*)E, slot_words + 1, (const int32_t*)status, pick, plane);
}

extern "C" {

size_t hgl_rle_encode_workspace_bytes(int S, int H, int W) {
  if (S <= 0 || H <= 0 || W <= 0) return 0;
  return hgl_align_up((size_t)S * (size_t)W * (size_t)((H + 63) / 64) * sizeof(unsigned long long), 256);
}

int hgl_rle_encode_device(const uint8_t* masks, int N, int H, int W, const int64_t* sel, int S, uint32_t* slots,
                          long long slot_words, int32_t* table, void* ws, size_t ws_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(masks && slots && table && N > 0 && H > 0 && W > 0 && S > 0 && slot_words >= 0, "rle_encode_device: bad arguments");
  HGL_REQUIRE(sel || S <= N, "rle_encode_device: without an index tensor S (%d) must not exceed N (%d)", S, N);
  HGL_REQUIRE((long long)N * H * W < (1ll << 31), "rle_encode_device: batch too large (N*H*W must be < 2^31)");
  const RleTiles t = rle_tiles(H, W, (uintptr_t)masks);
  const long long tiles = (long long)S * t.col_tiles * t.row_tiles;
  HGL_REQUIRE(tiles < (1ll << 31), "rle_encode_device: too many entries (%d) for one launch", S);
  if (!ws || ws_bytes < hgl_rle_encode_workspace_bytes(S, H, W)) {
    hgl_set_error("rle_encode_device: workspace too small");
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* plane = (unsigned long long*)ws;
  const long long* sel64 = (const long long*)sel;
  if (t.wide)
    hipLaunchKernelGGL(rle_columns_kernel<4>, dim3((unsigned)tiles), dim3(RLE_THREADS), 0, st, masks, N, H, W, sel64, t.HW64,
                       t.col_tiles, t.row_tiles, plane);
  else
    hipLaunchKernelGGL(rle_columns_kernel<1>, dim3((unsigned)tiles), dim3(RLE_THREADS), 0, st, masks, N, H, W, sel64, t.HW64,
                       t.col_tiles, t.row_tiles, plane);
  hipLaunchKernelGGL(rle_runs_kernel, dim3((unsigned)S), dim3(RLE_THREADS), 0, st, (const unsigned long long*)plane, N, H, W,
                     sel64, t.HW64, slots, slot_words, table);
  return hgl_check_launch("rle_encode_device");
}

size_t hgl_rle_decode_workspace_bytes(int S, int H, int W, long long slot_words) {
  if (S <= 0 || H <= 0 || W <= 0 || slot_words < 0) return 0;
  return rle_starts_bytes(S, slot_words);
}

int hgl_rle_decode_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S, int H, int W, uint8_t* masks,
                          int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(slots && table && masks && status && S > 0 && H > 0 && W > 0 && slot_words >= 0, "rle_decode_device: bad arguments");
  HGL_REQUIRE((long long)H * W < (1ll << 31), "rle_decode_device: image too large (H*W must be < 2^31)");
  HGL_REQUIRE((long long)S * H * W < (1ll << 31), "rle_decode_device: batch too large (S*H*W must be < 2^31)");
  const int64_t image[4] = {H, W, 0, 0};      // a group of one: every entry is this image's, from byte 0 on
  return rle_decode_launch("rle_decode_device", slots, slot_words, table, S, image, 1, masks, (long long)S * H * W, nullptr, status,
                           ws, ws_bytes, stream);
}

size_t hgl_rle_decode_group_workspace_bytes(int S, long long slot_words) {
  if (S <= 0 || slot_words < 0) return 0;
  return rle_starts_bytes(S, slot_words);
}

int hgl_rle_decode_group_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S,
                                const int64_t* images_host, int G, uint8_t* masks, long long masks_bytes, int32_t* boxes_xyxy,
                                int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(slots && table && images_host && masks && boxes_xyxy && status && S > 0 && slot_words >= 0 && masks_bytes >= 0,
              "rle_decode_group_device: bad arguments");
  return rle_decode_launch("rle_decode_group_device", slots, slot_words, table, S, images_host, G, masks, masks_bytes, boxes_xyxy,
                           status, ws, ws_bytes, stream);
}

size_t hgl_rle_iou_workspace_bytes(int S, int H, int W, long long slot_words_a, long long slot_words_b) {
  if (S <= 0 || H <= 0 || W <= 0 || slot_words_a < 0 || slot_words_b < 0) return 0;
  return rle_iou_ws(S, H, W, slot_words_a, slot_words_b).total;
}

int hgl_rle_iou_device(const uint32_t* slots_a, long long slot_words_a, const int32_t* table_a, const uint32_t* slots_b,
                       long long slot_words_b, const int32_t* table_b, int S, int H, int W, int64_t* iu, void* ws, size_t ws_bytes,
                       void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(slots_a && table_a && slots_b && table_b && iu && S > 0 && H > 0 && W > 0 && slot_words_a >= 0 && slot_words_b >= 0,
              "rle_iou_device: bad arguments");
  HGL_REQUIRE((long long)H * W < (1ll << 31), "rle_iou_device: image too large (H*W must be < 2^31)");
  HGL_REQUIRE((long long)S * H * W < (1ll << 31), "rle_iou_device: batch too large (S*H*W must be < 2^31)");
  const int HW64 = (H + 63) / 64;
  const unsigned Q = (unsigned)W * (unsigned)HW64;
  const int q_tiles = (int)((Q + RLE_THREADS - 1) / RLE_THREADS);
  HGL_REQUIRE((long long)S * q_tiles < (1ll << 31), "rle_iou_device: too many entries (%d) for one launch", S);
  const RleIouWs w = rle_iou_ws(S, H, W, slot_words_a, slot_words_b);
  if (!ws || ws_bytes < w.total) {
    hgl_set_error("rle_iou_device: workspace too small");
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const RleOne one = {H, W, HW64, 0, 0};
  const RlePlaneOne pone = {H, W, HW64, q_tiles};
  const RleStaged a = rle_stage_launch(slots_a, slot_words_a, table_a, S, (long long)S * q_tiles, one, pone, (char*)ws, w.side[0], st);
  const RleStaged b = rle_stage_launch(slots_b, slot_words_b, table_b, S, (long long)S * q_tiles, one, pone, (char*)ws, w.side[1], st);
  hipLaunchKernelGGL(rle_iou_kernel, dim3((unsigned)S), dim3(RLE_THREADS), 0, st, (const unsigned long long*)a.plane,
                     (const unsigned long long*)b.plane, (const int32_t*)a.status, (const int32_t*)b.status, Q, (long long*)iu);
  return hgl_check_launch("rle_iou_device");
}

size_t hgl_rle_match_workspace_bytes(const int64_t* images_host, int G, int Sa, long long slot_words_a, int Sb, long long slot_words_b,
                                     int want_inter) {
  if (!images_host || slot_words_a < 0 || slot_words_b < 0) return 0;
  RleMatchPlan plan;
  char why[200];
  // the caller's extents are the call's business: here only the geometry counts
  if (rle_match_plan(images_host, G, Sa, Sb, -1, &plan, why, sizeof(why)) != 0) return 0;
  (void)want_inter;      // the partial counts live in the workspace either way
  return rle_match_ws(plan, Sa, slot_words_a, Sb, slot_words_b).total;
}

int hgl_rle_match_device(const uint32_t* slots_a, long long slot_words_a, const int32_t* table_a, int Sa, const uint32_t* slots_b,
                         long long slot_words_b, const int32_t* table_b, int Sb, const int64_t* images_host, int G,
                         const uint8_t* crowd_b, int32_t* inter, long long inter_elems, int32_t* match_a, int32_t* match_b, void* ws,
                         size_t ws_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(images_host && Sa >= 0 && Sb >= 0 && slot_words_a >= 0 && slot_words_b >= 0 && (Sa == 0 || (slots_a && table_a && match_a)) &&
                  (Sb == 0 || (slots_b && table_b && match_b)) && (!inter || inter_elems >= 0),
              "rle_match_device: bad arguments");
  RleMatchPlan plan;
  char why[200];
  if (rle_match_plan(images_host, G, Sa, Sb, inter ? inter_elems : -1, &plan, why, sizeof(why)) != 0) {
    hgl_set_error("rle_match_device: %s", why);
    return HGL_EINVAL;
  }
  const RleMatchWs w = rle_match_ws(plan, Sa, slot_words_a, Sb, slot_words_b);
  if (w.total > 0 && (!ws || ws_bytes < w.total)) {
    hgl_set_error("rle_match_device: workspace too small");
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  // a side, a kernel or a matrix without an element has no launch; otherwise six launches whatever G and the sizes are
  const RleStaged a = rle_stage_launch(slots_a, slot_words_a, table_a, Sa, plan.a.blocks, plan.a, plan.a, base, w.side[0], st);
  const RleStaged b = rle_stage_launch(slots_b, slot_words_b, table_b, Sb, plan.b.blocks, plan.b, plan.b, base, w.side[1], st);
  const RlePairs& pr = plan.p;
  int32_t* partial = (int32_t*)(base + w.partial);
  if (pr.tiles > 0)      // tiles * splits <= max(tiles, RLE_MATCH_BLOCKS + tiles) < 2^31 + 1024
    hipLaunchKernelGGL(rle_match_tile_kernel, dim3((unsigned)(pr.tiles * pr.splits)), dim3(RLE_THREADS), 0, st,
                       (const unsigned long long*)a.plane, (const unsigned long long*)b.plane, (const int32_t*)a.status,
                       (const int32_t*)b.status, (const int32_t*)a.boxes, (const int32_t*)b.boxes, pr.m, pr.splits, pr.pairs, 0, partial);
  if (Sa + Sb > 0)
    hipLaunchKernelGGL(rle_match_best_kernel, dim3((unsigned)Sa + (unsigned)Sb), dim3(64), 0, st, (const int32_t*)a.status,
                       (const int32_t*)b.status, crowd_b, pr.m, pr.splits, pr.pairs, (const int32_t*)partial, inter, match_a, match_b);
  return hgl_check_launch("rle_match_device");
}

size_t hgl_rle_nms_workspace_bytes(const int64_t* images_host, int G, int S, long long slot_words) {
  if (!images_host || slot_words < 0 || S <= 0) return 0;
  RleNmsPlan plan;
  char why[200];
  if (rle_nms_plan(images_host, G, S, &plan, why, sizeof(why)) != 0) return 0;
  return rle_nms_ws(plan, S, slot_words).total;
}

int hgl_rle_nms_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S, const int64_t* images_host, int G,
                       const float* scores, double thr, int metric, int32_t* out_idx, int32_t* out_n, int32_t* result, void* ws,
                       size_t ws_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(images_host && S >= 0 && slot_words >= 0 && (S == 0 || (slots && table && out_idx && out_n && result)),
              "rle_nms_device: bad arguments");
  HGL_REQUIRE(thr == thr, "rle_nms_device: the threshold is NaN");
  HGL_REQUIRE(metric == 0 || metric == 1, "rle_nms_device: metric %d (0 = IoU, 1 = containment)", metric);
  RleNmsPlan plan;
  char why[200];
  if (rle_nms_plan(images_host, G, S, &plan, why, sizeof(why)) != 0) {
    hgl_set_error("rle_nms_device: %s", why);
    return HGL_EINVAL;
  }
  if (S == 0) return HGL_OK;      // nothing to rank: no launch, out_n is the caller's
  const RleNmsWs w = rle_nms_ws(plan, S, slot_words);
  if (!ws || ws_bytes < w.total) {
    hgl_set_error("rle_nms_device: workspace too small");
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  int32_t* partial = (int32_t*)(base + w.partial);
  int32_t* order = (int32_t*)(base + w.order);
  unsigned long long* sup = (unsigned long long*)(base + w.sup);
  const RlePairs& pr = plan.p;
  // six launches whatever G and the sizes are (S > 0: every one of them has a block)
  const RleStaged d = rle_stage_launch(slots, slot_words, table, S, plan.set.blocks, plan.set, plan.set, base, w.set, st);
  const int32_t* status = d.status;
  hipLaunchKernelGGL(rle_match_tile_kernel, dim3((unsigned)(pr.tiles * pr.splits)), dim3(RLE_THREADS), 0, st,
                     (const unsigned long long*)d.plane, (const unsigned long long*)d.plane, status, status, (const int32_t*)d.boxes,
                     (const int32_t*)d.boxes, pr.m, pr.splits, pr.pairs, 1, partial);
  hipLaunchKernelGGL(rle_nms_rank_kernel, dim3((unsigned)((S + RLE_THREADS - 1) / RLE_THREADS)), dim3(RLE_THREADS), 0, st, status, scores,
                     plan.n, order, result);
  const long long waves = RLE_THREADS / 64;
  hipLaunchKernelGGL(rle_nms_words_kernel, dim3((unsigned)((plan.sup_words + waves - 1) / waves)), dim3(RLE_THREADS), 0, st,
                     status, (const int32_t*)order, (const int32_t*)partial, plan.n, pr.splits, pr.pairs, plan.sup_words, thr, metric, sup);
  hipLaunchKernelGGL(rle_nms_walk_kernel, dim3((unsigned)G), dim3(RLE_THREADS), 0, st, status, (const int32_t*)order,
                     (const unsigned long long*)sup, plan.n, out_idx, out_n, result);
  return hgl_check_launch("rle_nms_device");
}

int hgl_rle_select_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S, const int64_t* images_host, int G,
                          const uint8_t* keep, const int32_t* nms_result, const uint32_t* cols, int C, uint32_t* out_slots,
                          int32_t* out_table, uint32_t* out_cols, int32_t* out_src, int32_t* out_n, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(images_host && S >= 0 && C >= 0 &&
                  (S == 0 || (slots && table && out_slots && out_table && out_src && out_n && (C == 0 || (cols && out_cols)))),
              "rle_select_device: bad arguments");
  RleSelectPlan plan;
  char why[200];
  if (rle_select_plan(images_host, G, S, slot_words, C, keep != nullptr, nms_result != nullptr, (uintptr_t)slots, (uintptr_t)out_slots,
                      (uintptr_t)table, (uintptr_t)out_table, &plan, why, sizeof(why)) != 0) {
    hgl_set_error("rle_select_device: %s", why);
    return HGL_EINVAL;
  }
  if (S == 0) return HGL_OK;      // nothing to move: no launch, out_n is the caller's
  hipStream_t st = (hipStream_t)stream;
  // two launches whatever G and the sizes are
  hipLaunchKernelGGL(rle_select_rank_kernel, dim3((unsigned)G), dim3(RLE_THREADS), 0, st, keep, nms_result, plan.s, out_src, out_n);
  auto move = plan.wide ? rle_select_move_kernel<true> : rle_select_move_kernel<false>;
  hipLaunchKernelGGL(move, dim3((unsigned)plan.blocks), dim3(64 * RLE_SELECT_WAVES), 0, st, slots, slot_words, table, cols, C, plan.s,
                     plan.chunks, (const int32_t*)out_src, out_slots, out_table, out_cols);
  return hgl_check_launch("rle_select_device");
}

size_t hgl_rle_merge_workspace_bytes(const int64_t* images_host, int G, int Ssrc, long long slot_words_src, int S, int M) {
  if (!images_host || slot_words_src < 0 || S == 0) return 0;
  RleMergePlan plan;
  char why[200];
  if (rle_merge_plan(images_host, G, Ssrc, S, M, &plan, why, sizeof(why)) != 0) return 0;
  return rle_merge_ws(plan, Ssrc, slot_words_src).total;
}

int hgl_rle_merge_device(const uint32_t* slots_src, long long slot_words_src, const int32_t* table_src, int Ssrc,
                         const int64_t* images_host, int G, const int32_t* members, int M, const int32_t* member_offsets,
                         const int32_t* bounds, uint32_t* slots, long long slot_words, int32_t* table, int S, int32_t* status, void* ws,
                         size_t ws_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(images_host && Ssrc >= 0 && S >= 0 && M >= 0 && slot_words_src >= 0 && slot_words >= 0 &&
                  (Ssrc == 0 || (slots_src && table_src)) && (M == 0 || members) &&
                  (S == 0 || (member_offsets && bounds && slots && table && status)),
              "rle_merge_device: bad arguments");
  RleMergePlan plan;
  char why[200];
  if (rle_merge_plan(images_host, G, Ssrc, S, M, &plan, why, sizeof(why)) != 0) {
    hgl_set_error("rle_merge_device: %s", why);
    return HGL_EINVAL;
  }
  if (S == 0) return HGL_OK;      // nothing to write: no launch, no workspace
  const RleMergeWs w = rle_merge_ws(plan, Ssrc, slot_words_src);
  if (!ws || ws_bytes < w.total) {
    hgl_set_error("rle_merge_device: workspace too small");
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  // three launches whatever G, S, M and the sizes are; two fewer for a source set without an entry
  const RleStaged src = rle_stage_launch(slots_src, slot_words_src, table_src, Ssrc, plan.src.blocks, plan.src, plan.src, base, w.src, st);
  hipLaunchKernelGGL(rle_merge_kernel, dim3((unsigned)S), dim3(RLE_THREADS), 0, st, (const unsigned long long*)src.plane,
                     (const int32_t*)src.status, plan.m, members, M, member_offsets, bounds, (unsigned long long*)(base + w.merged), slots,
                     slot_words, table, status);
  return hgl_check_launch("rle_merge_device");
}

}  // extern "C"
