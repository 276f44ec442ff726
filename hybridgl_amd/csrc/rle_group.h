// The geometry of the RLE entries (csrc/rle.hip): the tiling of an image, shared by the encoder and the decoder, and what the host
// works out of a decode call's image rows and hands to the two decoder kernels by value.  Plain C++ without a HIP construct:
// rle.hip includes it, and so does the sanitizer harness tests/native/rle_group_sanitize.cpp.
#ifndef HGL_RLE_GROUP_H
#define HGL_RLE_GROUP_H
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

// The tiles of one H x W mask whose first byte lies at address `base` (rle_columns_kernel and rle_rows_kernel alike): a block is
// 4 waves = 4 row tiles of 64 rows, by 64 lanes of one column each or, on the 4-column path (W % 4 == 0 and base 4-byte aligned:
// one aligned 32-bit access per row and lane), of four.
struct RleTiles {
  bool wide;
  int HW64, col_tiles, row_tiles;      // 64-row words per column; blocks across; blocks down
};
static inline RleTiles rle_tiles(long long H, long long W, uintptr_t base) {
  const bool wide = (W % 4 == 0) && ((base & 3u) == 0);
  const int HW64 = (int)((H + 63) / 64);
  return {wide, HW64, (int)((W + (wide ? 255 : 63)) / (wide ? 256 : 64)), (HW64 + 3) / 4};
}

constexpr int RLE_GROUP_MAX = 64;

struct RleGroup {
  long long off[RLE_GROUP_MAX];                 // byte offset of the image's first entry in masks
  int H[RLE_GROUP_MAX], W[RLE_GROUP_MAX];
  int first[RLE_GROUP_MAX];                     // the image's first entry (non-decreasing, first[0] = 0)
  unsigned tile0[RLE_GROUP_MAX];                // the image's first tile of rle_rows_kernel (non-decreasing, tile0[0] = 0)
  unsigned long long wide;                      // bit g: image g takes the 4-column store path
  int G;
};

// images [G,4] = (H, W, first entry, byte offset) -> *grp and the number of tiles of the rows kernel; 0, or -1 with the reason in
// why.  Checked: 1 <= G <= 64; sizes with H*W < 2^31; entries from 0 to S without a step back; n*H*W < 2^31 per image; every
// extent inside [0, masks_bytes) and no two of them overlapping; fewer than 2^31 tiles.  The 4-column path is an image's whose W
// is a multiple of 4 and whose first byte (masks + offset) is 4-byte aligned: H*W is then a multiple of 4 and every entry is.
static inline int rle_group_plan(const int64_t* images, int G, int S, uintptr_t masks, long long masks_bytes, RleGroup* grp,
                                 long long* tiles_out, char* why, size_t why_cap) {
#define RLE_GROUP_REQUIRE(cond, ...)        \
  do {                                      \
    if (!(cond)) {                          \
      snprintf(why, why_cap, __VA_ARGS__);  \
      return -1;                            \
    }                                       \
  } while (0)
  RLE_GROUP_REQUIRE(G >= 1 && G <= RLE_GROUP_MAX, "%d images (1 .. %d in one call)", G, RLE_GROUP_MAX);
  memset(grp, 0, sizeof(*grp));
  grp->G = G;
  long long tiles = 0;
  long long lo[RLE_GROUP_MAX], hi[RLE_GROUP_MAX];      // the byte extent [lo, hi) of every image
  for (int g = 0; g < G; ++g) {
    const long long H = images[4 * g], W = images[4 * g + 1], e = images[4 * g + 2], o = images[4 * g + 3];
    const long long e_next = g + 1 < G ? images[4 * (g + 1) + 2] : (long long)S;
    RLE_GROUP_REQUIRE(H > 0 && W > 0 && H < (1ll << 31) && W < (1ll << 31) && H * W < (1ll << 31),
                      "image %d: bad size %lld x %lld (H*W must be < 2^31)", g, H, W);
    RLE_GROUP_REQUIRE(e >= 0 && e <= e_next && e_next <= (long long)S && (g > 0 || e == 0),
                      "image %d: entries %lld .. %lld (rows must not decrease, from 0 to S = %d)", g, e, e_next, S);
    const long long n = e_next - e;
    RLE_GROUP_REQUIRE(n * H * W < (1ll << 31), "image %d too large (n*H*W must be < 2^31)", g);
    RLE_GROUP_REQUIRE(o >= 0 && o <= masks_bytes && n * H * W <= masks_bytes - o,
                      "image %d: bytes %lld .. %lld lie outside the %lld of masks", g, o, o + n * H * W, masks_bytes);
    lo[g] = o;
    hi[g] = o + n * H * W;
    for (int f = 0; f < g; ++f)
      RLE_GROUP_REQUIRE(lo[g] == hi[g] || lo[f] == hi[f] || hi[f] <= lo[g] || hi[g] <= lo[f],
                        "the extents of images %d and %d overlap", f, g);
    const RleTiles t = rle_tiles(H, W, masks + (uintptr_t)o);
    grp->off[g] = o;
    grp->H[g] = (int)H;
    grp->W[g] = (int)W;
    grp->first[g] = (int)e;
    grp->tile0[g] = (unsigned)tiles;
    if (t.wide) grp->wide |= 1ull << g;
    tiles += n * t.col_tiles * t.row_tiles;
    RLE_GROUP_REQUIRE(tiles < (1ll << 31), "too many entries (%d) for one launch", S);
  }
  *tiles_out = tiles;
  return 0;
#undef RLE_GROUP_REQUIRE
}

// A call of one image whose first entry lies at `masks` and which owns every entry: what the kernels take in place of RleGroup
// then -- nothing to look up, five scalars in the arguments.
struct RleOne {
  int H, W, HW64, col_tiles, row_tiles;      // rle_tiles' (the rows kernel reads the last two; 0 for a caller of the starts kernel alone)
};

#endif  // HGL_RLE_GROUP_H
