// The geometry of the RLE entries (csrc/rle.hip): the tiling of an image, shared by the encoder and the decoder, and what the host
// works out of a decode call's image rows (rle_group_plan), of a match call's (rle_match_plan) and of a merge call's
// (rle_merge_plan), of a mask NMS call's (rle_nms_plan) and of a compaction's (rle_select_plan) and hands to the kernels by value,
// and likewise of a polygon call's (rle_poly_plan, csrc/rle_poly.hip).  Plain C++ without a HIP construct: the .hip files include
// it, and so do the sanitizer harnesses tests/native/rle_group_sanitize.cpp, rle_match_sanitize.cpp, rle_merge_sanitize.cpp,
// rle_nms_sanitize.cpp and rle_select_sanitize.cpp.
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

// What a block of the plane kernel needs of the image that owns it (hgl_rle_iou_device: one image, hgl_rle_match_device: a
// group): the entries of an image lie back to back in the plane buffer, W * HW64 words each, 256 words per block.
struct RlePlaneOne {
  int H, W, HW64, q_tiles;
};
struct RlePlaneGroup {
  int H[RLE_GROUP_MAX], W[RLE_GROUP_MAX];
  int first[RLE_GROUP_MAX];                     // the image's first entry
  unsigned blk0[RLE_GROUP_MAX];                 // its first block of the plane kernel (non-decreasing, blk0[0] = 0)
  unsigned word0[RLE_GROUP_MAX];                // the plane word its first entry starts at
  int G;
};

// ---- hgl_rle_match_device: every mask of set A against every mask of set B, image by image.  A workgroup of the tile kernel
// owns RLE_MATCH_TA x RLE_MATCH_TB pairs of one image and walks the plane words RLE_MATCH_CHUNK at a time.
constexpr int RLE_MATCH_TA = 32, RLE_MATCH_TB = 64, RLE_MATCH_CHUNK = 32;
// A call with few tiles splits every tile's word range over `splits` workgroups (a 64 x 64 match is 2 tiles: alone they would
// walk 200 chunks each, one after the other, on 2 of the device's CUs); each writes its partial counts to a plane of its own.
constexpr int RLE_MATCH_BLOCKS = 1024, RLE_MATCH_SPLITS_MAX = 32;

struct RleMatch {
  long long off[RLE_GROUP_MAX];                           // element offset of the image's [na, nb] matrix
  int H[RLE_GROUP_MAX], W[RLE_GROUP_MAX];
  int first_a[RLE_GROUP_MAX + 1], first_b[RLE_GROUP_MAX + 1];      // first entries; [G] = Sa / Sb
  unsigned word0_a[RLE_GROUP_MAX], word0_b[RLE_GROUP_MAX];         // the plane word the image's first entry starts at
  unsigned tile0[RLE_GROUP_MAX];                          // the image's first tile (non-decreasing, tile0[0] = 0)
  long long pair0[RLE_GROUP_MAX];                         // the image's first element in a plane of partial counts
  int G;
};

struct RleMatchPlan {
  RleMatch m;
  RlePlaneGroup pa, pb;
  long long tiles, blocks_a, blocks_b;      // grid sizes: tile kernel, plane kernel of either side
  long long words_a, words_b;               // 64-bit plane words of either side
  long long pairs;                          // sum of na*nb: the elements of one plane of partial counts
  int splits;                               // workgroups per tile, 1 .. RLE_MATCH_SPLITS_MAX: ceil(RLE_MATCH_BLOCKS / tiles)
};

// images [G,5] = (H, W, first A entry, first B entry, element offset of the image's matrix) -> *plan; 0, or -1 with the reason
// in why.  inter_elems >= 0: the caller's matrix buffer holds that many elements, every extent [off, off + na*nb) must lie inside
// and no two may overlap.  inter_elems < 0: no matrix is wanted and column 4 is not read.  The partial counts of the tile kernel
// are always packed image after image (pair0, plan->pairs elements per split).  Checked besides: 1 <= G <= 64; Sa, Sb >= 0; H*W < 2^31; entries from 0 to Sa / Sb without
// a step back; Sa + Sb < 2^31; fewer than 2^31 tiles and plane blocks, fewer than 2^32 plane words per side.
static inline int rle_match_plan(const int64_t* images, int G, int Sa, int Sb, long long inter_elems, RleMatchPlan* plan, char* why,
                                 size_t why_cap) {
#define RLE_MATCH_REQUIRE(cond, ...)        \
  do {                                      \
    if (!(cond)) {                          \
      snprintf(why, why_cap, __VA_ARGS__);  \
      return -1;                            \
    }                                       \
  } while (0)
  RLE_MATCH_REQUIRE(G >= 1 && G <= RLE_GROUP_MAX, "%d images (1 .. %d in one call)", G, RLE_GROUP_MAX);
  RLE_MATCH_REQUIRE(Sa >= 0 && Sb >= 0 && (long long)Sa + Sb < (1ll << 31), "bad set sizes %d, %d (Sa + Sb must be < 2^31)", Sa, Sb);
  memset(plan, 0, sizeof(*plan));
  RleMatch* m = &plan->m;
  m->G = plan->pa.G = plan->pb.G = G;
  const bool packed = inter_elems < 0;
  long long lo[RLE_GROUP_MAX], hi[RLE_GROUP_MAX];      // the element extent [lo, hi) of every image's matrix
  for (int g = 0; g < G; ++g) {
    const int64_t* r = images + 5 * g;
    const long long H = r[0], W = r[1], ea = r[2], eb = r[3];
    const long long ea_next = g + 1 < G ? r[5 + 2] : (long long)Sa, eb_next = g + 1 < G ? r[5 + 3] : (long long)Sb;
    RLE_MATCH_REQUIRE(H > 0 && W > 0 && H < (1ll << 31) && W < (1ll << 31) && H * W < (1ll << 31),
                      "image %d: bad size %lld x %lld (H*W must be < 2^31)", g, H, W);
    RLE_MATCH_REQUIRE(ea >= 0 && ea <= ea_next && ea_next <= (long long)Sa && (g > 0 || ea == 0),
                      "image %d: A entries %lld .. %lld (rows must not decrease, from 0 to Sa = %d)", g, ea, ea_next, Sa);
    RLE_MATCH_REQUIRE(eb >= 0 && eb <= eb_next && eb_next <= (long long)Sb && (g > 0 || eb == 0),
                      "image %d: B entries %lld .. %lld (rows must not decrease, from 0 to Sb = %d)", g, eb, eb_next, Sb);
    const long long na = ea_next - ea, nb = eb_next - eb, n = na * nb;      // < 2^62
    const long long o = packed ? 0 : r[4];
    if (!packed) {
      RLE_MATCH_REQUIRE(o >= 0 && o <= inter_elems && n <= inter_elems - o,
                        "image %d: elements %lld .. +%lld lie outside the %lld of inter", g, o, n, inter_elems);
      lo[g] = o;
      hi[g] = o + n;
      for (int f = 0; f < g; ++f)
        RLE_MATCH_REQUIRE(lo[g] == hi[g] || lo[f] == hi[f] || hi[f] <= lo[g] || hi[g] <= lo[f],
                          "the matrices of images %d and %d overlap", f, g);
    }
    const long long HW64 = (H + 63) / 64, Q = W * HW64, q_tiles = (Q + 255) / 256;      // Q <= H*W < 2^31
    m->off[g] = o;
    m->H[g] = plan->pa.H[g] = plan->pb.H[g] = (int)H;
    m->W[g] = plan->pa.W[g] = plan->pb.W[g] = (int)W;
    m->first_a[g] = plan->pa.first[g] = (int)ea;
    m->first_b[g] = plan->pb.first[g] = (int)eb;
    m->word0_a[g] = plan->pa.word0[g] = (unsigned)plan->words_a;
    m->word0_b[g] = plan->pb.word0[g] = (unsigned)plan->words_b;
    m->tile0[g] = (unsigned)plan->tiles;
    m->pair0[g] = plan->pairs;
    plan->pa.blk0[g] = (unsigned)plan->blocks_a;
    plan->pb.blk0[g] = (unsigned)plan->blocks_b;
    plan->pairs += n;
    plan->words_a += na * Q;
    plan->words_b += nb * Q;
    plan->blocks_a += na * q_tiles;
    plan->blocks_b += nb * q_tiles;
    plan->tiles += ((na + RLE_MATCH_TA - 1) / RLE_MATCH_TA) * ((nb + RLE_MATCH_TB - 1) / RLE_MATCH_TB);
    RLE_MATCH_REQUIRE(plan->words_a < (1ll << 32) && plan->words_b < (1ll << 32),
                      "too many plane words for one call (sum of n*W*ceil(H/64) must be < 2^32 per side)");
    RLE_MATCH_REQUIRE(plan->blocks_a < (1ll << 31) && plan->blocks_b < (1ll << 31) && plan->tiles < (1ll << 31),
                      "too many entries (%d, %d) for one launch", Sa, Sb);
  }
  m->first_a[G] = Sa;
  m->first_b[G] = Sb;
  const long long want = plan->tiles > 0 ? (RLE_MATCH_BLOCKS + plan->tiles - 1) / plan->tiles : 1;
  plan->splits = (int)(want < 1 ? 1 : (want > RLE_MATCH_SPLITS_MAX ? RLE_MATCH_SPLITS_MAX : want));
  return 0;
#undef RLE_MATCH_REQUIRE
}

// ---- hgl_rle_merge_device: every output entry is a vote over source entries of its own image.  The source set goes through the
// plane kernel (RlePlaneGroup, as a side of the match does); a workgroup of the merge kernel owns one output entry, finds its
// image by its first output entry and writes the merged plane into the workspace before it writes the runs.
struct RleMerge {
  unsigned long long word0_out[RLE_GROUP_MAX];      // the plane word the image's first output entry starts at
  unsigned word0_src[RLE_GROUP_MAX];                // the plane word its first source entry starts at
  int H[RLE_GROUP_MAX], W[RLE_GROUP_MAX];
  int first_src[RLE_GROUP_MAX + 1], first_out[RLE_GROUP_MAX + 1];      // first entries; [G] = Ssrc / S
  int G;
};

struct RleMergePlan {
  RleMerge m;
  RlePlaneGroup src;
  long long blocks_src;                 // grid size of the plane kernel
  long long words_src, words_out;       // 64-bit plane words of the source set and of the merged set
};

// images [G,4] = (H, W, first source entry, first output entry) -> *plan; 0, or -1 with the reason in why.  Checked: 1 <= G <= 64;
// Ssrc, S, M >= 0; H*W < 2^31; entries from 0 to Ssrc / S without a step back; fewer than 2^31 plane blocks, fewer than 2^32 plane
// words on either side.
static inline int rle_merge_plan(const int64_t* images, int G, int Ssrc, int S, int M, RleMergePlan* plan, char* why, size_t why_cap) {
#define RLE_MERGE_REQUIRE(cond, ...)        \
  do {                                      \
    if (!(cond)) {                          \
      snprintf(why, why_cap, __VA_ARGS__);  \
      return -1;                            \
    }                                       \
  } while (0)
  RLE_MERGE_REQUIRE(G >= 1 && G <= RLE_GROUP_MAX, "%d images (1 .. %d in one call)", G, RLE_GROUP_MAX);
  RLE_MERGE_REQUIRE(Ssrc >= 0 && S >= 0 && M >= 0, "bad set sizes %d, %d and %d members", Ssrc, S, M);
  memset(plan, 0, sizeof(*plan));
  RleMerge* m = &plan->m;
  m->G = plan->src.G = G;
  for (int g = 0; g < G; ++g) {
    const int64_t* r = images + 4 * g;
    const long long H = r[0], W = r[1], es = r[2], eo = r[3];
    const long long es_next = g + 1 < G ? r[4 + 2] : (long long)Ssrc, eo_next = g + 1 < G ? r[4 + 3] : (long long)S;
    RLE_MERGE_REQUIRE(H > 0 && W > 0 && H < (1ll << 31) && W < (1ll << 31) && H * W < (1ll << 31),
                      "image %d: bad size %lld x %lld (H*W must be < 2^31)", g, H, W);
    RLE_MERGE_REQUIRE(es >= 0 && es <= es_next && es_next <= (long long)Ssrc && (g > 0 || es == 0),
                      "image %d: source entries %lld .. %lld (rows must not decrease, from 0 to Ssrc = %d)", g, es, es_next, Ssrc);
    RLE_MERGE_REQUIRE(eo >= 0 && eo <= eo_next && eo_next <= (long long)S && (g > 0 || eo == 0),
                      "image %d: output entries %lld .. %lld (rows must not decrease, from 0 to S = %d)", g, eo, eo_next, S);
    const long long ns = es_next - es, no = eo_next - eo;
    const long long HW64 = (H + 63) / 64, Q = W * HW64, q_tiles = (Q + 255) / 256;      // Q <= H*W < 2^31
    m->H[g] = plan->src.H[g] = (int)H;
    m->W[g] = plan->src.W[g] = (int)W;
    m->first_src[g] = plan->src.first[g] = (int)es;
    m->first_out[g] = (int)eo;
    m->word0_src[g] = plan->src.word0[g] = (unsigned)plan->words_src;
    m->word0_out[g] = (unsigned long long)plan->words_out;
    plan->src.blk0[g] = (unsigned)plan->blocks_src;
    plan->words_src += ns * Q;
    plan->words_out += no * Q;
    plan->blocks_src += ns * q_tiles;
    RLE_MERGE_REQUIRE(plan->words_src < (1ll << 32) && plan->words_out < (1ll << 32),
                      "too many plane words for one call (sum of n*W*ceil(H/64) must be < 2^32 per side)");
    RLE_MERGE_REQUIRE(plan->blocks_src < (1ll << 31), "too many entries (%d) for one launch", Ssrc);
  }
  m->first_src[G] = Ssrc;
  m->first_out[G] = S;
  return 0;
#undef RLE_MERGE_REQUIRE
}

// ---- hgl_rle_nms_device: greedy suppression by mask overlap of one set against itself, image by image.  The set goes through
// the plane kernel once and the tile kernel of the match counts it against itself (an RleMatchPlan with both sides the same,
// restricted to the tiles that hold a pair a < b); a row of an image's suppression words is ceil(n / 64) 64-bit words, one row
// per rank.  An image owns at most RLE_NMS_MAX entries: its pair counts are n * n int32 per split.
constexpr int RLE_NMS_MAX = 4096;

struct RleNms {
  long long pair0[RLE_GROUP_MAX];      // the image's first element in a plane of partial counts (RleMatch's)
  long long sup0[RLE_GROUP_MAX];       // its first suppression word (non-decreasing, sup0[0] = 0)
  int first[RLE_GROUP_MAX + 1];        // first entries; [G] = S
  int G;
};

struct RleNmsPlan {
  RleMatchPlan mp;           // the set against itself: m.first_a == m.first_b, pa == pb, tiles / splits / pairs of the full squares
  RleNms n;
  long long sup_words;       // 64-bit suppression words: sum of n_g * ceil(n_g / 64)
};

// images [G,3] = (H, W, first entry) -> *plan; 0, or -1 with the reason in why.  Checked: 1 <= G <= 64; S >= 0; H*W < 2^31; entries
// from 0 to S without a step back; at most RLE_NMS_MAX entries per image; and what rle_match_plan checks of the set against
// itself (fewer than 2^32 plane words, fewer than 2^31 blocks).
static inline int rle_nms_plan(const int64_t* images, int G, int S, RleNmsPlan* plan, char* why, size_t why_cap) {
#define RLE_NMS_REQUIRE(cond, ...)          \
  do {                                      \
    if (!(cond)) {                          \
      snprintf(why, why_cap, __VA_ARGS__);  \
      return -1;                            \
    }                                       \
  } while (0)
  RLE_NMS_REQUIRE(G >= 1 && G <= RLE_GROUP_MAX, "%d images (1 .. %d in one call)", G, RLE_GROUP_MAX);
  RLE_NMS_REQUIRE(S >= 0, "%d entries", S);
  int64_t rows[5 * RLE_GROUP_MAX];      // the match's rows: both sides the same set, no matrix
  for (int g = 0; g < G; ++g) {
    const long long H = images[3 * g], W = images[3 * g + 1], e = images[3 * g + 2];
    const long long e_next = g + 1 < G ? images[3 * (g + 1) + 2] : (long long)S;
    RLE_NMS_REQUIRE(H > 0 && W > 0 && H < (1ll << 31) && W < (1ll << 31) && H * W < (1ll << 31),
                    "image %d: bad size %lld x %lld (H*W must be < 2^31)", g, H, W);
    RLE_NMS_REQUIRE(e >= 0 && e <= e_next && e_next <= (long long)S && (g > 0 || e == 0),
                    "image %d: entries %lld .. %lld (rows must not decrease, from 0 to S = %d)", g, e, e_next, S);
    RLE_NMS_REQUIRE(e_next - e <= RLE_NMS_MAX, "image %d owns %lld entries (at most %d)", g, e_next - e, RLE_NMS_MAX);
    rows[5 * g] = H, rows[5 * g + 1] = W, rows[5 * g + 2] = rows[5 * g + 3] = e, rows[5 * g + 4] = 0;
  }
  if (rle_match_plan(rows, G, S, S, -1, &plan->mp, why, why_cap) != 0) return -1;      // S <= 64 * 4096: 2 S < 2^31
  memset(&plan->n, 0, sizeof(plan->n));
  plan->n.G = G;
  plan->sup_words = 0;
  for (int g = 0; g < G; ++g) {
    const long long n = plan->mp.m.first_a[g + 1] - plan->mp.m.first_a[g];
    plan->n.first[g] = plan->mp.m.first_a[g];
    plan->n.pair0[g] = plan->mp.m.pair0[g];
    plan->n.sup0[g] = plan->sup_words;
    plan->sup_words += n * ((n + 63) / 64);      // <= 64 * 4096 * 64
  }
  plan->n.first[G] = S;
  return 0;
#undef RLE_NMS_REQUIRE
}

// ---- hgl_rle_select_device: the kept entries of every image moved to the front of the image's range of a second set, in stored
// order, placeholders behind them.  One workgroup of the rank kernel per image; a wave of the move kernel owns one chunk of
// RLE_SELECT_CHUNK words of one destination entry, RLE_SELECT_WAVES waves to a workgroup.
constexpr int RLE_SELECT_COLS_MAX = 8, RLE_SELECT_WAVES = 4, RLE_SELECT_CHUNK = 2048;

struct RleSelect {
  int H[RLE_GROUP_MAX], W[RLE_GROUP_MAX];
  int first[RLE_GROUP_MAX + 1];        // first entries; [G] = S
  int max_keep[RLE_GROUP_MAX];         // the survivors an image may have: its entries when the caller sets no limit
  int G;
};

struct RleSelectPlan {
  RleSelect s;
  long long chunks;      // chunks of a slot: ceil(slot_words / RLE_SELECT_CHUNK), at least 1 (the table row and the columns ride in chunk 0)
  long long blocks;      // grid size of the move kernel: ceil(S / RLE_SELECT_WAVES) * chunks
  bool wide;             // the 16-byte path: slot_words % 4 == 0 and both slot buffers 16-byte aligned
};

// images [G,4] = (H, W, first entry, max_keep) -> *plan; 0, or -1 with the reason in why.  Checked: what rle_nms_plan checks of
// (H, W, first entry) -- 1 <= G <= 64, S >= 0, H*W < 2^31, entries from 0 to S without a step back, at most RLE_NMS_MAX entries per
// image, its plane-word limit -- and: 0 <= slot_words < 2^31, at least 1 when there is an entry (a placeholder is one count);
// 0 <= C <= RLE_SELECT_COLS_MAX; exactly one of the keep flags and the NMS rows is given; the byte ranges of slots / out_slots and
// of table / out_table do not overlap (addresses as numbers: nothing is read through them here); fewer than 2^31 blocks.
static inline int rle_select_plan(const int64_t* images, int G, int S, long long slot_words, int C, bool has_keep, bool has_nms,
                                  uintptr_t slots, uintptr_t out_slots, uintptr_t table, uintptr_t out_table, RleSelectPlan* plan,
                                  char* why, size_t why_cap) {
#define RLE_SELECT_REQUIRE(cond, ...)       \
  do {                                      \
    if (!(cond)) {                          \
      snprintf(why, why_cap, __VA_ARGS__);  \
      return -1;                            \
    }                                       \
  } while (0)
  RLE_SELECT_REQUIRE(G >= 1 && G <= RLE_GROUP_MAX, "%d images (1 .. %d in one call)", G, RLE_GROUP_MAX);
  RLE_SELECT_REQUIRE(slot_words >= 0 && slot_words < (1ll << 31), "slot_words %lld (0 .. 2^31 - 1)", slot_words);
  RLE_SELECT_REQUIRE(C >= 0 && C <= RLE_SELECT_COLS_MAX, "%d side columns (0 .. %d)", C, RLE_SELECT_COLS_MAX);
  RLE_SELECT_REQUIRE(has_keep != has_nms, "exactly one of keep and nms_result selects the entries (%s given)", has_keep ? "both" : "neither");
  int64_t rows[3 * RLE_GROUP_MAX];
  for (int g = 0; g < G; ++g) rows[3 * g] = images[4 * g], rows[3 * g + 1] = images[4 * g + 1], rows[3 * g + 2] = images[4 * g + 2];
  RleNmsPlan nms;
  if (rle_nms_plan(rows, G, S, &nms, why, why_cap) != 0) return -1;
  RLE_SELECT_REQUIRE(S == 0 || slot_words >= 1, "slot_words 0: a placeholder needs one word");
  memset(plan, 0, sizeof(*plan));
  plan->s.G = G;
  for (int g = 0; g < G; ++g) {
    const int n = nms.n.first[g + 1] - nms.n.first[g];
    const long long mk = images[4 * g + 3];
    plan->s.H[g] = nms.mp.m.H[g];
    plan->s.W[g] = nms.mp.m.W[g];
    plan->s.first[g] = nms.n.first[g];
    plan->s.max_keep[g] = (mk < 0 || mk > n) ? n : (int)mk;
  }
  plan->s.first[G] = S;
  const unsigned long long slot_bytes = (unsigned long long)S * (unsigned long long)slot_words * 4ull;      // < 2^18 * 2^31 * 4
  const unsigned long long table_bytes = (unsigned long long)S * 16ull;
  RLE_SELECT_REQUIRE(slot_bytes == 0 || (unsigned long long)slots + slot_bytes <= (unsigned long long)out_slots ||
                         (unsigned long long)out_slots + slot_bytes <= (unsigned long long)slots,
                     "out_slots overlaps slots");
  RLE_SELECT_REQUIRE(table_bytes == 0 || (unsigned long long)table + table_bytes <= (unsigned long long)out_table ||
                         (unsigned long long)out_table + table_bytes <= (unsigned long long)table,
                     "out_table overlaps table");
  plan->chunks = slot_words > 0 ? (slot_words + RLE_SELECT_CHUNK - 1) / RLE_SELECT_CHUNK : 1;
  plan->blocks = (((long long)S + RLE_SELECT_WAVES - 1) / RLE_SELECT_WAVES) * plan->chunks;      // <= 2^16 * 2^20
  RLE_SELECT_REQUIRE(plan->blocks < (1ll << 31), "too many words (%d entries of %lld) for one launch", S, slot_words);
  plan->wide = slot_words % 4 == 0 && ((slots | out_slots) & 15u) == 0;
  return 0;
#undef RLE_SELECT_REQUIRE
}

// ---- hgl_rle_from_polygons_device (csrc/rle_poly.hip): polygons -> RLE, one workgroup per entry.  A polygon's toggle plane --
// one bit per run-order position 0 .. H*W, H*W / 32 + 1 words -- lives in LDS when it has at most RLE_POLY_LDS_WORDS words
// (40 KB: 480 x 640 is 9601) and in the workspace otherwise; the entry's two coverage planes always live in the workspace.
constexpr int RLE_POLY_LDS_WORDS = 10240;

struct RlePoly {
  unsigned long long word0[RLE_GROUP_MAX];      // the 32-bit workspace word the image's first entry starts at
  int H[RLE_GROUP_MAX], W[RLE_GROUP_MAX];
  int first[RLE_GROUP_MAX];                     // the image's first entry (non-decreasing, first[0] = 0)
  int G;
};

// the words of one plane of an H x W entry, and the workspace words of the entry: two planes, a third when LDS cannot hold it
static inline unsigned long long rle_poly_plane_words(long long H, long long W) { return (unsigned long long)(H * W) / 32u + 1u; }
static inline unsigned long long rle_poly_entry_words(long long H, long long W) {
  const unsigned long long nw = rle_poly_plane_words(H, W);
  return nw * (nw > (unsigned long long)RLE_POLY_LDS_WORDS ? 3u : 2u);
}

// images [G,3] = (H, W, first entry) -> *geo and the 32-bit words of workspace the call needs; 0, or -1 with the reason in why.
// Checked: 1 <= G <= 64; S >= 0; sizes with H*W < 2^31; entries from 0 to S without a step back.
static inline int rle_poly_plan(const int64_t* images, int G, int S, RlePoly* geo, unsigned long long* words_out, char* why,
                                size_t why_cap) {
#define RLE_POLY_REQUIRE(cond, ...)         \
  do {                                      \
    if (!(cond)) {                          \
      snprintf(why, why_cap, __VA_ARGS__);  \
      return -1;                            \
    }                                       \
  } while (0)
  RLE_POLY_REQUIRE(G >= 1 && G <= RLE_GROUP_MAX, "%d images (1 .. %d in one call)", G, RLE_GROUP_MAX);
  RLE_POLY_REQUIRE(S >= 0, "%d entries", S);
  memset(geo, 0, sizeof(*geo));
  geo->G = G;
  unsigned long long words = 0;
  for (int g = 0; g < G; ++g) {
    const long long H = images[3 * g], W = images[3 * g + 1], e = images[3 * g + 2];
    const long long e_next = g + 1 < G ? images[3 * (g + 1) + 2] : (long long)S;
    RLE_POLY_REQUIRE(H > 0 && W > 0 && H < (1ll << 31) && W < (1ll << 31) && H * W < (1ll << 31),
                     "image %d: bad size %lld x %lld (H*W must be < 2^31)", g, H, W);
    RLE_POLY_REQUIRE(e >= 0 && e <= e_next && e_next <= (long long)S && (g > 0 || e == 0),
                     "image %d: entries %lld .. %lld (rows must not decrease, from 0 to S = %d)", g, e, e_next, S);
    geo->word0[g] = words;
    geo->H[g] = (int)H;
    geo->W[g] = (int)W;
    geo->first[g] = (int)e;
    words += (unsigned long long)(e_next - e) * rle_poly_entry_words(H, W);      // < 2^31 * 3 * 2^26
  }
  *words_out = words;
  return 0;
#undef RLE_POLY_REQUIRE
}

#endif  // HGL_RLE_GROUP_H
