// The geometry of the RLE entries (csrc/rle.hip, csrc/rle_poly.hip): the tiling of an image, shared by the encoder and the
// decoder; the checks every plan makes of its caller's image rows (rle_plan_count, rle_plan_size, rle_plan_entries); RleSet, the
// one description of "a set of entries that belongs to G images" and of its bit planes in the workspace, built image by image
// through rle_set_add; and the plans -- what the host works out of a decode call's rows (rle_group_plan), a match call's
// (rle_match_plan), a merge call's (rle_merge_plan), a mask NMS call's (rle_nms_plan), a compaction's (rle_select_plan), a
// polygon call's (rle_poly_plan), a clean-up's (rle_clean_plan) and a paint call's (rle_paint_plan).  A plan holds the RleSets the plane kernel stages and the structs the other kernels take by
// value (RleGroup, RleMatch, RleMerge, RleNms, RleSelect, RlePoly: their layout is the kernels' and stays); what such a struct
// repeats of a set is copied out of the set in one place.  Plain C++ without a HIP construct: the .hip files include it, and so
// do the sanitizer harnesses tests/native/rle_group_sanitize.cpp, rle_match_sanitize.cpp, rle_merge_sanitize.cpp,
// rle_nms_sanitize.cpp, rle_select_sanitize.cpp, rle_clean_sanitize.cpp and rle_paint_sanitize.cpp.  heat_paint_plan, the host
// side of the heat-map painter in csrc/rle_paint.hip, lives here too (tests/native/heat_paint_sanitize.cpp): it shares the canvas
// checks of rle_paint_plan.
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

// ---- what every plan checks of its rows.  A plan and a check return 0, or -1 with the reason in why.
#define RLE_PLAN_REQUIRE(cond, ...)         \
  do {                                      \
    if (!(cond)) {                          \
      snprintf(why, why_cap, __VA_ARGS__);  \
      return -1;                            \
    }                                       \
  } while (0)

static inline int rle_plan_count(int G, char* why, size_t why_cap) {
  RLE_PLAN_REQUIRE(G >= 1 && G <= RLE_GROUP_MAX, "%d images (1 .. %d in one call)", G, RLE_GROUP_MAX);
  return 0;
}
static inline int rle_plan_size(int g, long long H, long long W, char* why, size_t why_cap) {
  RLE_PLAN_REQUIRE(H > 0 && W > 0 && H < (1ll << 31) && W < (1ll << 31) && H * W < (1ll << 31),
                   "image %d: bad size %lld x %lld (H*W must be < 2^31)", g, H, W);
  return 0;
}
// the entries e .. e_next of image g in a set of S: from 0 to S without a step back.  `side` ("", "A ", "source " ..) and `total`
// ("S", "Sa", "Ssrc" ..) are what the callers' messages differ in.
static inline int rle_plan_entries(int g, long long e, long long e_next, int S, const char* side, const char* total, char* why,
                                   size_t why_cap) {
  RLE_PLAN_REQUIRE(e >= 0 && e <= e_next && e_next <= (long long)S && (g > 0 || e == 0),
                   "image %d: %sentries %lld .. %lld (rows must not decrease, from 0 to %s = %d)", g, side, e, e_next, total, S);
  return 0;
}
// column `col` of the row after `row` (image g of G, `stride` numbers to a row), or S behind the last row: where g's entries end
static inline long long rle_row_next(const int64_t* row, int stride, int col, int g, int G, int S) {
  return g + 1 < G ? row[stride + col] : (long long)S;
}

// canvas g (rle_paint_plan, heat_paint_plan): its n pixels from pixel o on lie inside [0, canvas_pixels) and apart from the
// canvases before it; lo / hi collect the extents
static inline int rle_plan_canvas(int g, long long o, long long n, long long canvas_pixels, long long* lo, long long* hi, char* why,
                                  size_t why_cap) {
  RLE_PLAN_REQUIRE(o >= 0 && o <= canvas_pixels && n <= canvas_pixels - o,
                   "image %d: pixels %lld .. %lld lie outside the %lld of the canvas", g, o, o + n, canvas_pixels);
  lo[g] = o;
  hi[g] = o + n;
  for (int f = 0; f < g; ++f)
    RLE_PLAN_REQUIRE(hi[f] <= lo[g] || hi[g] <= lo[f], "the canvases of images %d and %d overlap", f, g);
  return 0;
}
// the out_bytes at `out` apart from the base_bytes at `base`, unless base is 0 (addresses as numbers)
static inline int rle_plan_apart(uintptr_t base, unsigned long long base_bytes, uintptr_t out, unsigned long long out_bytes, char* why,
                                 size_t why_cap) {
  RLE_PLAN_REQUIRE(base == 0 || base_bytes == 0 || out_bytes == 0 || (unsigned long long)base + base_bytes <= (unsigned long long)out ||
                       (unsigned long long)out + out_bytes <= (unsigned long long)base,
                   "out overlaps base");
  return 0;
}

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
  if (rle_plan_count(G, why, why_cap)) return -1;
  memset(grp, 0, sizeof(*grp));
  grp->G = G;
  long long tiles = 0;
  long long lo[RLE_GROUP_MAX], hi[RLE_GROUP_MAX];      // the byte extent [lo, hi) of every image
  for (int g = 0; g < G; ++g) {
    const int64_t* r = images + 4 * g;
    const long long H = r[0], W = r[1], e = r[2], o = r[3], e_next = rle_row_next(r, 4, 2, g, G, S);
    if (rle_plan_size(g, H, W, why, why_cap) || rle_plan_entries(g, e, e_next, S, "", "S", why, why_cap)) return -1;
    const long long n = e_next - e;
    RLE_PLAN_REQUIRE(n * H * W < (1ll << 31), "image %d too large (n*H*W must be < 2^31)", g);
    RLE_PLAN_REQUIRE(o >= 0 && o <= masks_bytes && n * H * W <= masks_bytes - o,
                     "image %d: bytes %lld .. %lld lie outside the %lld of masks", g, o, o + n * H * W, masks_bytes);
    lo[g] = o;
    hi[g] = o + n * H * W;
    for (int f = 0; f < g; ++f)
      RLE_PLAN_REQUIRE(lo[g] == hi[g] || lo[f] == hi[f] || hi[f] <= lo[g] || hi[g] <= lo[f],
                       "the extents of images %d and %d overlap", f, g);
    const RleTiles t = rle_tiles(H, W, masks + (uintptr_t)o);
    grp->off[g] = o;
    grp->H[g] = (int)H;
    grp->W[g] = (int)W;
    grp->first[g] = (int)e;
    grp->tile0[g] = (unsigned)tiles;
    if (t.wide) grp->wide |= 1ull << g;
    tiles += n * t.col_tiles * t.row_tiles;
    RLE_PLAN_REQUIRE(tiles < (1ll << 31), "too many entries (%d) for one launch", S);
  }
  *tiles_out = tiles;
  return 0;
}

// A call of one image whose first entry lies at `masks` and which owns every entry: what the kernels take in place of RleGroup
// then -- nothing to look up, five scalars in the arguments.
struct RleOne {
  int H, W, HW64, col_tiles, row_tiles;      // rle_tiles' (the rows kernel reads the last two; 0 for a caller of the starts kernel alone)
};

// What a block of the plane kernel needs of the image that owns it: the entries of an image lie back to back in the plane
// buffer, W * HW64 words each, 256 words per block.  One image of one size (hgl_rle_iou_device) is four scalars ..
struct RlePlaneOne {
  int H, W, HW64, q_tiles;
};
// .. and a set over G images is an RleSet: a side of the match, the set of the mask NMS, the source set of the merge.  The
// starts kernel and the plane kernel take it by value.
struct RleSet {
  int H[RLE_GROUP_MAX], W[RLE_GROUP_MAX];
  int first[RLE_GROUP_MAX + 1];                 // the image's first entry (non-decreasing, first[0] = 0); [G] = S
  unsigned blk0[RLE_GROUP_MAX];                 // its first block of the plane kernel (non-decreasing, blk0[0] = 0)
  unsigned word0[RLE_GROUP_MAX];                // the plane word its first entry starts at
  long long words, blocks;                      // 64-bit plane words of the set; grid size of the plane kernel
  int G;
};

// Image g (the images come in order, into a zeroed set) with the entries e .. e_next, checked by rle_plan_size and
// rle_plan_entries.  Returns 0 or which of the set's two limits the image takes it beyond: fewer than 2^32 plane words, fewer than
// 2^31 plane blocks.  A caller with several sets adds all of them and then refuses the words before the blocks.
constexpr int RLE_SET_WORDS = 1, RLE_SET_BLOCKS = 2;
constexpr const char* RLE_SET_WORDS_WHY = "too many plane words for one call (sum of n*W*ceil(H/64) must be < 2^32 per side)";
static inline int rle_set_add(RleSet* set, int g, long long H, long long W, long long e, long long e_next) {
  const long long Q = W * ((H + 63) / 64), q_tiles = (Q + 255) / 256;      // Q <= H*W < 2^31
  set->H[g] = (int)H;
  set->W[g] = (int)W;
  set->first[g] = (int)e;
  set->first[g + 1] = (int)e_next;      // S in the end
  set->blk0[g] = (unsigned)set->blocks;
  set->word0[g] = (unsigned)set->words;
  set->words += (e_next - e) * Q;
  set->blocks += (e_next - e) * q_tiles;
  set->G = g + 1;
  return (set->words < (1ll << 32) ? 0 : RLE_SET_WORDS) | (set->blocks < (1ll << 31) ? 0 : RLE_SET_BLOCKS);
}

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

// The pairs of two sets over the same images (or of one set with itself): tiles and partial counts.
struct RlePairs {
  RleMatch m;
  long long tiles;      // grid size of the tile kernel, per split
  long long pairs;      // sum of na*nb: the elements of one plane of partial counts
  int splits;           // workgroups per tile, 1 .. RLE_MATCH_SPLITS_MAX: ceil(RLE_MATCH_BLOCKS / tiles)
};
// image g brings na x nb pairs (into a zeroed *p, in order): its first tile and its first partial count
static inline void rle_pairs_add(RlePairs* p, int g, long long na, long long nb) {
  p->m.tile0[g] = (unsigned)p->tiles;
  p->m.pair0[g] = p->pairs;
  p->pairs += na * nb;      // < 2^62
  p->tiles += ((na + RLE_MATCH_TA - 1) / RLE_MATCH_TA) * ((nb + RLE_MATCH_TB - 1) / RLE_MATCH_TB);
}
// every image is in: what the kernels' struct repeats of the two sets, and the splits
static inline void rle_pairs_close(RlePairs* p, const RleSet& a, const RleSet& b) {
  RleMatch* m = &p->m;
  m->G = a.G;
  for (int g = 0; g < a.G; ++g) {
    m->H[g] = a.H[g], m->W[g] = a.W[g];
    m->first_a[g] = a.first[g], m->first_b[g] = b.first[g];
    m->word0_a[g] = a.word0[g], m->word0_b[g] = b.word0[g];
  }
  m->first_a[a.G] = a.first[a.G], m->first_b[a.G] = b.first[a.G];
  const long long want = p->tiles > 0 ? (RLE_MATCH_BLOCKS + p->tiles - 1) / p->tiles : 1;
  p->splits = (int)(want < 1 ? 1 : (want > RLE_MATCH_SPLITS_MAX ? RLE_MATCH_SPLITS_MAX : want));
}

struct RleMatchPlan {
  RlePairs p;
  RleSet a, b;
};

// images [G,5] = (H, W, first A entry, first B entry, element offset of the image's matrix) -> *plan; 0, or -1 with the reason
// in why.  inter_elems >= 0: the caller's matrix buffer holds that many elements, every extent [off, off + na*nb) must lie inside
// and no two may overlap.  inter_elems < 0: no matrix is wanted and column 4 is not read.  The partial counts of the tile kernel
// are always packed image after image (pair0, p.pairs elements per split).  Checked besides: 1 <= G <= 64; Sa, Sb >= 0; H*W < 2^31;
// entries from 0 to Sa / Sb without a step back; Sa + Sb < 2^31; fewer than 2^31 tiles and plane blocks, fewer than 2^32 plane
// words per side.
static inline int rle_match_plan(const int64_t* images, int G, int Sa, int Sb, long long inter_elems, RleMatchPlan* plan, char* why,
                                 size_t why_cap) {
  if (rle_plan_count(G, why, why_cap)) return -1;
  RLE_PLAN_REQUIRE(Sa >= 0 && Sb >= 0 && (long long)Sa + Sb < (1ll << 31), "bad set sizes %d, %d (Sa + Sb must be < 2^31)", Sa, Sb);
  memset(plan, 0, sizeof(*plan));
  const bool packed = inter_elems < 0;
  long long lo[RLE_GROUP_MAX], hi[RLE_GROUP_MAX];      // the element extent [lo, hi) of every image's matrix
  for (int g = 0; g < G; ++g) {
    const int64_t* r = images + 5 * g;
    const long long H = r[0], W = r[1], ea = r[2], eb = r[3];
    const long long ea_next = rle_row_next(r, 5, 2, g, G, Sa), eb_next = rle_row_next(r, 5, 3, g, G, Sb);
    if (rle_plan_size(g, H, W, why, why_cap) || rle_plan_entries(g, ea, ea_next, Sa, "A ", "Sa", why, why_cap) ||
        rle_plan_entries(g, eb, eb_next, Sb, "B ", "Sb", why, why_cap))
      return -1;
    const long long na = ea_next - ea, nb = eb_next - eb, n = na * nb;      // < 2^62
    const long long o = packed ? 0 : r[4];
    if (!packed) {
      RLE_PLAN_REQUIRE(o >= 0 && o <= inter_elems && n <= inter_elems - o,
                       "image %d: elements %lld .. +%lld lie outside the %lld of inter", g, o, n, inter_elems);
      lo[g] = o;
      hi[g] = o + n;
      for (int f = 0; f < g; ++f)
        RLE_PLAN_REQUIRE(lo[g] == hi[g] || lo[f] == hi[f] || hi[f] <= lo[g] || hi[g] <= lo[f],
                         "the matrices of images %d and %d overlap", f, g);
    }
    plan->p.m.off[g] = o;
    rle_pairs_add(&plan->p, g, na, nb);
    const int over = rle_set_add(&plan->a, g, H, W, ea, ea_next) | rle_set_add(&plan->b, g, H, W, eb, eb_next);
    RLE_PLAN_REQUIRE(!(over & RLE_SET_WORDS), "%s", RLE_SET_WORDS_WHY);
    RLE_PLAN_REQUIRE(!(over & RLE_SET_BLOCKS) && plan->p.tiles < (1ll << 31), "too many entries (%d, %d) for one launch", Sa, Sb);
  }
  rle_pairs_close(&plan->p, plan->a, plan->b);
  return 0;
}

// ---- hgl_rle_merge_device: every output entry is a vote over source entries of its own image.  The source set goes through the
// plane kernel (an RleSet, as a side of the match does); a workgroup of the merge kernel owns one output entry, finds its
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
  RleSet src;
  long long words_out;      // 64-bit plane words of the merged set
};

// images [G,4] = (H, W, first source entry, first output entry) -> *plan; 0, or -1 with the reason in why.  Checked: 1 <= G <= 64;
// Ssrc, S, M >= 0; H*W < 2^31; entries from 0 to Ssrc / S without a step back; fewer than 2^31 plane blocks, fewer than 2^32 plane
// words on either side.
static inline int rle_merge_plan(const int64_t* images, int G, int Ssrc, int S, int M, RleMergePlan* plan, char* why, size_t why_cap) {
  if (rle_plan_count(G, why, why_cap)) return -1;
  RLE_PLAN_REQUIRE(Ssrc >= 0 && S >= 0 && M >= 0, "bad set sizes %d, %d and %d members", Ssrc, S, M);
  memset(plan, 0, sizeof(*plan));
  RleMerge* m = &plan->m;
  for (int g = 0; g < G; ++g) {
    const int64_t* r = images + 4 * g;
    const long long H = r[0], W = r[1], es = r[2], eo = r[3];
    const long long es_next = rle_row_next(r, 4, 2, g, G, Ssrc), eo_next = rle_row_next(r, 4, 3, g, G, S);
    if (rle_plan_size(g, H, W, why, why_cap) || rle_plan_entries(g, es, es_next, Ssrc, "source ", "Ssrc", why, why_cap) ||
        rle_plan_entries(g, eo, eo_next, S, "output ", "S", why, why_cap))
      return -1;
    m->first_out[g] = (int)eo;
    m->word0_out[g] = (unsigned long long)plan->words_out;
    plan->words_out += (eo_next - eo) * (W * ((H + 63) / 64));      // as rle_set_add counts
    const int over = rle_set_add(&plan->src, g, H, W, es, es_next);
    RLE_PLAN_REQUIRE(!(over & RLE_SET_WORDS) && plan->words_out < (1ll << 32), "%s", RLE_SET_WORDS_WHY);
    RLE_PLAN_REQUIRE(!(over & RLE_SET_BLOCKS), "too many entries (%d) for one launch", Ssrc);
  }
  m->first_out[G] = S;
  m->G = G;      // what the kernel's struct repeats of the source set
  for (int g = 0; g < G; ++g) m->H[g] = plan->src.H[g], m->W[g] = plan->src.W[g], m->word0_src[g] = plan->src.word0[g];
  memcpy(m->first_src, plan->src.first, sizeof(int) * (size_t)(G + 1));
  return 0;
}

// ---- hgl_rle_nms_device: greedy suppression by mask overlap of one set against itself, image by image.  The set goes through
// the plane kernel once and the tile kernel of the match counts it against itself (RlePairs with both sides the same set,
// restricted to the tiles that hold a pair a < b); a row of an image's suppression words is ceil(n / 64) 64-bit words, one row
// per rank.  An image owns at most RLE_NMS_MAX entries: its pair counts are n * n int32 per split.
constexpr int RLE_NMS_MAX = 4096;

struct RleNms {
  long long pair0[RLE_GROUP_MAX];      // the image's first element in a plane of partial counts (RleMatch's)
  long long sup0[RLE_GROUP_MAX];       // its first suppression word (non-decreasing, sup0[0] = 0)
  int first[RLE_GROUP_MAX + 1];        // first entries; [G] = S
  int G;
};

// The set of a mask NMS or of a compaction: rows of `stride` numbers that begin (H, W, first entry) -> *set.  Checked: S >= 0;
// H*W < 2^31; entries from 0 to S without a step back; at most RLE_NMS_MAX entries per image -- of every image, before the set's
// plane words (fewer than 2^32) are counted.  S <= 64 * 4096 then, so the set's blocks, at most words / 256 + S, need no check.
static inline int rle_nms_set(const int64_t* images, int stride, int G, int S, RleSet* set, char* why, size_t why_cap) {
  RLE_PLAN_REQUIRE(S >= 0, "%d entries", S);
  for (int g = 0; g < G; ++g) {
    const int64_t* r = images + stride * g;
    const long long e = r[2], e_next = rle_row_next(r, stride, 2, g, G, S);
    if (rle_plan_size(g, r[0], r[1], why, why_cap) || rle_plan_entries(g, e, e_next, S, "", "S", why, why_cap)) return -1;
    RLE_PLAN_REQUIRE(e_next - e <= RLE_NMS_MAX, "image %d owns %lld entries (at most %d)", g, e_next - e, RLE_NMS_MAX);
  }
  memset(set, 0, sizeof(*set));
  for (int g = 0; g < G; ++g) {
    const int64_t* r = images + stride * g;
    RLE_PLAN_REQUIRE(!(rle_set_add(set, g, r[0], r[1], r[2], rle_row_next(r, stride, 2, g, G, S)) & RLE_SET_WORDS), "%s", RLE_SET_WORDS_WHY);
  }
  return 0;
}

struct RleNmsPlan {
  RleSet set;
  RlePairs p;                // the set against itself: m.first_a == m.first_b, tiles / splits / pairs of the full squares
  RleNms n;
  long long sup_words;       // 64-bit suppression words: sum of n_g * ceil(n_g / 64)
};

// images [G,3] = (H, W, first entry) -> *plan; 0, or -1 with the reason in why.  Checked: 1 <= G <= 64 and what rle_nms_set checks.
static inline int rle_nms_plan(const int64_t* images, int G, int S, RleNmsPlan* plan, char* why, size_t why_cap) {
  if (rle_plan_count(G, why, why_cap) || rle_nms_set(images, 3, G, S, &plan->set, why, why_cap)) return -1;
  memset(&plan->p, 0, sizeof(plan->p));
  memset(&plan->n, 0, sizeof(plan->n));
  plan->n.G = G;
  plan->sup_words = 0;
  for (int g = 0; g < G; ++g) {
    const long long n = plan->set.first[g + 1] - plan->set.first[g];
    rle_pairs_add(&plan->p, g, n, n);      // at most 64 * 128 * 64 tiles
    plan->n.first[g] = plan->set.first[g];
    plan->n.pair0[g] = plan->p.m.pair0[g];
    plan->n.sup0[g] = plan->sup_words;
    plan->sup_words += n * ((n + 63) / 64);      // <= 64 * 4096 * 64
  }
  plan->n.first[G] = S;
  rle_pairs_close(&plan->p, plan->set, plan->set);
  return 0;
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
  if (rle_plan_count(G, why, why_cap)) return -1;
  RLE_PLAN_REQUIRE(slot_words >= 0 && slot_words < (1ll << 31), "slot_words %lld (0 .. 2^31 - 1)", slot_words);
  RLE_PLAN_REQUIRE(C >= 0 && C <= RLE_SELECT_COLS_MAX, "%d side columns (0 .. %d)", C, RLE_SELECT_COLS_MAX);
  RLE_PLAN_REQUIRE(has_keep != has_nms, "exactly one of keep and nms_result selects the entries (%s given)", has_keep ? "both" : "neither");
  RleSet set;
  if (rle_nms_set(images, 4, G, S, &set, why, why_cap)) return -1;
  RLE_PLAN_REQUIRE(S == 0 || slot_words >= 1, "slot_words 0: a placeholder needs one word");
  memset(plan, 0, sizeof(*plan));
  plan->s.G = G;
  for (int g = 0; g < G; ++g) {
    const int n = set.first[g + 1] - set.first[g];
    const long long mk = images[4 * g + 3];
    plan->s.H[g] = set.H[g];
    plan->s.W[g] = set.W[g];
    plan->s.first[g] = set.first[g];
    plan->s.max_keep[g] = (mk < 0 || mk > n) ? n : (int)mk;
  }
  plan->s.first[G] = S;
  const unsigned long long slot_bytes = (unsigned long long)S * (unsigned long long)slot_words * 4ull;      // < 2^18 * 2^31 * 4
  const unsigned long long table_bytes = (unsigned long long)S * 16ull;
  RLE_PLAN_REQUIRE(slot_bytes == 0 || (unsigned long long)slots + slot_bytes <= (unsigned long long)out_slots ||
                       (unsigned long long)out_slots + slot_bytes <= (unsigned long long)slots,
                   "out_slots overlaps slots");
  RLE_PLAN_REQUIRE(table_bytes == 0 || (unsigned long long)table + table_bytes <= (unsigned long long)out_table ||
                       (unsigned long long)out_table + table_bytes <= (unsigned long long)table,
                   "out_table overlaps table");
  plan->chunks = slot_words > 0 ? (slot_words + RLE_SELECT_CHUNK - 1) / RLE_SELECT_CHUNK : 1;
  plan->blocks = (((long long)S + RLE_SELECT_WAVES - 1) / RLE_SELECT_WAVES) * plan->chunks;      // <= 2^16 * 2^20
  RLE_PLAN_REQUIRE(plan->blocks < (1ll << 31), "too many words (%d entries of %lld) for one launch", S, slot_words);
  plan->wide = slot_words % 4 == 0 && ((slots | out_slots) & 15u) == 0;
  return 0;
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
  if (rle_plan_count(G, why, why_cap)) return -1;
  RLE_PLAN_REQUIRE(S >= 0, "%d entries", S);
  memset(geo, 0, sizeof(*geo));
  geo->G = G;
  unsigned long long words = 0;
  for (int g = 0; g < G; ++g) {
    const int64_t* r = images + 3 * g;
    const long long H = r[0], W = r[1], e = r[2], e_next = rle_row_next(r, 3, 2, g, G, S);
    if (rle_plan_size(g, H, W, why, why_cap) || rle_plan_entries(g, e, e_next, S, "", "S", why, why_cap)) return -1;
    geo->word0[g] = words;
    geo->H[g] = (int)H;
    geo->W[g] = (int)W;
    geo->first[g] = (int)e;
    words += (unsigned long long)(e_next - e) * rle_poly_entry_words(H, W);      // < 2^31 * 3 * 2^26
  }
  *words_out = words;
  return 0;
}

// ---- hgl_rle_clean_device (csrc/rle_clean.hip): small holes filled and small islands dropped in every entry of a set, on
// column segments (csrc/ccl_runs.h).  The set goes through the plane kernel; one workgroup per entry works on the entry's own
// plane words, one 32-bit segment rank per plane word and RLE_CLEAN_ARRAYS arrays of `cap` 32-bit words.
constexpr int RLE_CLEAN_ARRAYS = 5;      // first row, last row, parent link, area, raster key of a segment

struct RleCleanPlan {
  RleSet set;
  long long cap;      // segments per entry and colour the workspace holds: seg_cap, or the most any entry of the set can have
};

// images [G,3] = (H, W, first entry) -> *plan; 0, or -1 with the reason in why.  Checked: what rle_nms_plan checks -- 1 <= G <= 64,
// S >= 0, H*W < 2^31, entries from 0 to S without a step back, at most RLE_NMS_MAX entries per image, fewer than 2^32 plane words
// -- and: 0 <= slot_words, out_slot_words < 2^31; area_thresh >= 0; modes 1 .. 3 (bit 0 holes, bit 1 islands); 1 <= seg_cap < 2^31.
static inline int rle_clean_plan(const int64_t* images, int G, int S, long long slot_words, long long out_slot_words, int area_thresh,
                                 int modes, long long seg_cap, RleCleanPlan* plan, char* why, size_t why_cap) {
  if (rle_plan_count(G, why, why_cap)) return -1;
  RLE_PLAN_REQUIRE(slot_words >= 0 && slot_words < (1ll << 31), "slot_words %lld (0 .. 2^31 - 1)", slot_words);
  RLE_PLAN_REQUIRE(out_slot_words >= 0 && out_slot_words < (1ll << 31), "out_slot_words %lld (0 .. 2^31 - 1)", out_slot_words);
  RLE_PLAN_REQUIRE(area_thresh >= 0, "area_thresh %d (must not be negative)", area_thresh);
  RLE_PLAN_REQUIRE(modes >= 1 && modes <= 3, "modes %d (bit 0 = holes, bit 1 = islands: 1 .. 3)", modes);
  RLE_PLAN_REQUIRE(seg_cap >= 1 && seg_cap < (1ll << 31), "seg_cap %lld (1 .. 2^31 - 1)", seg_cap);
  if (rle_nms_set(images, 3, G, S, &plan->set, why, why_cap)) return -1;
  long long most = 1;      // ccl_seg_bound of the largest image that owns an entry
  for (int g = 0; g < G; ++g) {
    const long long b = (long long)plan->set.W[g] * (((long long)plan->set.H[g] + 1) / 2);
    if (plan->set.first[g + 1] > plan->set.first[g] && b > most) most = b;
  }
  plan->cap = seg_cap < most ? seg_cap : most;
  return 0;
}

// ---- hgl_rle_paint_device (csrc/rle_paint.hip): an ordered list of K positions, each naming an entry of its image, painted
// onto the images' RGB canvases.  Only the listed entries are staged: the starts kernel and the plane kernel run over the LIST
// (one row of run starts, one status row and one plane per position), and RlePick is the geometry they take for it -- the set of
// the positions, and where a position's entry is found.  A wave of the paint kernel owns one tile of RLE_PAINT_TILE columns x 64
// rows of one canvas.
constexpr int RLE_PAINT_TILE = 64;

struct RlePick {
  RleSet pos;                                   // the positions as a set: first[] = the image's first list position, [G] = K
  int entry0[RLE_GROUP_MAX], entries[RLE_GROUP_MAX];      // the image's first entry in the caller's set, and how many it owns
  const int32_t* order;                         // device [K]: position t of image g names entry entry0[g] + order[t]
};

struct RlePaint {
  long long pix0[RLE_GROUP_MAX];                // the pixel the image's canvas starts at
  int H[RLE_GROUP_MAX], W[RLE_GROUP_MAX];
  int first[RLE_GROUP_MAX + 1];                 // first list positions; [G] = K
  unsigned word0[RLE_GROUP_MAX];                // the plane word the image's first position starts at
  unsigned tile0[RLE_GROUP_MAX];                // the image's first tile (increasing, tile0[0] = 0)
  int G;
};

struct RlePaintPlan {
  RlePick pick;
  RlePaint p;
  long long tiles;      // tiles of all canvases: ceil(tiles / 4) workgroups of the paint kernel
};

// images [G,5] = (H, W, first entry, first list position, pixel offset) -> *plan; 0, or -1 with the reason in why.  Checked:
// 1 <= G <= 64; S, K >= 0; 0 <= slot_words < 2^31; 0 <= canvas_pixels < 2^60; H*W < 2^31; entries from 0 to S and list positions
// from 0 to K without a step back; every canvas [p, p + H*W) inside [0, canvas_pixels) and no two overlapping; fewer than 2^32
// plane words and 2^31 plane blocks over the list; fewer than 2^31 tiles; the 3 * canvas_pixels bytes at `out` apart from those at
// `base` unless base is 0 (addresses as numbers: nothing is read through them here).
static inline int rle_paint_plan(const int64_t* images, int G, int S, int K, long long slot_words, long long canvas_pixels,
                                 uintptr_t base, uintptr_t out, RlePaintPlan* plan, char* why, size_t why_cap) {
  if (rle_plan_count(G, why, why_cap)) return -1;
  RLE_PLAN_REQUIRE(S >= 0 && K >= 0, "bad sizes: %d entries, %d list positions", S, K);
  RLE_PLAN_REQUIRE(slot_words >= 0 && slot_words < (1ll << 31), "slot_words %lld (0 .. 2^31 - 1)", slot_words);
  RLE_PLAN_REQUIRE(canvas_pixels >= 0 && canvas_pixels < (1ll << 60), "canvas_pixels %lld (0 .. 2^60 - 1)", canvas_pixels);
  memset(plan, 0, sizeof(*plan));
  RlePaint* p = &plan->p;
  long long lo[RLE_GROUP_MAX], hi[RLE_GROUP_MAX];      // the pixel extent [lo, hi) of every canvas
  for (int g = 0; g < G; ++g) {
    const int64_t* r = images + 5 * g;
    const long long H = r[0], W = r[1], e = r[2], k = r[3], o = r[4];
    const long long e_next = rle_row_next(r, 5, 2, g, G, S), k_next = rle_row_next(r, 5, 3, g, G, K);
    if (rle_plan_size(g, H, W, why, why_cap) || rle_plan_entries(g, e, e_next, S, "", "S", why, why_cap) ||
        rle_plan_entries(g, k, k_next, K, "list ", "K", why, why_cap))
      return -1;
    if (rle_plan_canvas(g, o, H * W, canvas_pixels, lo, hi, why, why_cap)) return -1;
    const int over = rle_set_add(&plan->pick.pos, g, H, W, k, k_next);
    RLE_PLAN_REQUIRE(!(over & RLE_SET_WORDS), "%s", RLE_SET_WORDS_WHY);
    RLE_PLAN_REQUIRE(!(over & RLE_SET_BLOCKS), "too many list positions (%d) for one launch", K);
    plan->pick.entry0[g] = (int)e;
    plan->pick.entries[g] = (int)(e_next - e);
    p->pix0[g] = o;
    p->H[g] = (int)H;
    p->W[g] = (int)W;
    p->first[g] = (int)k;
    p->word0[g] = plan->pick.pos.word0[g];
    p->tile0[g] = (unsigned)plan->tiles;
    plan->tiles += ((W + RLE_PAINT_TILE - 1) / RLE_PAINT_TILE) * ((H + 63) / 64);
    RLE_PLAN_REQUIRE(plan->tiles < (1ll << 31), "too many tiles (%lld) for one launch", plan->tiles);
  }
  p->first[G] = K;
  p->G = G;
  const unsigned long long bytes = 3ull * (unsigned long long)canvas_pixels;
  return rle_plan_apart(base, bytes, out, bytes, why, why_cap);
}

// ---- hgl_heat_paint_device (csrc/rle_paint.hip): M heat-maps turned into colours on RGB canvases.  A workgroup of each of the
// three kernels owns one share of consecutive pixels of one map: HEAT_BLOCK_PIX pixels, or the multiple of it that keeps a map
// at HEAT_PARTS_MAX shares at the most -- a workgroup folds its map's partials, one per share, with one load per thread.
constexpr int HEAT_BLOCK_PIX = 4096, HEAT_PARTS_MAX = 256;

// the pixels of one share of a map of n pixels (0 < n < 2^31): a multiple of HEAT_BLOCK_PIX, ceil(n / share) <= HEAT_PARTS_MAX
// (constexpr: the kernels call it as well)
constexpr long long heat_share(long long n) {
  const long long per = (n + HEAT_PARTS_MAX - 1) / HEAT_PARTS_MAX;
  return ((per + HEAT_BLOCK_PIX - 1) / HEAT_BLOCK_PIX) * HEAT_BLOCK_PIX;
}

struct HeatPaint {
  long long heat0[RLE_GROUP_MAX];               // the element of heat the map starts at
  long long base0[RLE_GROUP_MAX];               // the pixel of base its image starts at
  long long pix0[RLE_GROUP_MAX];                // the pixel of out (the element of levels) its canvas starts at
  int H[RLE_GROUP_MAX], W[RLE_GROUP_MAX];
  unsigned blk0[RLE_GROUP_MAX + 1];             // the map's first workgroup = its first partial (increasing, blk0[0] = 0); [M] = all
  unsigned char dirflag[RLE_GROUP_MAX];
  int M;
};

struct HeatPaintPlan {
  HeatPaint p;
  long long blocks;      // workgroups of each launch and partials of each kind: at most RLE_GROUP_MAX * HEAT_PARTS_MAX
};

// maps [M,6] = (H, W, dirflag, heat element, base pixel, out pixel) -> *plan; 0, or -1 with the reason in why.  Checked:
// 1 <= M <= 64; 0 <= heat_elems, canvas_pixels < 2^60; H*W < 2^31; dirflag 0 .. 3; every heat extent [h, h + H*W) inside
// [0, heat_elems) and every base extent from a pixel 0 <= b < 2^60 on (both are only read: they may coincide or overlap); every
// canvas [p, p + H*W) inside [0, canvas_pixels) and no two overlapping; the 3 * canvas_pixels bytes at `out` apart from the bytes
// of base that the maps name, unless base is 0 (addresses as numbers: nothing is read through them here).
static inline int heat_paint_plan(const int64_t* maps, int M, long long heat_elems, long long canvas_pixels, uintptr_t base,
                                  uintptr_t out, HeatPaintPlan* plan, char* why, size_t why_cap) {
  RLE_PLAN_REQUIRE(M >= 1 && M <= RLE_GROUP_MAX, "%d maps (1 .. %d in one call)", M, RLE_GROUP_MAX);
  RLE_PLAN_REQUIRE(heat_elems >= 0 && heat_elems < (1ll << 60), "heat_elems %lld (0 .. 2^60 - 1)", heat_elems);
  RLE_PLAN_REQUIRE(canvas_pixels >= 0 && canvas_pixels < (1ll << 60), "canvas_pixels %lld (0 .. 2^60 - 1)", canvas_pixels);
  memset(plan, 0, sizeof(*plan));
  HeatPaint* p = &plan->p;
  long long lo[RLE_GROUP_MAX], hi[RLE_GROUP_MAX];      // the pixel extent [lo, hi) of every canvas
  long long b_lo = 0, b_hi = 0;                        // the pixels of base that some map names
  for (int m = 0; m < M; ++m) {
    const int64_t* r = maps + 6 * m;
    const long long H = r[0], W = r[1], d = r[2], h = r[3], b = r[4], o = r[5];
    if (rle_plan_size(m, H, W, why, why_cap)) return -1;
    const long long n = H * W;
    RLE_PLAN_REQUIRE(d >= 0 && d <= 3, "map %d: dirflag %lld (0 none, 1 left, 2 right, 3 middle)", m, d);
    RLE_PLAN_REQUIRE(h >= 0 && h <= heat_elems && n <= heat_elems - h,
                     "map %d: elements %lld .. %lld lie outside the %lld of heat", m, h, h + n, heat_elems);
    RLE_PLAN_REQUIRE(b >= 0 && b < (1ll << 60), "map %d: base pixel %lld (0 .. 2^60 - 1)", m, b);
    if (rle_plan_canvas(m, o, n, canvas_pixels, lo, hi, why, why_cap)) return -1;
    if (m == 0 || b < b_lo) b_lo = b;
    if (m == 0 || b + n > b_hi) b_hi = b + n;
    p->heat0[m] = h;
    p->base0[m] = b;
    p->pix0[m] = o;
    p->H[m] = (int)H;
    p->W[m] = (int)W;
    p->dirflag[m] = (unsigned char)d;
    p->blk0[m] = (unsigned)plan->blocks;
    const long long share = heat_share(n);
    plan->blocks += (n + share - 1) / share;
  }
  p->blk0[M] = (unsigned)plan->blocks;
  p->M = M;
  return rle_plan_apart(base ? base + 3ull * (unsigned long long)b_lo : 0, 3ull * (unsigned long long)(b_hi - b_lo), out,
                        3ull * (unsigned long long)canvas_pixels, why, why_cap);
}

#undef RLE_PLAN_REQUIRE
#endif  // HGL_RLE_GROUP_H
