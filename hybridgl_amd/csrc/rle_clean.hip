// remove_small_regions (utils/amg.py:267-291) on an ENCODED mask set: small holes filled, small islands dropped, the set encoded
// again with its boxes -- hgl_rle_clean_device.  The rule is the one csrc/sam_ccl.hip applies to byte masks; here no mask becomes
// bytes and no pixel gets a label: the components are found on column segments (csrc/ccl_runs.h), of which a mask has about as
// many as it has runs.
//
// THREE launches whatever G, S and the sizes are, none for S = 0; no host synchronisation, no allocation.
//
//   1, 2. rle_stage_set (rle.hip's starts kernel and plane kernel): status and area of every entry, and its 64-bit column words
//      in the workspace -- word x*HW64 + j = rows 64j .. 64j+63 of column x, padding bits clear.
//   3. rle_clean_kernel     one workgroup per entry, on the entry's own plane words.  A pass (rle_clean_pass) works on one colour:
//      the complement for holes, then the foreground -- of the plane the hole filling left -- for islands.
//        a. a segment starts where a pixel of the colour has none above it in its column: the pop-counts of the words' start bits,
//           sum-scanned 256 words at a time with a carry, give every word the rank of its first segment (one 32-bit word per plane
//           word) and the entry its segment count.  More than the workspace holds: the entry is refused (code 3), nothing written.
//        b. every word writes the segments that start in it: first row, last row (followed through the words below), parent link =
//           own rank, area = length, raster key = y0 * W + x.
//        c. one thread per column pair x | x+1 walks both columns' segments with two pointers and unites the ones that touch
//           (ccl_touch): a lock-free union-find, the higher root hung under the lower with atomicMin.
//        d. every segment finds its root and adds its area to the root's (atomicAdd) and its key (atomicMin).
//        e. the roots are the components: whether any is small or large and the best ccl_rank, block-reduced.
//        f. nothing small: the pass changed nothing.  Otherwise every plane word collects the bits of the segments in it whose
//           component flips (ccl_flips) and is rewritten, by its own thread alone.
//      Then the box of the plane (hgl_mask_boxes' rule), and rle_write_runs: the encoder's slot and table row.
//
// Atomics: atomicMin on parent links (the union-find's link by minimum: the root of a component is its lowest segment rank,
// whoever links first), atomicAdd on a root's area and atomicMin on its key (a sum and a minimum).  None of the three can show an
// order, so two calls give the same bytes.  Values another thread's atomic may have changed are read with relaxed agent-scope
// loads: a plain load could be served from a stale L1 line.  An entry of at most 4096 segments keeps those three arrays in LDS.
#include "hgl_common.h"
#include "rle_group.h"      // RleSet, rle_clean_plan
#include "rle_scan.h"       // RLE_THREADS, the block reductions, rle_group_find, rle_write_runs, rle_stage_ws, rle_stage_set
#include "ccl_runs.h"       // the segment arithmetic and the decision rule: shared with tests/native/rle_clean_sanitize.cpp

namespace {

__device__ __forceinline__ int clean_load(const int* a, int i) { return __hip_atomic_load(a + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void clean_store(int* a, int i, int v) { __hip_atomic_store(a + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Parent links only ever decrease and what atomicMin returns is authoritative (sam_ccl.hip's union-find, over segment ranks)
__device__ __forceinline__ int clean_find(int* L, int x) {
  int p = clean_load(L, x);
  while (p != x) {
    const int gp = clean_load(L, p);
    if (gp != p) atomicMin(&L[x], gp);      // path halving keeps the links monotone
    x = p;
    p = gp;
  }
  return x;
}
__device__ __forceinline__ void clean_union(int* L, int a, int b) {
  while (true) {
    a = clean_find(L, a);
    b = clean_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }      // a > b: hang a under b
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;      // somebody re-parented a meanwhile: go on from its new parent
  }
}

// the workgroup-wide maximum of a 64-bit v (rle_block_max's shape); lds: 4 elements
__device__ __forceinline__ unsigned long long clean_block_max64(unsigned long long v, unsigned long long* lds) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d, 64);
    v = v > o ? v : o;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const unsigned long long a = lds[0] > lds[1] ? lds[0] : lds[1], b = lds[2] > lds[3] ? lds[2] : lds[3];
  return a > b ? a : b;
}

// every write of the workgroup so far, plain or atomic, is visible to every thread of it
__device__ __forceinline__ void clean_sync() {
  __threadfence();
  __syncthreads();
}

struct CleanLds {
  unsigned red[4], wsum[4], wmax[4];
  unsigned long long red64[4];
};

// the segments of one entry and colour: cap words each in the workspace.  The three arrays the atomics work on live in LDS
// instead whenever the entry has at most CLEAN_LDS_SEGS segments (a proposal of 640 x 640 has one to two thousand): a find is a
// chain of dependent loads, and from the workspace every one of them is a round trip to L2.
constexpr int CLEAN_LDS_SEGS = 4096;      // 3 arrays: 48 KB
struct CleanSegs {
  int *y0, *y1, *parent, *area, *key;
};

// One pass over the plane P of an H x W entry (Q = W * HW64 words; wb: Q words).  -> -1: more than cap segments, nothing
// changed; 0: no small component; 1: a small component was found (and P rewritten, unless it was the one island that stays).
// Uniform over the workgroup.
__device__ int rle_clean_pass(unsigned long long* P, unsigned* wb, const CleanSegs& ws, int* seg_lds, int H, int W, int HW64, bool holes,
                              int thresh, long long cap, CleanLds& lds) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned Q = (unsigned)W * (unsigned)HW64;
  // ---- a. the rank of every word's first segment
  unsigned nseg = 0;
  for (unsigned base = 0; base < Q; base += RLE_THREADS) {
    const unsigned q = base + t;
    unsigned cnt = 0;
    if (q < Q) cnt = __popcll(ccl_word_starts(P + (size_t)(q / (unsigned)HW64) * HW64, H, (int)(q % (unsigned)HW64), holes));
    unsigned isum = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned a = __shfl_up(isum, d, 64);
      if (lane >= d) isum += a;
    }
    __syncthreads();      // the previous chunk's reads of wsum are over
    if (lane == 63) lds.wsum[wave] = isum;
    __syncthreads();
    unsigned before = nseg + isum - cnt, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) before += lds.wsum[w];
      tot += lds.wsum[w];
    }
    if (q < Q) wb[q] = before;
    nseg += tot;      // at most H*W / 2 + W < 2^31
  }
  if ((long long)nseg > cap) return -1;
  if (nseg == 0) return 0;
  CleanSegs sg = ws;
  if (nseg <= (unsigned)CLEAN_LDS_SEGS) {      // uniform over the workgroup
    sg.parent = seg_lds;
    sg.area = seg_lds + CLEAN_LDS_SEGS;
    sg.key = seg_lds + 2 * CLEAN_LDS_SEGS;
  }
  // ---- b. the segments (id < nseg <= cap)
  for (unsigned q = t; q < Q; q += RLE_THREADS) {
    const int x = (int)(q / (unsigned)HW64), j = (int)(q % (unsigned)HW64);
    const unsigned long long* col = P + (size_t)x * HW64;
    unsigned long long st = ccl_word_starts(col, H, j, holes);
    int id = (int)wb[q];
    while (st) {
      const int b = __builtin_ctzll(st);
      st &= st - 1ull;
      const int y0 = 64 * j + b, y1 = ccl_seg_end(col, H, HW64, holes, j, b);
      sg.y0[id] = y0;
      sg.y1[id] = y1;
      clean_store(sg.parent, id, id);
      clean_store(sg.area, id, y1 - y0 + 1);
      clean_store(sg.key, id, (int)ccl_key(y0, x, W));
      ++id;
    }
  }
  clean_sync();
  // ---- c. unions across every column boundary
  for (int x = t; x + 1 < W; x += RLE_THREADS) {
    int a = (int)wb[(size_t)x * HW64];
    const int a_end = (int)wb[(size_t)(x + 1) * HW64];
    int b = a_end;
    const int b_end = x + 2 < W ? (int)wb[(size_t)(x + 2) * HW64] : (int)nseg;
    while (a < a_end && b < b_end) {
      const int a1 = sg.y1[a], b1 = sg.y1[b];
      if (ccl_touch(sg.y0[a], a1, sg.y0[b], b1)) clean_union(sg.parent, a, b);
      if (ccl_first_moves(a1, b1)) ++a; else ++b;
    }
  }
  clean_sync();
  // ---- d. every segment under its root; area and key to the root (the roots are final: no union runs any more, and a segment
  // that is not a root keeps the area and key it was given)
  for (int i = t; i < (int)nseg; i += RLE_THREADS) {
    const int r = clean_find(sg.parent, i);
    if (r != i) {
      clean_store(sg.parent, i, r);
      atomicAdd(&sg.area[r], clean_load(sg.area, i));
      atomicMin(&sg.key[r], clean_load(sg.key, i));
    }
  }
  clean_sync();
  // ---- e. the components
  unsigned n_small = 0, n_large = 0;
  unsigned long long best = 0;
  for (int i = t; i < (int)nseg; i += RLE_THREADS) {
    if (clean_load(sg.parent, i) != i) continue;
    const unsigned area = (unsigned)clean_load(sg.area, i), key = (unsigned)clean_load(sg.key, i);
    if (ccl_small(area, thresh)) ++n_small; else ++n_large;
    const unsigned long long r = ccl_rank(area, key);
    best = best > r ? best : r;
  }
  n_small = rle_block_sum(n_small, lds.red);
  n_large = rle_block_sum(n_large, lds.red);
  if (n_small == 0) return 0;
  best = clean_block_max64(best, lds.red64);
  // ---- f. every word takes the bits of the segments in it that flip: the ones that start in it, and the one that reaches into
  // it from above
  for (unsigned q = t; q < Q; q += RLE_THREADS) {
    const int x = (int)(q / (unsigned)HW64), j = (int)(q % (unsigned)HW64);
    int lo = (int)wb[q];
    const int hi = q + 1 < Q ? (int)wb[q + 1] : (int)nseg;
    if (lo > (int)wb[(size_t)x * HW64] && sg.y1[lo - 1] >= 64 * j) --lo;
    unsigned long long m = 0;
    for (int id = lo; id < hi; ++id) {
      const int r = clean_load(sg.parent, id);
      if (ccl_flips(holes, (unsigned)clean_load(sg.area, r), (unsigned)clean_load(sg.key, r), thresh, n_large != 0, best))
        m |= ccl_seg_bits(sg.y0[id], sg.y1[id], j);
    }
    if (m) P[q] = holes ? (P[q] | m) : (P[q] & ~m);
  }
  clean_sync();      // the next pass, and the run writer, read any word
  return 1;
}

// boxes [S,4]: hgl_mask_boxes' rule for the cleaned mask; result [S,4] = (code, area after, changed, area before)
__global__ __launch_bounds__(RLE_THREADS) void rle_clean_kernel(unsigned long long* plane, const int32_t* __restrict__ status,
                                                                const RleSet geo, int thresh, int modes, long long cap,
                                                                unsigned* wbase, int* segs,
                                                                uint32_t* __restrict__ out_slots, long long out_slot_words,
                                                                int32_t* __restrict__ out_table, int32_t* __restrict__ boxes,
                                                                int32_t* __restrict__ result) {
  __shared__ CleanLds lds;
  __shared__ int seg_lds[3 * CLEAN_LDS_SEGS];
  const int s = blockIdx.x, t = threadIdx.x;
  const int g = rle_group_find(geo.first, geo.G, s);
  const int H = geo.H[g], W = geo.W[g], HW64 = (H + 63) / 64;
  const unsigned Q = (unsigned)W * (unsigned)HW64;
  const size_t word0 = (size_t)geo.word0[g] + (size_t)(s - geo.first[g]) * Q;
  unsigned long long* P = plane + word0;
  int* base = segs + (size_t)s * (size_t)cap * RLE_CLEAN_ARRAYS;
  const CleanSegs sg = {base, base + cap, base + 2 * cap, base + 3 * cap, base + 4 * cap};
  int32_t* row = out_table + (size_t)s * 4;
  int32_t* box = boxes + (size_t)s * 4;
  int32_t* res = result + (size_t)s * 4;
  int code = status[(size_t)s * 4];      // uniform over the workgroup, as everything up to the box
  const int area_before = status[(size_t)s * 4 + 1];
  int changed = 0;
  if (code != 2) {
    for (int pass = 0; pass < 2; ++pass) {
      if (!((modes >> pass) & 1)) continue;
      const int r = rle_clean_pass(P, wbase + word0, sg, seg_lds, H, W, HW64, pass == 0, thresh, cap, lds);
      if (r < 0) { code = 3; break; }
      changed |= r << pass;
    }
  }
  if (code >= 2) {      // no mask in the slot, or more segments than the workspace holds: nothing of the entry is written
    if (t == 0) {
      row[0] = 0; row[1] = 3; row[2] = 0; row[3] = 0;
      box[0] = 0; box[1] = 0; box[2] = 0; box[3] = 0;
      res[0] = code; res[1] = 0; res[2] = 0; res[3] = 0;
    }
    return;
  }
  unsigned area = 0, bx0 = 0x7fffffffu, by0 = 0x7fffffffu, bx1 = 0, by1 = 0;      // the box of this thread's words
  for (unsigned q = t; q < Q; q += RLE_THREADS) {
    const unsigned long long c = P[q];
    if (!c) continue;
    const unsigned x = q / (unsigned)HW64, y = 64u * (q % (unsigned)HW64);
    const unsigned ya = y + (unsigned)__builtin_ctzll(c), yb = y + 63u - (unsigned)__builtin_clzll(c);
    area += __popcll(c);
    bx0 = bx0 < x ? bx0 : x;
    bx1 = bx1 > x ? bx1 : x;
    by0 = by0 < ya ? by0 : ya;
    by1 = by1 > yb ? by1 : yb;
  }
  area = rle_block_sum(area, lds.red);
  bx0 = 0x7fffffffu - rle_block_max(0x7fffffffu - bx0, lds.red);      // minima as maxima of the complement
  by0 = 0x7fffffffu - rle_block_max(0x7fffffffu - by0, lds.red);
  bx1 = rle_block_max(bx1, lds.red);
  by1 = rle_block_max(by1, lds.red);
  if (t == 0) {
    box[0] = area ? (int32_t)bx0 : 0;      // an empty mask keeps the zeros of batched_mask_to_box
    box[1] = area ? (int32_t)by0 : 0;
    box[2] = area ? (int32_t)bx1 : 0;
    box[3] = area ? (int32_t)by1 : 0;
    res[0] = code; res[1] = (int32_t)area; res[2] = changed; res[3] = area_before;
  }
  rle_write_runs(P, H, W, HW64, out_slots + (size_t)s * (size_t)out_slot_words, out_slot_words, row, lds.red, lds.wsum, lds.wmax);
}

// the workspace of a clean-up: the set staged without boxes; a segment rank per plane word; the segment arrays
struct RleCleanWs {
  RleStageWs set;
  size_t wbase, segs, total;
};
RleCleanWs rle_clean_ws(const RleCleanPlan& plan, int S, long long sw) {
  RleCleanWs w;
  size_t p = 0;
  w.set = rle_stage_ws(&p, S, sw, plan.set.words, false);
  w.wbase = p;
  p += hgl_align_up((size_t)plan.set.words * sizeof(unsigned), 256);
  w.segs = p;
  w.total = p + hgl_align_up((size_t)S * (size_t)plan.cap * RLE_CLEAN_ARRAYS * sizeof(int), 256);
  return w;
}

}  // namespace

extern "C" {

size_t hgl_rle_clean_workspace_bytes(const int64_t* images_host, int G, int S, long long slot_words, long long seg_cap) {
  if (!images_host || S <= 0) return 0;
  RleCleanPlan plan;
  char why[200];
  // the thresholds and the output slots are the call's business: here only the geometry counts
  if (rle_clean_plan(images_host, G, S, slot_words, 0, 0, 3, seg_cap, &plan, why, sizeof(why)) != 0) return 0;
  return rle_clean_ws(plan, S, slot_words).total;
}

int hgl_rle_clean_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S, const int64_t* images_host, int G,
                         int area_thresh, int modes, long long seg_cap, uint32_t* out_slots, long long out_slot_words,
                         int32_t* out_table, int32_t* boxes_xyxy, int32_t* result, void* ws, size_t ws_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(images_host && S >= 0 && (S == 0 || (slots && table && out_slots && out_table && boxes_xyxy && result)),
              "rle_clean_device: bad arguments");
  RleCleanPlan plan;
  char why[200];
  if (rle_clean_plan(images_host, G, S, slot_words, out_slot_words, area_thresh, modes, seg_cap, &plan, why, sizeof(why)) != 0) {
    hgl_set_error("rle_clean_device: %s", why);
    return HGL_EINVAL;
  }
  if (S == 0) return HGL_OK;      // nothing to clean: no launch, no workspace
  const RleCleanWs w = rle_clean_ws(plan, S, slot_words);
  if (!ws || ws_bytes < w.total) {
    hgl_set_error("rle_clean_device: workspace too small");
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  int32_t* status = (int32_t*)(base + w.set.status);
  unsigned long long* plane = (unsigned long long*)(base + w.set.plane);
  // three launches whatever G, S and the sizes are (S > 0: every one of them has a block)
  rle_stage_set(slots, slot_words, table, S, plan.set, (uint32_t*)(base + w.set.E), status, plane, stream);
  hipLaunchKernelGGL(rle_clean_kernel, dim3((unsigned)S), dim3(RLE_THREADS), 0, st, plane, (const int32_t*)status, plan.set, area_thresh,
                     modes, plan.cap, (unsigned*)(base + w.wbase), (int*)(base + w.segs), out_slots, out_slot_words, out_table,
                     boxes_xyxy, result);
  return hgl_check_launch("rle_clean_device");
}

}  // extern "C"
