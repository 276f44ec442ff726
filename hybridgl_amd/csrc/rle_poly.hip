// Ground-truth polygons rasterised on the device, straight into RLE (hgl_rle_from_polygons_device): the device form of
// refer/external/maskApi.c rleFrPoly (:161-201) followed by the per-pixel polygon count of refer/refer.py:283-291 and the
// dataset's rule (data/dataset_refer_bert.py:118-121: pixels covered by exactly one polygon) or mask.merge's (at least one).
// gtmask.cpp hgl_gt_mask_from_polygons is the sequential host form and the yardstick; the walk's arithmetic is shared with it
// in spirit and with the sanitizer harness in letter (poly_walk.h).  The masks never exist as pixels: what leaves the kernel
// is what hgl_rle_encode_device would have written for them.
//
// One launch whatever G, S, P and the sizes are; one workgroup per entry, which takes its polygons one after the other:
//
//   1. toggle   every step of the 5x super-sampled boundary walk stands alone (poly_walk.h): a wave takes an edge, its lanes
//      stride over the edge's steps, and a step that crosses a column XORs one bit of the toggle plane at the column-major
//      position x*H + y (H*W + 1 bits; position H*W toggles nothing inside the image and is dropped).  THIS IS THE FIRST ATOMIC
//      OF THE RLE FAMILY: an integer XOR is order-independent, positions listed an even number of times cancel by themselves, and
//      the bytes depend on no scheduling.  The plane lives in LDS when it has at most RLE_POLY_LDS_WORDS words (ds_xor_b32),
//      else in the workspace (global_atomic_xor).
//   2. fill     the polygon's mask is the prefix parity of the toggle stream: shift-XOR within a word; across words the parity
//      of the pop-counts, 256 words at a time (a ballot per wave, four wave parities through LDS) with a carry.
//   3. combine  two coverage planes in the workspace, once / more: more |= once & m; once ^= m.  The pop-count of m is the
//      polygon's own area (what the host codec sums into `area`).
//   4. encode   C = once & ~more (rule 0) or once | more (rule 1), in column-major order, IS the encoder's form-1 plane; its
//      transitions T = C ^ ((C << 1) | carry) are the form-0 counts, written by the scan rle_runs_kernel ends in
//      (rle_counts_chunk, rle_scan.h).
//
// An entry whose polygons the host codec refuses (a polygon without a vertex, a coordinate that is NaN or outside (-1e5, 1e5))
// or whose walk has 2^31 steps or more writes table (0, 3, 0, 0) and status code 2 and touches no slot word.
#include "hgl_common.h"
#include "rle_group.h"      // RlePoly, rle_poly_plan, RLE_POLY_LDS_WORDS
#include "rle_scan.h"       // RLE_THREADS, rle_block_sum, rle_group_find, rle_counts_chunk
#include "poly_walk.h"

namespace {

// step 1: the toggles of one polygon (k >= 1 vertices at xy) into the plane T of nw words, cleared here
__device__ __forceinline__ void poly_toggle(unsigned* T, unsigned nw, const double* __restrict__ xy, int k, int H, int W, unsigned HW) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (unsigned w = t; w < nw; w += RLE_THREADS) T[w] = 0u;
  __syncthreads();
  for (int j = wave; j < k; j += RLE_THREADS / 64) {
    const PolyEdge e = poly_edge_of(xy, k, j);
    for (int d = lane; d <= e.n; d += 64) {
      unsigned pos;
      if (poly_step(xy, k, j, e, d, H, W, &pos) && pos < HW) atomicXor(&T[pos >> 5], 1u << (pos & 31u));      // pos >> 5 < nw
    }
  }
  __syncthreads();
}

// steps 2 and 3: the prefix parity of T, masked to the H*W pixels, joined into once / more (first: they hold nothing yet);
// returns this thread's share of the polygon's area.  wpar: 4 words of LDS.
__device__ __forceinline__ unsigned poly_fill(const unsigned* T, unsigned nw, unsigned HW, unsigned* __restrict__ once,
                                              unsigned* __restrict__ more, bool first, unsigned* wpar) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  unsigned carry = 0, area = 0;      // the parity of all toggles before this chunk
  for (unsigned base = 0; base < nw; base += RLE_THREADS) {
    const unsigned w = base + t;
    // an atomic load: the toggles were made by atomics at the L2, a plain load could be served by a line the L1 kept
    unsigned x = w < nw ? __hip_atomic_load(&T[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    const unsigned long long odd = __ballot((int)(__popc(x) & 1u));      // the lanes whose word flips the parity
    x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;      // bit i: the parity of the word's toggles at bits 0 .. i
    unsigned before = (unsigned)__popcll(odd & ((1ull << lane) - 1ull)) & 1u;
    __syncthreads();      // the previous chunk's reads of wpar are over
    if (lane == 0) wpar[wave] = (unsigned)__popcll(odd) & 1u;
    __syncthreads();
    unsigned tot = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (v < wave) before ^= wpar[v];
      tot ^= wpar[v];
    }
    before ^= carry;
    carry ^= tot;
    if (w < nw) {
      unsigned m = before ? ~x : x;
      const unsigned lo = 32u * w;      // <= H*W
      if (HW - lo < 32u) m &= (1u << (HW - lo)) - 1u;      // the bits of positions >= H*W
      area += __popc(m);
      if (first) {
        once[w] = m;
        more[w] = 0u;
      } else {
        const unsigned o = once[w];
        more[w] |= o & m;
        once[w] = o ^ m;
      }
    }
  }
  return area;
}

// the transitions of word w of the run-order plane C (w < plane_words; bits beyond H*W are 0 in C)
__device__ __forceinline__ unsigned poly_transitions(const unsigned* __restrict__ C, unsigned w, unsigned HW) {
  const unsigned c = C[w], carry = w > 0 ? C[w - 1] >> 31 : 0u;
  const unsigned lo = 32u * w;      // < H*W
  const unsigned valid = HW - lo < 32u ? (1u << (HW - lo)) - 1u : ~0u;
  return (c ^ ((c << 1) | carry)) & valid;
}

__global__ __launch_bounds__(RLE_THREADS) void rle_poly_kernel(const double* __restrict__ xy, const int32_t* __restrict__ point_offsets,
                                                               int P, const int32_t* __restrict__ entry_polys, const RlePoly geo,
                                                               int rule, uint32_t* __restrict__ slots, long long slot_words,
                                                               int32_t* __restrict__ table, int32_t* __restrict__ status,
                                                               unsigned* __restrict__ ws) {
  __shared__ unsigned toggles[RLE_POLY_LDS_WORDS];
  __shared__ unsigned red[4], wsum[4], wmax[4];
  __shared__ unsigned long long red64[4];
  const int s = blockIdx.x, t = threadIdx.x;
  const int g = rle_group_find(geo.first, geo.G, s);
  const int H = geo.H[g], W = geo.W[g];
  const unsigned HW = (unsigned)H * (unsigned)W;      // < 2^31 (checked by the host entry)
  const unsigned nw = HW / 32u + 1u;                  // words of a plane of H*W + 1 bits
  const bool in_lds = nw <= (unsigned)RLE_POLY_LDS_WORDS;
  unsigned* once = ws + geo.word0[g] + (unsigned long long)(s - geo.first[g]) * (unsigned long long)nw * (in_lds ? 2u : 3u);
  unsigned* more = once + nw;
  int32_t* row = table + (size_t)s * 4;
  int32_t* stat = status + (size_t)s * 4;

  // ---- what the host codec refuses, before anything is written
  const int p0 = entry_polys[s], p1 = entry_polys[s + 1];
  unsigned bad = (p0 < 0 || p1 < p0 || p1 > P) ? 1u : 0u;      // uniform over the workgroup
  if (!bad) {
    for (int i = p0 + t; i < p1; i += RLE_THREADS)
      if (point_offsets[i + 1] - point_offsets[i] < 1 || point_offsets[i] < 0) bad = 1u;
    bad = rle_block_sum(bad, red);
  }
  if (!bad && p1 > p0) {      // every polygon has a vertex: the offsets rise and the entry's coordinates are one stretch
    const long long c1 = 2ll * point_offsets[p1];
    for (long long c = 2ll * point_offsets[p0] + t; c < c1; c += RLE_THREADS)
      if (!poly_coord_ok(xy[c])) bad = 1u;
    bad = rle_block_sum(bad, red);
  }
  unsigned long long area_sum = 0;
  for (int i = p0; i < p1 && !bad; ++i) {      // bad, i, k: uniform over the workgroup
    const int k = point_offsets[i + 1] - point_offsets[i];
    const double* pxy = xy + 2 * (size_t)point_offsets[i];
    // an edge has at most 10^6 + 1 steps (the grid spans +-5*10^5): only a polygon of thousands of vertices can reach 2^31
    if ((long long)k * 1000001ll >= (1ll << 31)) {
      unsigned long long steps = 0;
      for (int j = t; j < k; j += RLE_THREADS) steps += (unsigned long long)poly_edge_of(pxy, k, j).n + 1ull;
      if (rle_block_sum(steps, red64) >= (1ull << 31)) { bad = 1u; break; }
    }
    // two copies of the same two calls, so that each addresses its plane directly: LDS (ds_xor_b32) or the workspace
    auto polygon = [&](unsigned* T) {
      poly_toggle(T, nw, pxy, k, H, W, HW);
      return poly_fill(T, nw, HW, once, more, i == p0, red);
    };
    const unsigned a = in_lds ? polygon(toggles) : polygon(more + nw);
    area_sum += rle_block_sum(a, red);
  }
  if (bad) {
    if (t == 0) {
      row[0] = 0; row[1] = 3; row[2] = 0; row[3] = 0;
      stat[0] = 2; stat[1] = 0; stat[2] = 0; stat[3] = 0;
    }
    return;
  }

  // ---- the final mask in run order, in place of `once`: the encoder's form-1 plane
  const unsigned plane_words = (HW + 31u) / 32u;      // <= nw
  __syncthreads();      // the last polygon's planes are written
  for (unsigned w = t; w < plane_words; w += RLE_THREADS) {
    const unsigned o = p1 > p0 ? once[w] : 0u, m = p1 > p0 ? more[w] : 0u;      // an entry without a polygon: the empty mask
    once[w] = rule ? (o | m) : (o & ~m);
  }
  __syncthreads();
  const unsigned* C = once;
  unsigned trans = 0, area = 0;
  for (unsigned w = t; w < plane_words; w += RLE_THREADS) {
    trans += __popc(poly_transitions(C, w, HW));
    area += __popc(C[w]);
  }
  trans = rle_block_sum(trans, red);
  area = rle_block_sum(area, red);
  const unsigned n_counts = trans + 1u;
  const int form = (long long)n_counts <= slot_words ? 0 : ((long long)plane_words <= slot_words ? 1 : 2);
  if (t == 0) {
    row[0] = (int32_t)n_counts; row[1] = form; row[2] = (int32_t)area; row[3] = 0;
    stat[0] = 0; stat[1] = (int32_t)(area_sum < 0x7fffffffull ? area_sum : 0x7fffffffull); stat[2] = 0; stat[3] = 0;
  }
  uint32_t* slot = slots + (size_t)s * (size_t)slot_words;
  if (form == 2) return;
  if (form == 1) {
    for (unsigned w = t; w < plane_words; w += RLE_THREADS) slot[w] = C[w];
    return;
  }
  unsigned rank_base = 0, last_base = 0;
  for (unsigned base = 0; base < plane_words; base += RLE_THREADS) {
    const unsigned w = base + t;
    const unsigned long long tr = w < plane_words ? (unsigned long long)poly_transitions(C, w, HW) : 0ull;
    rle_counts_chunk(tr, 32u * w, slot, rank_base, last_base, wsum, wmax);
  }
  if (t == 0) slot[trans] = HW - last_base;
}

}  // namespace

extern "C" {

size_t hgl_rle_from_polygons_workspace_bytes(const int64_t* images_host, int G, int S, int P) {
  if (!images_host || P < 0) return 0;
  RlePoly geo;
  unsigned long long words = 0;
  char why[200];
  if (rle_poly_plan(images_host, G, S, &geo, &words, why, sizeof(why)) != 0) return 0;
  return hgl_align_up((size_t)words * sizeof(uint32_t), 256);
}

int hgl_rle_from_polygons_device(const double* xy, const int32_t* point_offsets, int P, const int32_t* entry_polys, int S,
                                 const int64_t* images_host, int G, int rule, uint32_t* slots, long long slot_words, int32_t* table,
                                 int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(images_host && S >= 0 && P >= 0 && (S == 0 || (entry_polys && slots && table && status)) &&
                  (P == 0 || (xy && point_offsets)),
              "rle_from_polygons_device: bad arguments");
  HGL_REQUIRE(rule == 0 || rule == 1, "rle_from_polygons_device: rule %d (0: covered exactly once, 1: covered at least once)", rule);
  HGL_REQUIRE(slot_words >= 1, "rle_from_polygons_device: slot_words %lld (the empty mask alone is one count)", slot_words);
  RlePoly geo;
  unsigned long long words = 0;
  char why[200];
  if (rle_poly_plan(images_host, G, S, &geo, &words, why, sizeof(why)) != 0) {
    hgl_set_error("rle_from_polygons_device: %s", why);
    return HGL_EINVAL;
  }
  if (S == 0) return HGL_OK;      // nothing to rasterise, nothing to launch
  if (!ws || ws_bytes < hgl_align_up((size_t)words * sizeof(uint32_t), 256)) {
    hgl_set_error("rle_from_polygons_device: workspace too small");
    return HGL_EWORKSPACE;
  }
  hipLaunchKernelGGL(rle_poly_kernel, dim3((unsigned)S), dim3(RLE_THREADS), 0, (hipStream_t)stream, xy, point_offsets, P, entry_polys,
                     geo, rule, slots, slot_words, table, status, (unsigned*)ws);
  return hgl_check_launch("rle_from_polygons_device");
}

}  // extern "C"
