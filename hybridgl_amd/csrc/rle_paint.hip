// Encoded masks painted onto RGB canvases on the device (hgl_rle_paint_device): the paint-side sibling of the grouped decoder.
// An ordered list of K positions, each naming one entry of its image and carrying a style, is composited onto the canvases of
// G images of their own sizes.  The work is done on the runs: no byte mask exists anywhere and nothing is read back.
//
// FOUR launches whatever G, K and the sizes are (ONE for K = 0: the bases are still copied); no host synchronisation, no
// allocation, no atomics; every output byte has one writer, so two calls give the same bytes.
//
//   1, 2. rle_stage_picked (rle.hip's starts kernel and plane kernel over the LIST, geometry RlePick): for every list position
//      the status row (code, area, 0, 0) of the entry it names -- code 3 when it names none -- and the entry's 64-bit column
//      words in the workspace: word x*HW64 + j = rows 64j .. 64j+63 of column x, padding bits clear.  An entry that no position
//      names is never touched; one that two positions name is staged twice.
//   3. rle_paint_status_kernel   one workgroup per position: code 4 when a weight is not finite, else the pixels of the edge,
//      pop-counted over the position's plane words and block-reduced into column 2 of the status row.
//   4. rle_paint_kernel<LABELS>  one wave per tile of 64 columns x 64 rows of one canvas, one lane per column.  The lane reads
//      its 64 pixels once (3 bytes each, packed into one register per pixel), walks the image's positions in list order -- the
//      position's mask word M is one load, the words above and below and of the two neighbouring columns give the edge -- and
//      blends in registers; then every row leaves as one run of 192 contiguous bytes per wave.  A canvas byte is read once and
//      written once however many positions cover it.  Canvases start at any byte (3 * pixel offset), so the kernel moves bytes.
#include "hgl_common.h"
#include "rle_group.h"      // RlePick, RlePaint, rle_paint_plan: plain C++, shared with tests/native/rle_paint_sanitize.cpp
#include "rle_scan.h"       // RLE_THREADS, rle_block_sum, rle_group_find, rle_starts_bytes, rle_stage_picked

namespace {

constexpr uint32_t PAINT_FILL = 1u << 24, PAINT_OUTLINE = 1u << 25;

// 0x00RRGGBB -> the pixel as the kernel holds it: byte 0 = R, as in memory
__device__ __forceinline__ uint32_t paint_colour(uint32_t rgb) {
  return ((rgb >> 16) & 255u) | (rgb & 0xff00u) | ((rgb & 255u) << 16);
}

__device__ __forceinline__ bool paint_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

// The pixels of word j of column x of plane P (m = P[x*HW64 + j]) that lack a set neighbour above, below, left or right; a
// neighbour outside the image counts as clear (the padding bits of a word are clear, and so is what lies beyond the plane).
__device__ __forceinline__ unsigned long long paint_edge_word(const unsigned long long* __restrict__ P, int x, int j, int W, int HW64,
                                                              unsigned long long m) {
  const size_t q = (size_t)x * (size_t)HW64 + (size_t)j;
  const unsigned long long above = j > 0 ? P[q - 1] >> 63 : 0ull;
  const unsigned long long below = j + 1 < HW64 ? P[q + 1] << 63 : 0ull;
  const unsigned long long left = x > 0 ? P[q - (size_t)HW64] : 0ull;
  const unsigned long long right = x + 1 < W ? P[q + (size_t)HW64] : 0ull;
  return m & ~(((m << 1) | above) & ((m >> 1) | below) & left & right);
}

// sat_u8(rint(f32(c) * a + f32(k) * b)) on the three channels of a pixel: both products and the sum rounded to fp32 each (no
// fused multiply-add: the pragma binds whatever the command line says), rint to nearest even, the clamp written as comparisons,
// so that a NaN (an overflowed product against one of the other sign) gives 0.
__device__ __forceinline__ uint32_t paint_blend(uint32_t pix, uint32_t colour, float a, float b) {
#pragma clang fp contract(off)
  uint32_t out = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float c = (float)((pix >> (8 * ch)) & 255u), k = (float)((colour >> (8 * ch)) & 255u);
    const float ca = c * a;
    const float kb = k * b;
    const float v = rintf(ca + kb);
    const float s = v >= 255.0f ? 255.0f : (v > 0.0f ? v : 0.0f);
    out |= (uint32_t)s << (8 * ch);
  }
  return out;
}

__global__ __launch_bounds__(RLE_THREADS) void rle_paint_status_kernel(const unsigned long long* __restrict__ plane,
                                                                      const uint32_t* __restrict__ style, const RlePaint geo,
                                                                      int32_t* __restrict__ status) {
  __shared__ unsigned red[4];
  const int t = blockIdx.x;
  int32_t* row = status + (size_t)t * 4;
  if (row[0] > 1) return;      // 2 or 3: (code, 0, 0, 0) stands; uniform over the workgroup
  if (!paint_finite(style[(size_t)t * 4 + 1]) || !paint_finite(style[(size_t)t * 4 + 2])) {
    if (threadIdx.x == 0) row[0] = 4;
    return;
  }
  const int g = rle_group_find(geo.first, geo.G, t);
  const int H = geo.H[g], W = geo.W[g], HW64 = (H + 63) / 64;
  const unsigned Q = (unsigned)W * (unsigned)HW64;
  const unsigned long long* P = plane + (size_t)geo.word0[g] + (size_t)(t - geo.first[g]) * Q;
  unsigned edge = 0;
  for (unsigned q = threadIdx.x; q < Q; q += RLE_THREADS) {
    const unsigned long long m = P[q];
    if (m) edge += __popcll(paint_edge_word(P, (int)(q / (unsigned)HW64), (int)(q % (unsigned)HW64), W, HW64, m));
  }
  edge = rle_block_sum(edge, red);
  if (threadIdx.x == 0) row[2] = (int32_t)edge;
}

template <bool LABELS>
__global__ __launch_bounds__(RLE_THREADS) void rle_paint_kernel(const unsigned long long* __restrict__ plane,
                                                               const int32_t* __restrict__ status, const uint32_t* __restrict__ style,
                                                               const RlePaint geo, unsigned tiles, const uint8_t* __restrict__ base,
                                                               uint8_t* __restrict__ out, int32_t* __restrict__ labels) {
  // the wave's rank, as a scalar: everything up to the lane's column is then uniform and the geometry is read with scalar loads
  const unsigned tile = blockIdx.x * (RLE_THREADS / 64) + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (tile >= tiles) return;
  const int lane = threadIdx.x & 63;
  const int g = rle_group_find(geo.tile0, geo.G, tile);
  const int H = geo.H[g], W = geo.W[g], HW64 = (H + 63) / 64, col_tiles = (W + RLE_PAINT_TILE - 1) / RLE_PAINT_TILE;
  const unsigned local = tile - geo.tile0[g];
  const int j = (int)(local / (unsigned)col_tiles), x = (int)(local % (unsigned)col_tiles) * RLE_PAINT_TILE + lane;
  if (x >= W) return;      // no barrier and no cross-lane operation below
  const int y0 = 64 * j;
  const int rows = H - y0 < 64 ? H - y0 : 64;
  const size_t p = (size_t)geo.pix0[g] + (size_t)y0 * (size_t)W + (size_t)x;      // (y0 + r) * W + x < H * W for r < rows

  uint32_t pix[64];
  int lab[LABELS ? 64 : 1];
#pragma unroll
  for (int r = 0; r < 64; ++r) {
    pix[r] = 0;
    if constexpr (LABELS) lab[r] = -1;
    if (base && r < rows) {
      const uint8_t* s = base + 3 * (p + (size_t)r * (size_t)W);
      pix[r] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
    }
  }

  const int k0 = geo.first[g], k1 = geo.first[g + 1];
  const size_t Q = (size_t)W * (size_t)HW64;
  for (int t = k0; t < k1; ++t) {
    if (status[(size_t)t * 4] > 1) continue;      // 2, 3, 4: the position paints nothing
    const uint32_t w0 = style[(size_t)t * 4];
    const bool fill = w0 & PAINT_FILL, line = w0 & PAINT_OUTLINE;
    const unsigned long long* P = plane + (size_t)geo.word0[g] + (size_t)(t - k0) * Q;
    const unsigned long long m = P[(size_t)x * (size_t)HW64 + (size_t)j];
    if (!m) continue;
    const unsigned long long edge = line ? paint_edge_word(P, x, j, W, HW64, m) : 0ull;
    const unsigned long long body = fill ? m : 0ull;
    if (!(body | edge)) continue;
    const float a = __uint_as_float(style[(size_t)t * 4 + 1]), b = __uint_as_float(style[(size_t)t * 4 + 2]);
    const uint32_t colour = paint_colour(w0), ink = paint_colour(style[(size_t)t * 4 + 3]);
#pragma unroll
    for (int r = 0; r < 64; ++r) {
      if ((body >> r) & 1ull) pix[r] = paint_blend(pix[r], colour, a, b);
      if ((edge >> r) & 1ull) pix[r] = ink;
      if constexpr (LABELS)
        if (((body | edge) >> r) & 1ull) lab[r] = t - k0;
    }
  }

#pragma unroll
  for (int r = 0; r < 64; ++r) {
    if (r < rows) {
      uint8_t* d = out + 3 * (p + (size_t)r * (size_t)W);
      d[0] = (uint8_t)pix[r];
      d[1] = (uint8_t)(pix[r] >> 8);
      d[2] = (uint8_t)(pix[r] >> 16);
      if constexpr (LABELS) labels[p + (size_t)r * (size_t)W] = lab[r];
    }
  }
}

// the workspace of a paint: one row of run starts and one plane per list position (the status rows are the caller's)
struct RlePaintWs {
  size_t E, plane, total;
};
RlePaintWs rle_paint_ws(const RlePaintPlan& plan, int K, long long sw) {
  RlePaintWs w;
  w.E = 0;
  w.plane = rle_starts_bytes(K, sw);
  w.total = w.plane + hgl_align_up((size_t)plan.pick.pos.words * sizeof(unsigned long long), 256);
  return w;
}

}  // namespace

extern "C" {

size_t hgl_rle_paint_workspace_bytes(const int64_t* images_host, int G, int S, long long slot_words, int K, long long canvas_pixels) {
  if (!images_host || K <= 0) return 0;
  RlePaintPlan plan;
  char why[200];
  // where base and out lie is the call's business: here only the geometry counts
  if (rle_paint_plan(images_host, G, S, K, slot_words, canvas_pixels, 0, 0, &plan, why, sizeof(why)) != 0) return 0;
  return rle_paint_ws(plan, K, slot_words).total;
}

int hgl_rle_paint_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S, const int32_t* order,
                         const uint32_t* style, int K, const int64_t* images_host, int G, const uint8_t* base, uint8_t* out,
                         long long canvas_pixels, int32_t* labels, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(images_host && out && (S <= 0 || (slots && table)) && (K <= 0 || (order && style && status)),
              "rle_paint_device: bad arguments");
  RlePaintPlan plan;
  char why[200];
  if (rle_paint_plan(images_host, G, S, K, slot_words, canvas_pixels, (uintptr_t)base, (uintptr_t)out, &plan, why, sizeof(why)) != 0) {
    hgl_set_error("rle_paint_device: %s", why);
    return HGL_EINVAL;
  }
  const RlePaintWs w = rle_paint_ws(plan, K, slot_words);
  if (K > 0 && (!ws || ws_bytes < w.total)) {
    hgl_set_error("rle_paint_device: workspace too small");
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* wsb = (char*)ws;
  const unsigned long long* plane = K > 0 ? (const unsigned long long*)(wsb + w.plane) : nullptr;
  // four launches whatever G, K and the sizes are; the paint kernel alone for K = 0 (a plain copy of the bases)
  if (K > 0) {
    plan.pick.order = order;
    rle_stage_picked(slots, slot_words, table, K, plan.pick, (uint32_t*)(wsb + w.E), status, (unsigned long long*)(wsb + w.plane), stream);
    hipLaunchKernelGGL(rle_paint_status_kernel, dim3((unsigned)K), dim3(RLE_THREADS), 0, st, plane, style, plan.p, status);
  }
  const unsigned blocks = (unsigned)((plan.tiles + RLE_THREADS / 64 - 1) / (RLE_THREADS / 64));
  auto paint = labels ? rle_paint_kernel<true> : rle_paint_kernel<false>;
  hipLaunchKernelGGL(paint, dim3(blocks), dim3(RLE_THREADS), 0, st, plane, (const int32_t*)status, style, plan.p, (unsigned)plan.tiles, base,
                     out, labels);
  return hgl_check_launch("rle_paint_device");
}

}  // extern "C"
