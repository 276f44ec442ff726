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
//
// The same file paints heat-maps (hgl_heat_paint_device, further down): the scorer's guided map as colours through paint_blend.
#include "hgl_common.h"
#include "dir_ramp.h"       // dir_weight: the column weight the coherence pooling multiplies with (csrc/scoring.hip)
#include "rle_group.h"      // RlePick, RlePaint, rle_paint_plan, heat_paint_plan: plain C++, shared with tests/native/*_sanitize.cpp
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

// ---- hgl_heat_paint_device: M heat-maps -> colours on their canvases ----------------------------------------------------------
// THREE launches whatever M and the sizes are, all on the same grid: a workgroup owns one share of consecutive pixels of one map
// (heat_share: 4096 pixels, more for a map beyond 2^20 pixels, so that a map has at most 256 shares and a workgroup folds its
// map's partials with one load per thread).  No atomics, no host synchronisation, no allocation; minimum and maximum do not depend
// on the order they are taken in, so every byte is defined by the contract alone (include/hybridgl.h).
//   1. heat_minmax_kernel   per share: (min, max) of the map's values, (NaN, NaN) when one of them is NaN or +-inf
//   2. heat_peak_kernel     folds the map's (min, max) partials -- the map's first share keeps (code, mn, mx) -- and writes
//                           per share: max of g = ((x - mn) / (mx - mn)) * dir_weight(col)
//   3. heat_paint_kernel    folds the map's peak partials -- the map's first share writes the status row -- and paints: a lane
//                           owns four consecutive pixels whose first canvas pixel is a multiple of four, 12 bytes of out = three
//                           aligned words and one word of levels (base and heat come as words as well where THEIR alignment
//                           allows); the up to three pixels in front of and behind a share's groups, and every pixel of a call
//                           whose out is not word-aligned, move as bytes.  A canvas byte is read once and written once.
struct HeatBlock {
  int m, W;
  long long lo, hi;      // the share: pixels lo .. hi of map m
  unsigned b0, nb;       // the map's first partial and how many it has
};
__device__ __forceinline__ HeatBlock heat_block(const HeatPaint& geo) {
  HeatBlock s;
  s.m = rle_group_find(geo.blk0, geo.M, (unsigned)blockIdx.x);
  s.W = geo.W[s.m];
  const long long n = (long long)geo.H[s.m] * (long long)s.W, share = heat_share(n);
  s.b0 = geo.blk0[s.m];
  s.nb = geo.blk0[s.m + 1] - s.b0;
  s.lo = (long long)(blockIdx.x - s.b0) * share;      // < n: the map has ceil(n / share) shares
  s.hi = s.lo + share < n ? s.lo + share : n;
  return s;
}

// the workgroup-wide minimum / maximum of v (rle_block_max's shape); lds: 4 elements
template <bool MAX>
__device__ __forceinline__ float heat_block_fold(float v, float* lds) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const float o = __shfl_xor(v, d, 64);
    v = MAX ? fmaxf(v, o) : fminf(v, o);
  }
  __syncthreads();      // the previous use of lds is over
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return MAX ? fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3])) : fminf(fminf(lds[0], lds[1]), fminf(lds[2], lds[3]));
}

// f(value, column) for the pixels lo .. hi of a map of width W that starts at x, each once: 16-byte loads where x + lo is
// 16-byte aligned (lo is a multiple of 4096, so it is whenever the map itself is)
template <typename F>
__device__ __forceinline__ void heat_for_each(const float* __restrict__ x, long long lo, long long hi, int W, F f) {
  const float* p = x + lo;
  const long long cnt = hi - lo;
  long long done = 0;
  if (((uintptr_t)p & 15u) == 0) {
    const long long q = cnt >> 2;
    for (long long k = threadIdx.x; k < q; k += RLE_THREADS) {
      const float4 v = reinterpret_cast<const float4*>(p)[k];
      unsigned col = (unsigned)(lo + 4 * k) % (unsigned)W;      // lo + 4k < H*W < 2^31
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f(e[j], (int)col);
        col = col + 1 == (unsigned)W ? 0u : col + 1;
      }
    }
    done = 4 * q;
  }
  for (long long i = done + threadIdx.x; i < cnt; i += RLE_THREADS) f(p[i], (int)((unsigned)(lo + i) % (unsigned)W));
}

__global__ __launch_bounds__(RLE_THREADS) void heat_minmax_kernel(const float* __restrict__ heat, const HeatPaint geo,
                                                                 float2* __restrict__ part) {
  __shared__ float red[4];
  const HeatBlock s = heat_block(geo);
  float mn = INFINITY, mx = -INFINITY;
  unsigned bad = 0;
  heat_for_each(heat + geo.heat0[s.m], s.lo, s.hi, s.W, [&](float v, int) {
    bad |= paint_finite(__float_as_uint(v)) ? 0u : 1u;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  });
  unsigned* redu = reinterpret_cast<unsigned*>(red);
  bad = rle_block_max(bad, redu);
  mn = heat_block_fold<false>(mn, red);
  mx = heat_block_fold<true>(mx, red);
  if (threadIdx.x == 0) part[blockIdx.x] = bad ? make_float2(NAN, NAN) : make_float2(mn, mx);
}

// (code 0 / 1 / 2, mn, mx) of the map out of its nb <= RLE_THREADS (min, max) partials, the same in every thread
__device__ __forceinline__ int heat_fold_minmax(const float2* __restrict__ part, unsigned b0, unsigned nb, float* red, float& mn, float& mx) {
#pragma clang fp contract(off)
  float a = INFINITY, b = -INFINITY;
  unsigned bad = 0;
  if (threadIdx.x < nb) {
    const float2 v = part[b0 + threadIdx.x];
    if (v.x != v.x) bad = 1; else { a = v.x; b = v.y; }
  }
  bad = rle_block_max(bad, reinterpret_cast<unsigned*>(red));
  mn = heat_block_fold<false>(a, red);
  mx = heat_block_fold<true>(b, red);
  const float range = mx - mn;
  if (bad || !paint_finite(__float_as_uint(range))) return 2;
  return mx == mn ? 1 : 0;
}

// g of one value: the normalised value times the weight of its column, each operation rounded to fp32 on its own
__device__ __forceinline__ float heat_guided(float x, float mn, float range, int dirflag, int col, int W) {
#pragma clang fp contract(off)
  const float n = (x - mn) / range;
  const float w = dir_weight(dirflag, col, W);
  return n * w;
}

__global__ __launch_bounds__(RLE_THREADS) void heat_peak_kernel(const float* __restrict__ heat, const HeatPaint geo,
                                                               const float2* __restrict__ part, float* __restrict__ peak_part,
                                                               int32_t* __restrict__ stat) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  const HeatBlock s = heat_block(geo);
  float mn, mx;
  const int code = heat_fold_minmax(part, s.b0, s.nb, red, mn, mx);
  if (blockIdx.x == s.b0 && threadIdx.x == 0) {
    int32_t* row = stat + (size_t)s.m * 4;
    row[0] = code;
    row[1] = (int32_t)__float_as_uint(mn);
    row[2] = (int32_t)__float_as_uint(mx);
    row[3] = 0;
  }
  if (code) {      // uniform over the workgroup; the paint kernel does not read the partial of such a map
    if (threadIdx.x == 0) peak_part[blockIdx.x] = 0.f;
    return;
  }
  const float range = mx - mn;
  const int dirflag = geo.dirflag[s.m];
  float peak = -INFINITY;
  heat_for_each(heat + geo.heat0[s.m], s.lo, s.hi, s.W,
                [&](float v, int col) { peak = fmaxf(peak, heat_guided(v, mn, range, dirflag, col, s.W)); });
  peak = heat_block_fold<true>(peak, red);
  if (threadIdx.x == 0) peak_part[blockIdx.x] = peak;
}

// What a pixel becomes: level L of the ramp over `pix`.  ramp: [256,3] words in LDS.
struct HeatLook {
  const uint32_t* ramp;
  float mn, range, peak;
  int dirflag, W;
  bool live;      // code 0: a map with another code is a plain copy of its base at level 0
  __device__ __forceinline__ uint32_t at(float x, int col, uint32_t pix, uint32_t& L) const {
#pragma clang fp contract(off)
    L = 0;
    if (!live) return pix;
    const float g = heat_guided(x, mn, range, dirflag, col, W);
    const float t = g / peak;
    const int l = (int)rintf(t * 255.f);      // 0 <= g <= peak: 0 .. 255
    L = (uint32_t)(l < 0 ? 0 : (l > 255 ? 255 : l));
    return paint_blend(pix, paint_colour(ramp[3 * L]), __uint_as_float(ramp[3 * L + 1]), __uint_as_float(ramp[3 * L + 2]));
  }
};

template <bool LEVELS>
__global__ __launch_bounds__(RLE_THREADS) void heat_paint_kernel(const float* __restrict__ heat, const HeatPaint geo,
                                                                const uint32_t* __restrict__ ramp, const float* __restrict__ peak_part,
                                                                const int32_t* __restrict__ stat, const uint8_t* __restrict__ base,
                                                                uint8_t* __restrict__ out, uint8_t* __restrict__ levels,
                                                                int32_t* __restrict__ status) {
  __shared__ float red[4];
  __shared__ uint32_t lut[768];
  const HeatBlock s = heat_block(geo);
  const int32_t* st = stat + (size_t)s.m * 4;
  int code = st[0];      // uniform over the workgroup
  HeatLook look;
  look.ramp = lut;
  look.mn = __uint_as_float((uint32_t)st[1]);
  look.range = __uint_as_float((uint32_t)st[2]) - look.mn;      // mx - mn, as the peak kernel took it
  look.peak = 0.f;
  look.dirflag = geo.dirflag[s.m];
  look.W = s.W;
  if (code == 0) {
    look.peak = heat_block_fold<true>(threadIdx.x < s.nb ? peak_part[s.b0 + threadIdx.x] : -INFINITY, red);
    if (look.peak == 0.f) code = 3;
  }
  look.live = code == 0;
  if (blockIdx.x == s.b0 && threadIdx.x == 0) {
    int32_t* row = status + (size_t)s.m * 4;
    row[0] = code;
    row[1] = code ? 0 : st[1];
    row[2] = code ? 0 : st[2];
    row[3] = code ? 0 : (int32_t)__float_as_uint(look.peak);
  }
  for (int i = threadIdx.x; i < 768; i += RLE_THREADS) lut[i] = ramp[i];
  __syncthreads();

  const float* x = heat + geo.heat0[s.m];
  const uint8_t* src = base ? base + 3 * (size_t)geo.base0[s.m] : nullptr;
  const long long c0 = geo.pix0[s.m];                  // the canvas pixel of the map's pixel 0
  uint8_t* dst = out + 3 * (size_t)c0;
  const long long cnt = s.hi - s.lo;
  // [lo, lo + head) bytes | groups of four pixels, the first of each at a canvas pixel that is a multiple of 4 | bytes up to hi
  long long head = ((uintptr_t)out & 3u) == 0 ? (long long)((4u - (unsigned)((c0 + s.lo) & 3)) & 3u) : cnt;
  if (head > cnt) head = cnt;
  const long long groups = (cnt - head) >> 2, tail0 = head + 4 * groups;
  for (long long j = threadIdx.x; j < head + (cnt - tail0); j += RLE_THREADS) {
    const long long i = s.lo + (j < head ? j : tail0 + (j - head));
    uint32_t pix = 0, L;
    if (src) pix = (uint32_t)src[3 * i] | ((uint32_t)src[3 * i + 1] << 8) | ((uint32_t)src[3 * i + 2] << 16);
    pix = look.at(look.live ? x[i] : 0.f, (int)((unsigned)i % (unsigned)s.W), pix, L);
    dst[3 * i] = (uint8_t)pix;
    dst[3 * i + 1] = (uint8_t)(pix >> 8);
    dst[3 * i + 2] = (uint8_t)(pix >> 16);
    if constexpr (LEVELS) levels[c0 + i] = (uint8_t)L;
  }
  const long long i0 = s.lo + head;
  const bool heat_wide = ((uintptr_t)(x + i0) & 15u) == 0;
  const bool base_wide = src && ((uintptr_t)(src + 3 * i0) & 3u) == 0;      // then of every group: they lie 12 bytes apart
  const bool levels_wide = LEVELS && ((uintptr_t)levels & 3u) == 0;         // c0 + i is a multiple of 4
  for (long long k = threadIdx.x; k < groups; k += RLE_THREADS) {
    const long long i = i0 + 4 * k;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (look.live) {
      if (heat_wide) {
        const float4 q = *reinterpret_cast<const float4*>(x + i);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = x[i + e];
      }
    }
    uint32_t pix[4] = {0, 0, 0, 0};
    if (base_wide) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(src + 3 * i);
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
      pix[0] = w0 & 0xffffffu;
      pix[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
      pix[2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
      pix[3] = w2 >> 8;
    } else if (src) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint8_t* b = src + 3 * (i + e);
        pix[e] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16);
      }
    }
    unsigned col = (unsigned)i % (unsigned)s.W;
    uint32_t L[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      pix[e] = look.at(v[e], (int)col, pix[e], L[e]);
      col = col + 1 == (unsigned)s.W ? 0u : col + 1;
    }
    uint32_t* d = reinterpret_cast<uint32_t*>(dst + 3 * i);      // 3 * (c0 + i) is a multiple of 12 and out is word-aligned
    d[0] = pix[0] | (pix[1] << 24);
    d[1] = (pix[1] >> 8) | (pix[2] << 16);
    d[2] = (pix[2] >> 16) | (pix[3] << 8);
    if constexpr (LEVELS) {
      if (levels_wide) {
        *reinterpret_cast<uint32_t*>(levels + c0 + i) = L[0] | (L[1] << 8) | (L[2] << 16) | (L[3] << 24);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) levels[c0 + i + e] = (uint8_t)L[e];
      }
    }
  }
}

// the workspace of a heat paint: the (min, max) and the peak partials, one of each per workgroup, and (code, mn, mx, 0) per map
struct HeatPaintWs {
  size_t minmax, peak, stat, total;
};
HeatPaintWs heat_paint_ws(const HeatPaintPlan& plan) {
  HeatPaintWs w;
  w.minmax = 0;
  w.peak = hgl_align_up((size_t)plan.blocks * sizeof(float2), 256);
  w.stat = w.peak + hgl_align_up((size_t)plan.blocks * sizeof(float), 256);
  w.total = w.stat + hgl_align_up((size_t)plan.p.M * 4 * sizeof(int32_t), 256);
  return w;
}

}  // namespace

extern "C" {

size_t hgl_heat_paint_workspace_bytes(const int64_t* maps_host, int M, long long heat_elems, long long canvas_pixels) {
  if (!maps_host) return 0;
  HeatPaintPlan plan;
  char why[200];
  // where base and out lie is the call's business: here only the geometry counts
  if (heat_paint_plan(maps_host, M, heat_elems, canvas_pixels, 0, 0, &plan, why, sizeof(why)) != 0) return 0;
  return heat_paint_ws(plan).total;
}

int hgl_heat_paint_device(const float* heat, long long heat_elems, const int64_t* maps_host, int M, const uint32_t* ramp,
                          const uint8_t* base, uint8_t* out, long long canvas_pixels, uint8_t* levels, int32_t* status,
                          void* ws, size_t ws_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(heat && maps_host && ramp && out && status, "heat_paint_device: bad arguments");
  HeatPaintPlan plan;
  char why[200];
  if (heat_paint_plan(maps_host, M, heat_elems, canvas_pixels, (uintptr_t)base, (uintptr_t)out, &plan, why, sizeof(why)) != 0) {
    hgl_set_error("heat_paint_device: %s", why);
    return HGL_EINVAL;
  }
  const HeatPaintWs w = heat_paint_ws(plan);
  if (!ws || ws_bytes < w.total) {
    hgl_set_error("heat_paint_device: workspace too small");
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* wsb = (char*)ws;
  float2* part = (float2*)(wsb + w.minmax);
  float* peak_part = (float*)(wsb + w.peak);
  int32_t* stat = (int32_t*)(wsb + w.stat);
  // three launches whatever M and the sizes are, one workgroup per share of a map in each
  const dim3 grid((unsigned)plan.blocks), block(RLE_THREADS);
  hipLaunchKernelGGL(heat_minmax_kernel, grid, block, 0, st, heat, plan.p, part);
  hipLaunchKernelGGL(heat_peak_kernel, grid, block, 0, st, heat, plan.p, (const float2*)part, peak_part, stat);
  auto paint = levels ? heat_paint_kernel<true> : heat_paint_kernel<false>;
  hipLaunchKernelGGL(paint, grid, block, 0, st, heat, plan.p, ramp, (const float*)peak_part, (const int32_t*)stat, base, out, levels, status);
  return hgl_check_launch("heat_paint_device");
}

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
