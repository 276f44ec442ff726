// Scoring tail + image synthesis kernels (all HBM / latency bound, no matrix work).
//   calculate_score      model/backbone.py:74-87
//   coherence scores     Hybridgl_main.py:201-223 (+ gen_dir_mask utils.py:135-161)
//   IoU                  utils.py:365-384
//   score_sentence       Hybridgl_main.py:153-196,225-228 (+ relation_boxes utils.py:240-268)
//   synthesize_views     Hybridgl_main.py:93-125
#include "hgl_common.h"
#include "dir_ramp.h"      // linspace_at, dir_weight: shared with csrc/rle_paint.hip
#include <mutex>
#include <vector>
#include <condition_variable>
#include <math.h>
#include <stdio.h>
#include <string.h>

namespace {

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- calculate_score: one wave per (n,t) ----
__global__ __launch_bounds__(256) void calc_score_kernel(const float* __restrict__ img,
                                                         const float* __restrict__ txt, int N, int T,
                                                         int E, float logit_scale,
                                                         float* __restrict__ logits) {
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= N * T) return;
  const int n = pair / T, tt = pair - n * T;
  const float* ir = img + (long long)n * E;
  const float* tr = txt + (long long)tt * E;
  float si = 0.f, stx = 0.f;
  for (int i = lane; i < E; i += 64) {
    si += ir[i] * ir[i];
    stx += tr[i] * tr[i];
  }
  const float ni = sqrtf(wave_sum_f(si)), nt = sqrtf(wave_sum_f(stx));
  float d = 0.f;
  for (int i = lane; i < E; i += 64) d += (logit_scale * (ir[i] / ni)) * (tr[i] / nt);
  d = wave_sum_f(d);
  if (lane == 0) logits[pair] = d;
}

// ---- heat-map statistics ----
// stats[0]=min, stats[1]=max (as ordered-int encodings), reduced with atomics on monotone keys
__device__ __forceinline__ int f2ord(float f) {
  int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

__global__ __launch_bounds__(256) void minmax_kernel(const float* __restrict__ a, long long n,
                                                     int* __restrict__ stats) {
  float mn = INFINITY, mx = -INFINITY;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const float v = a[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o));
    mx = fmaxf(mx, __shfl_xor(mx, o));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&stats[0], f2ord(mn));
    atomicMax(&stats[1], f2ord(mx));
  }
}

__global__ void init_stats_kernel(int* stats) {
  stats[0] = 0x7fffffff;          // +max ordered key
  stats[1] = (int)0x80000000;     // -max ordered key
}

// Masked pooling.  One block = PIX_PER_BLOCK consecutive pixels x all masks.
// The normalised heat-map tile lives in registers (16 px per lane); each mask's bytes
// are read exactly once with 16-byte loads; partial sums (double) go to part[blk][n].
constexpr int PX_LANE = 16;
constexpr int PIX_PER_BLOCK = 256 * PX_LANE;  // 4096

// masks per pooling workgroup (blockIdx.y), both by measurement: 8 for the per-sentence pooling and for hgl_score_ref (the
// launch of a single ref needs the workgroups: 130 against 139 us with 32), 32 for hgl_score_group (three sentences of up to
// sixteen refs per launch are enough workgroups without splitting the masks eight ways, and the normalised heat-map values of a
// block's pixels -- a division and a direction weight per pixel -- are computed once per 32 masks instead of once per 8).  The
// partial sums per (mask, part) do not depend on the grouping.
constexpr int MASK_GROUP = 8;
constexpr int REF_MASK_GROUP = 32;

// ---- the pooling of a block, shared by the pooling kernels (one heat-map / the maps of the rows of a table) --------------------
// One workgroup = PIX_PER_BLOCK consecutive pixels x a group of masks x UP TO FOUR heat-maps at once: the normalised values of
// the maps at the lane's 16 pixels live in registers (16 VGPRs per map), and a mask's 16 bytes are loaded ONCE, turned into
// sixteen 0.0 / 1.0 floats once, and multiplied into all the maps: cvt + one fma per (pixel, map) instead of a 64-bit select
// and a double-precision add per (pixel, map) and a re-read of the bytes per map.  (Until round 5 every (block, group, map) was
// its own workgroup with a double-precision sum per pixel: 130 vector instructions per KiB of mask bytes and map, the bytes
// fetched S times -- 1.37 TB/s on the algorithmic bytes, instruction-bound.)
// Arithmetic of one (map, mask, wave) partial -- THE definition the pooling kernels share, so their results are the same bits:
//   lane: a = 0; for e = 0..15 in order: a = fma(m_e, v_e, a) in fp32 (m_e is 0 or 1: the products are exact, the 16-term sum
//   carries at most a few 1e-8 of relative error); the 64 lane sums folded in fp32 by pool_sum_f's fixed DPP tree; the wave's
//   sum widened to double; partials over a mask's waves are added in double by the scoring kernels as before.
// The partials give a mask's INSIDE sum and the map's total; the final reductions (coherence_final_kernel, ref_coherence_body)
// take the outside sum as  total - inside  while the mask leaves at least half of the plane outside (or covers all of it), and
// otherwise sum the outside pixels themselves in double (pool_outside_sum, one function for both reductions: the entries stay
// the same bits) -- the float32 roundings of two large sums must not be divided by a small outside count.
struct PoolMap {
  const float* attn;   // the heat-map
  int dirflag, sidx;   // gen_dir_mask weight; index of the map in the partial arrays
  float mn, range;     // min and (max - min) of the map
};

// dir_weight(dirflag, x, W) with everything that does not depend on x computed once per map: the weight of a column is
// linspace_at on one of at most two segments (dirflag 3: the two ramps of `middle`; 0: the constant 1 as a ramp of step 0).
// Same operations on the same values as dir_weight / linspace_at: same bits.
struct DirRamp {
  int xsplit;                       // columns < xsplit lie on segment A, the others on segment B (index x - xsplit)
  float stepA, startA, endA, stepB, startB, endB;
  int stepsA, halfA, stepsB, halfB;
  __device__ __forceinline__ void seg(float start, float end, int steps, float& st, float& s0, float& e0, int& n, int& h) {
    if (steps <= 1) { st = 0.f; s0 = start; e0 = start; n = 1; h = 1; return; }     // linspace_at: steps == 1 -> start
    st = (end - start) / (float)(steps - 1);
    s0 = start; e0 = end; n = steps; h = steps / 2;
  }
  __device__ __forceinline__ void init(int dirflag, int W) {
    xsplit = W;
    seg(1.f, 1.f, W, stepB, startB, endB, stepsB, halfB);
    if (dirflag == 1) seg(1.f, 0.f, W, stepA, startA, endA, stepsA, halfA);
    else if (dirflag == 2) seg(0.f, 1.f, W, stepA, startA, endA, stepsA, halfA);
    else if (dirflag == 3) {
      const int w1 = W / 2;
      xsplit = w1;
      seg(0.f, 1.f, w1, stepA, startA, endA, stepsA, halfA);
      seg(1.f, 0.f, W - w1, stepB, startB, endB, stepsB, halfB);
    } else {
      stepA = 0.f; startA = 1.f; endA = 1.f; stepsA = W; halfA = W;      // fma(0, i, 1) == 1
    }
  }
  __device__ __forceinline__ float at(int x) const {
    const bool a = x < xsplit;
    const int i = a ? x : x - xsplit;
    const float st = a ? stepA : stepB, s0 = a ? startA : startB, e0 = a ? endA : endB;
    const int n = a ? stepsA : stepsB, h = a ? halfA : halfB;
    return i < h ? fmaf(st, (float)i, s0) : fmaf(-st, (float)(n - i - 1), e0);
  }
};

// Sum over the 64 lanes for the pooling loop (EXEC all ones there), on the VALU alone, in fp32: six adds whose second operand
// comes through DPP (quad_perm xor 1, xor 2, row_half_mirror, row_mirror: every lane then holds its row's sum; row_bcast:15 into
// rows 1 and 3, row_bcast:31 into rows 2 and 3) -- the total, ((r2 + r3) + (r0 + r1)), ends in lanes 48..63.  One instruction
// per step (v_add_f32 with a DPP operand).  (__shfl_xor compiles to ds_bpermute_b32: a double-precision butterfly was twelve
// LDS-crossbar operations and six adds per (mask, map), as much of the loop as its arithmetic; the DPP form in double costs three
// instructions per step.)  The wave's 1024 products are thus summed in fp32 -- as the reference sums ALL its products
// (Hybridgl_main.py:221, torch.sum of an fp32 tensor) -- in a fixed tree: deterministic, and the same function in all
// pooling kernels; partials of different waves are added in double by the scoring kernels.
template <int CTRL, int ROWS>
__device__ __forceinline__ float pool_dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROWS, 0xf, false));
}
__device__ __forceinline__ float pool_sum_f(float v) {      // valid in lanes 48..63 (read it in lane 63)
  v += pool_dpp_f<0xB1, 0xf>(v);      // quad_perm [1,0,3,2]
  v += pool_dpp_f<0x4E, 0xf>(v);      // quad_perm [2,3,0,1]
  v += pool_dpp_f<0x141, 0xf>(v);     // row_half_mirror
  v += pool_dpp_f<0x140, 0xf>(v);     // row_mirror
  v += pool_dpp_f<0x142, 0xa>(v);     // row_bcast:15 -> rows 1, 3 (the other rows add 0)
  v += pool_dpp_f<0x143, 0xc>(v);     // row_bcast:31 -> rows 2, 3
  return v;
}
__device__ __forceinline__ unsigned pool_sum_u(unsigned v) {   // valid in lanes 48..63
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false);
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false);
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
  return v;
}

typedef unsigned pool_u32x4 __attribute__((ext_vector_type(4)));
typedef pool_u32x4 pool_u32x4_u __attribute__((aligned(1)));     // 16 bytes at ANY address: one global_load_dwordx4 (the hardware takes
typedef f32x4 pool_f32x4_u __attribute__((aligned(4)));          // unaligned vector loads; a plane of an odd-sized image starts anywhere)

// FULL: the whole block of PIX_PER_BLOCK pixels lies inside the plane (wave-uniform; every block but the last one of a plane):
// no per-pixel predicate anywhere.  !FULL: the last block, pixel by pixel with predicates -- instantiated for one map only.
template <int NS, bool FULL>
__device__ __forceinline__ void pool_block(int blk, const PoolMap (&pm)[NS], int n0, int n1, const uint8_t* __restrict__ masks, int N, int H,
                                           int W, bool write_tot, double* __restrict__ part_sum, unsigned* __restrict__ part_cnt,
                                           double* __restrict__ part_tot, int nparts) {
  const long long HW = (long long)H * W;
  const long long p0 = (long long)blk * PIX_PER_BLOCK + threadIdx.x * PX_LANE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long part = (long long)blk * 4 + wave;      // one partial per wave: no block sync
  float v[NS][PX_LANE];
  const int xcol0 = (int)(p0 % W);      // ONE 64-bit division per lane; the pixels' columns follow by increment and wrap
  int cnt_map = -1;                     // the map (if any of these) that files the pixel counts: sidx == 0
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const float* attn = pm[j].attn;
    float raw[PX_LANE];      // four 16-byte loads issued together (sixteen conditional scalar loads are sixteen round trips)
    if (FULL) {
      const f32x4 r0 = *(const pool_f32x4_u*)(attn + p0), r1 = *(const pool_f32x4_u*)(attn + p0 + 4);
      const f32x4 r2 = *(const pool_f32x4_u*)(attn + p0 + 8), r3 = *(const pool_f32x4_u*)(attn + p0 + 12);
#pragma unroll
      for (int e = 0; e < 4; ++e) { raw[e] = r0[e]; raw[4 + e] = r1[e]; raw[8 + e] = r2[e]; raw[12 + e] = r3[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < PX_LANE; ++e) raw[e] = attn[min(p0 + e, HW - 1)];
    }
    int xcol = xcol0;
    DirRamp ramp;
    ramp.init(pm[j].dirflag, W);
    // the map's total over the wave's pixels in EXACTLY the arithmetic of a mask that covers them all (fma by 1.0 in order, the
    // same fold over the lanes): for a full mask  total - sum  is then 0 and the "outside" mean 0 / 0 = NaN, as in the reference
    // (Hybridgl_main.py:221: every term of its sum is x * 0 / 0) -- not +-inf from two roundings of the same sum
    float ta = 0.f;
#pragma unroll
    for (int e = 0; e < PX_LANE; ++e) {
      float val = ((raw[e] - pm[j].mn) / pm[j].range) * ramp.at(xcol);
      if (!FULL && p0 + e >= HW) val = 0.f;
      v[j][e] = val;
      ta = __builtin_fmaf(1.0f, val, ta);
      if (++xcol >= W) xcol = 0;
    }
    if (write_tot) {
      const float tot = pool_sum_f(ta);
      if (lane == 63) part_tot[(long long)pm[j].sidx * nparts + part] = (double)tot;
    }
    if (pm[j].sidx == 0) cnt_map = j;
  }
  for (int n = n0; n < n1; ++n) {
    const uint8_t* m = masks + (long long)n * HW + p0;
    unsigned w4[4] = {0u, 0u, 0u, 0u};
    if (FULL) {
      const pool_u32x4 mv = *(const pool_u32x4_u*)m;
      w4[0] = mv.x; w4[1] = mv.y; w4[2] = mv.z; w4[3] = mv.w;
    } else {      // byte loads at clamped addresses, pixels beyond the plane count as 0
#pragma unroll
      for (int e = 0; e < PX_LANE; ++e) {
        const long long pe = min(p0 + e, HW - 1) - p0;
        const unsigned byte = p0 + e < HW ? (unsigned)m[pe] : 0u;
        w4[e >> 2] |= byte << (8 * (e & 3));
      }
    }
    unsigned c = 0;
    float mf[PX_LANE];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // every byte -> (byte != 0): bit 7 of ((b & 0x7f) + 0x7f) | b is set exactly for b != 0 (no carry crosses a byte)
      const unsigned w = w4[q];
      const unsigned nz = ((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) >> 7) & 0x01010101u;
      c += (unsigned)__popc(nz);
      mf[4 * q + 0] = (float)(nz & 0xffu);
      mf[4 * q + 1] = (float)((nz >> 8) & 0xffu);
      mf[4 * q + 2] = (float)((nz >> 16) & 0xffu);
      mf[4 * q + 3] = (float)(nz >> 24);
    }
    float sum[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      float a = 0.f;
#pragma unroll
      for (int e = 0; e < PX_LANE; ++e) a = __builtin_fmaf(mf[e], v[j][e], a);
      sum[j] = a;
    }
    // the folds of the maps and of the count in ONE basic block (their DPP steps interleave and fill each other's wait states),
    // then all the stores of lane 63 behind one branch
#pragma unroll
    for (int j = 0; j < NS; ++j) sum[j] = pool_sum_f(sum[j]);
    c = pool_sum_u(c);
    if (lane == 63) {
#pragma unroll
      for (int j = 0; j < NS; ++j) part_sum[((long long)pm[j].sidx * nparts + part) * N + n] = (double)sum[j];
      if (cnt_map >= 0) part_cnt[part * N + n] = c;
    }
  }
}

// ---- the outside sum of a mask that leaves little outside ---------------------------------------------------------------------
// The final reductions take a mask's outside sum as  total - inside.  Both are sums of float32 wave partials: each carries up to
// 22 roundings of its own size (15 adds in a lane, 6 folds, the widening exact), so the difference is off by up to
// 22 u (total + inside), u = 2^-24 -- harmless beside an outside sum of the total's size, but divided by a small one it is
// the whole error of the score: with one pixel outside a 64 x 65 plane the score missed the bound of
// tests/coherence_cases.py 117 times over.
// Switch point.  tests/coherence_cases.py allows an implementation C = 64 roundings of  |in| + |out|, of which the reference's
// own rounding of its mean, of a / mean and of the result take 3.  With f = (HW - c) / HW the outside share of the plane and a
// heat-map spread evenly over it (outside sum = f total), the outside term is  black / f * (1 - inside / total), and the up to
// 22 + 22 roundings of inside / total reach it multiplied by (1 - f) / f:  44 (1 - f) / f + 3 <= 64  <=>  f >= 0.42.  The switch is
// the next plain value above that, f < 1/2: a mask that covers more than half of the plane (and not all of it) has its outside
// pixels summed directly.  (The 1 % .. 40 % masks of the benchmark and SAM's proposals but for a background-sized one stay on
// the subtraction; a full mask does too: its  total - inside  is 0 bit for bit and the outside mean 0 / 0 = NaN, see pool_block.)
__device__ __forceinline__ bool pool_outside_direct(unsigned long long c, long long HW) {
  return (long long)c < HW && 2 * (HW - (long long)c) < HW;
}
// The direct sum, by ONE WHOLE WAVE (all 64 lanes call it with the same arguments; the result is valid in every lane): lane l
// walks the 16-pixel runs l, l + 64, ... of the plane with pool_block's 16-byte mask loads and its byte -> (byte != 0) rule,
// and adds the normalised value of every pixel outside the mask -- the same float32 expression as pool_block's, same bits -- in
// double, in pixel order; the lanes are folded by wave_sum_d's fixed butterfly.  Deterministic; no float32 sum at all.  At most
// half of the plane's values are computed, and a run without an outside pixel costs its mask load alone.  Out of line: the
// reductions that call it are latency-bound loops unrolled four masks wide, and this is their cold path.
__device__ __noinline__ double pool_outside_sum(const float* __restrict__ attn, const uint8_t* __restrict__ m, long long HW, int W,
                                                int dirflag, float mn, float range) {
  const int lane = threadIdx.x & 63;
  DirRamp ramp;
  ramp.init(dirflag, W);
  double acc = 0.0;
  for (long long p0 = (long long)lane * PX_LANE; p0 < HW; p0 += 64ll * PX_LANE) {
    unsigned w4[4] = {0u, 0u, 0u, 0u};
    if (p0 + PX_LANE <= HW) {
      const pool_u32x4 mv = *(const pool_u32x4_u*)(m + p0);
      w4[0] = mv.x; w4[1] = mv.y; w4[2] = mv.z; w4[3] = mv.w;
    } else {      // the plane's last run: byte loads, pixels beyond the plane count as inside (never summed, never read)
#pragma unroll
      for (int e = 0; e < PX_LANE; ++e) {
        const unsigned byte = p0 + e < HW ? (unsigned)m[e + p0] : 1u;
        w4[e >> 2] |= byte << (8 * (e & 3));
      }
    }
    unsigned out16 = 0;      // bit e: pixel p0 + e lies outside the mask
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned w = w4[q];
      const unsigned z = ~((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) >> 7) & 0x01010101u;      // 1 per zero byte (as pool_block)
      out16 |= ((z & 1u) | ((z >> 7) & 2u) | ((z >> 14) & 4u) | ((z >> 21) & 8u)) << (4 * q);
    }
    if (out16 == 0) continue;
    int xcol = (int)(p0 % W);
#pragma unroll 1
    for (int e = 0; e < PX_LANE; ++e) {
      if ((out16 >> e) & 1u) acc += (double)(((attn[p0 + e] - mn) / range) * ramp.at(xcol));
      if (++xcol >= W) xcol = 0;
    }
  }
  return wave_sum_d(acc);
}

// The kernels below come in pairs: the main launch covers the blocks that lie wholly inside the plane (FULL: HW / PIX_PER_BLOCK
// of them -- all 100 of a 640 x 640 plane), a second, small launch the partial last block when there is one (!FULL, one map at a
// time; its 16 byte loads per lane and predicates would otherwise set the register count of the main kernel).
template <bool FULL>
__global__ __launch_bounds__(256) void masked_pool_kernel(const float* __restrict__ attn,
                                                          const uint8_t* __restrict__ masks, int N,
                                                          int H, int W, int dirflag,
                                                          const int* __restrict__ stats,
                                                          double* __restrict__ part_sum,
                                                          unsigned* __restrict__ part_cnt,
                                                          double* __restrict__ part_tot, int blk0) {
  const float mn = ord2f(stats[0]), mx = ord2f(stats[1]);
  const PoolMap pm[1] = {{attn, dirflag, 0, mn, mx - mn}};
  const int n0 = blockIdx.y * MASK_GROUP;
  pool_block<1, FULL>(blk0 + blockIdx.x, pm, n0, min(N, n0 + MASK_GROUP), masks, N, H, W, blockIdx.y == 0, part_sum, part_cnt, part_tot, 0);
}

// one wave per mask: lanes stride over the per-wave partials in a fixed pattern, then a fixed-order
// butterfly -- deterministic run to run
__global__ __launch_bounds__(256) void coherence_final_kernel(const double* __restrict__ part_sum,
                                                              const unsigned* __restrict__ part_cnt,
                                                              const double* __restrict__ part_tot,
                                                              int nblk, int N, long long HW,
                                                              float black, float* __restrict__ score,
                                                              const float* __restrict__ attn, const uint8_t* __restrict__ masks, int W,
                                                              int dirflag, const int* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  double tot = 0.0, s = 0.0;
  unsigned long long c = 0;
  for (int b = lane; b < nblk; b += 64) {
    tot += part_tot[b];
    s += part_sum[(long long)b * N + n];
    c += part_cnt[(long long)b * N + n];
  }
  tot = wave_sum_d(tot);
  s = wave_sum_d(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  double outside = tot - s;
  if (pool_outside_direct(c, HW)) {      // wave-uniform: tot, s and c are the same in all lanes
    const float mn = ord2f(stats[0]), mx = ord2f(stats[1]);
    outside = pool_outside_sum(attn, masks + (long long)n * HW, HW, W, dirflag, mn, mx - mn);
  }
  if (lane != 0) return;
  const double mean = tot / (double)HW;
  const double in_sum = s / mean, out_sum = outside / mean;
  // (imgattn*(2-black)*m/m.sum()).sum() - (imgattn*black*(1-m)/(1-m).sum()).sum()
  const double a = (double)(2.f - black) * in_sum / (double)c;
  const double bterm = (double)black * out_sum / (double)(HW - (long long)c);
  score[n] = (float)(a - bterm);
}

// ---- IoU ----
// |p & g| and |p | g| (a byte counts when it is not zero) over ONE BLOCK's share of two planes of n bytes, folded over each wave
// (valid in every lane): the blocks of the grid's x dimension stride over the planes, 16 bytes per thread and trip when both
// planes start on a 16-byte boundary (nonzero byte -> 0x01 per byte, popcount), byte by byte otherwise and for the last n % 16.
// THE count of hgl_iou, hgl_iou_select and the fused tail (integers: no order to keep).
__device__ __forceinline__ void iou_count_wave(const uint8_t* __restrict__ p, const uint8_t* __restrict__ g, long long n, unsigned& Iout,
                                               unsigned& Uout) {
  unsigned I = 0, U = 0;
  const bool al = ((((uintptr_t)p) | ((uintptr_t)g)) & 15) == 0;
  const long long n16 = al ? n / 16 : 0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) {
    const uint4 a = ((const uint4*)p)[i], b = ((const uint4*)g)[i];
    const unsigned aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      unsigned x = aw[w], y = bw[w];
      x |= x >> 4; x |= x >> 2; x |= x >> 1; x &= 0x01010101u;
      y |= y >> 4; y |= y >> 2; y |= y >> 1; y &= 0x01010101u;
      I += __popc(x & y);
      U += __popc(x | y);
    }
  }
  for (long long i = n16 * 16 + blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const bool a = p[i] != 0, b = g[i] != 0;
    I += (a && b);
    U += (a || b);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    I += __shfl_xor(I, o);
    U += __shfl_xor(U, o);
  }
  Iout = I;
  Uout = U;
}

__global__ __launch_bounds__(256) void iou_kernel(const uint8_t* __restrict__ p,
                                                  const uint8_t* __restrict__ g, long long n,
                                                  unsigned long long* __restrict__ out) {
  unsigned I, U;
  iou_count_wave(p, g, n, I, U);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&out[0], (unsigned long long)I);
    atomicAdd(&out[1], (unsigned long long)U);
  }
}

// same with pred = masks[idx[which]] resolved on the device
__global__ __launch_bounds__(256) void iou_select_kernel(const uint8_t* __restrict__ masks,
                                                         const int* __restrict__ idx, int which,
                                                         const uint8_t* __restrict__ g, long long n,
                                                         unsigned long long* __restrict__ out) {
  unsigned I, U;
  iou_count_wave(masks + (long long)idx[which] * n, g, n, I, U);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&out[0], (unsigned long long)I);
    atomicAdd(&out[1], (unsigned long long)U);
  }
}

// ---- per-sentence tail: single workgroup ----
constexpr int MAXK = 16;

__device__ float relation_boxes_dev(const long long* bi, const long long* bj, float si, float sj,
                                    int rela) {
  // utils.py:240-268 ; integer tensors /2 -> float32 true division
  switch (rela) {
    case 1: return si * sj * (float)(((float)bi[0] + (float)bi[2] / 2.f) < ((float)bj[0] + (float)bj[2] / 2.f));
    case 2: return si * sj * (float)(((float)bi[0] + (float)bi[2] / 2.f) > ((float)bj[0] + (float)bj[2] / 2.f));
    case 3: return si * sj * (float)(((float)bi[1] + (float)bi[3] / 2.f) < ((float)bj[1] + (float)bj[3] / 2.f));
    case 4: return si * sj * (float)(((float)bi[1] + (float)bi[3] / 2.f) > ((float)bj[1] + (float)bj[3] / 2.f));
    case 5: return si * sj * (float)((bi[2] * bi[3]) > (bj[2] * bj[3]));
    case 6: return si * sj * (float)((bi[2] * bi[3]) < (bj[2] * bj[3]));
    case 7: {
      const long long x1 = max(bi[0], bj[0]);
      const long long x2 = max(x1, min(bi[0] + bi[2], bj[0] + bj[2]));
      const long long y1 = max(bi[1], bj[1]);
      const long long y2 = max(y1, min(bi[1] + bi[3], bj[1] + bj[3]));
      return si * sj * (float)(x2 - x1) * (float)(y2 - y1) / (float)(bi[2] * bi[3]);
    }
    default: return si;
  }
}

// The body of a sentence comes in two parts, so that the sweep over (r, alpha, k1, k2) (grp_sweep_score_kernel) runs the very
// same code: score_lists_body -- everything that depends on r alone: text ensemble, logits, both soft-maxes, the pure arg-max
// (idx[0]) and the two top-k lists top1 / top2 (LDS, MAXK entries each) to k1 / k2 -- and score_blend_body, the single-thread
// end that depends on k1, k2 and alpha.  A list built by repeated arg-max for a smaller k is a prefix of the list for a larger
// one: a caller may build the lists once to the largest k and run score_blend_body per (k1, k2, alpha).
__device__ __forceinline__ void score_lists_body(
    const float* __restrict__ hybrid, const float* __restrict__ sent, const float* __restrict__ nphr,
    const float* __restrict__ others, int n_other, float r_mix, int N, int E,
    float logit_scale, int k1, int k2, int* __restrict__ idx,
    float* __restrict__ score_clip, float* __restrict__ score_neg, float* __restrict__ soft_scratch,
    int* __restrict__ top1, int* __restrict__ top2) {
  // soft_scratch: [2*N] softmax values + [2*E] text vectors (global scratch so N, E are unbounded)
  float* tpos = soft_scratch + 2 * N;
  float* tneg = tpos + E;
  // text_ensemble = r*sentence + (1-r)*noun_phrase ; neg = mean of "a photo of <other noun>"
  // features accumulated in order (Hybridgl_main.py:153,157-164); zeros when there is none
  for (int i = threadIdx.x; i < E; i += 256) {
    tpos[i] = r_mix * sent[i] + (1.f - r_mix) * nphr[i];
    float a = 0.f;
    for (int k = 0; k < n_other; ++k) a += others[(long long)k * E + i];
    tneg[i] = n_other > 0 ? a / (float)n_other : 0.f;
  }
  __syncthreads();
  __threadfence_block();
  __shared__ float red[8];
  __shared__ int redi[8];
  __shared__ float nrm[2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;

  // text norms
  for (int which = wave; which < 2; which += 4) {
    const float* tv = which == 0 ? tpos : tneg;
    float s = 0.f;
    for (int i = lane; i < E; i += 64) s += tv[i] * tv[i];
    s = wave_sum_f(s);
    if (lane == 0) nrm[which] = sqrtf(s);
  }
  __syncthreads();
  // logits: one wave per mask (strided).  A lane's elements of a feature row (and of the two text vectors) are fetched in
  // batches of eight and four masks are in flight per wave: `for (i = lane; i < E; i += 64) s += ir[i] * ir[i]` is one memory
  // round trip per trip, twice per mask, sixteen masks per wave -- most of this kernel's 80-130 us.  Same operations in the
  // same order per lane: identical logits.
  {
    constexpr int UE = 8, MQ = 4;
    for (int nb = wave; nb < N; nb += 4 * MQ) {
      float sq[MQ], d0[MQ], d1[MQ], ni[MQ];
#pragma unroll
      for (int j = 0; j < MQ; ++j) { sq[j] = 0.f; d0[j] = 0.f; d1[j] = 0.f; }
      for (int i0 = lane; i0 < E; i0 += 64 * UE) {
        float x[MQ][UE];
#pragma unroll
        for (int j = 0; j < MQ; ++j) {
          const float* ir = hybrid + (long long)min(nb + 4 * j, N - 1) * E;
#pragma unroll
          for (int u = 0; u < UE; ++u) x[j][u] = ir[min(i0 + 64 * u, E - 1)];
        }
#pragma unroll
        for (int j = 0; j < MQ; ++j)
#pragma unroll
          for (int u = 0; u < UE; ++u)
            if (i0 + 64 * u < E) sq[j] += x[j][u] * x[j][u];
      }
#pragma unroll
      for (int j = 0; j < MQ; ++j) ni[j] = sqrtf(wave_sum_f(sq[j]));
      for (int i0 = lane; i0 < E; i0 += 64 * UE) {
        float x[MQ][UE], tp[UE], tn[UE];
#pragma unroll
        for (int u = 0; u < UE; ++u) {
          tp[u] = tpos[min(i0 + 64 * u, E - 1)];
          tn[u] = tneg[min(i0 + 64 * u, E - 1)];
        }
#pragma unroll
        for (int j = 0; j < MQ; ++j) {
          const float* ir = hybrid + (long long)min(nb + 4 * j, N - 1) * E;
#pragma unroll
          for (int u = 0; u < UE; ++u) x[j][u] = ir[min(i0 + 64 * u, E - 1)];
        }
#pragma unroll
        for (int j = 0; j < MQ; ++j)
#pragma unroll
          for (int u = 0; u < UE; ++u)
            if (i0 + 64 * u < E) {
              const float v = logit_scale * (x[j][u] / ni[j]);
              d0[j] += v * (tp[u] / nrm[0]);
              d1[j] += v * (tn[u] / nrm[1]);
            }
      }
#pragma unroll
      for (int j = 0; j < MQ; ++j) {
        const float r0 = wave_sum_f(d0[j]), r1 = wave_sum_f(d1[j]);
        if (lane == 0 && nb + 4 * j < N) {
          score_clip[nb + 4 * j] = r0;
          score_neg[nb + 4 * j] = r1;
        }
      }
    }
  }
  __syncthreads();
  __threadfence_block();

  // softmax over masks of both logit vectors + argmax of score_clip.  torch.argmax's order: a NaN is larger than every
  // number, the first of equal maxima (or NaNs) wins; a NaN maximum then makes the whole soft-max NaN, as torch's does.
  auto better = [](float v, int n, float mx, int mi) {
    const bool vn = v != v, mn = mx != mx;
    if (vn != mn) return vn;
    if (vn) return n < mi;
    return v > mx || (v == mx && n < mi);
  };
  for (int which = 0; which < 2; ++which) {
    const float* lg = which == 0 ? score_clip : score_neg;
    float mx = -INFINITY;
    int mi = 0x7fffffff;
    for (int n = t; n < N; n += 256) {
      const float v = lg[n];
      if (better(v, n, mx, mi)) { mx = v; mi = n; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(mx, o);
      const int oi = __shfl_xor(mi, o);
      if (better(ov, oi, mx, mi)) { mx = ov; mi = oi; }
    }
    if (lane == 0) { red[wave] = mx; redi[wave] = mi; }
    __syncthreads();
    float gmx = red[0];
    int gmi = redi[0];
    for (int w = 1; w < 4; ++w)
      if (better(red[w], redi[w], gmx, gmi)) { gmx = red[w]; gmi = redi[w]; }
    __syncthreads();
    if (which == 0 && t == 0) idx[0] = gmi == 0x7fffffff ? 0 : gmi;   // all-NaN logits (a NaN text feature): a valid index, NaN scores
    float se = 0.f;
    for (int n = t; n < N; n += 256) se += expf(lg[n] - gmx);
    se = wave_sum_f(se);
    if (lane == 0) red[wave] = se;
    __syncthreads();
    const float denom = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    for (int n = t; n < N; n += 256) soft_scratch[which * N + n] = expf(lg[n] - gmx) / denom;
  }
  __syncthreads();
  __threadfence_block();

  // top-k (descending, lowest index on ties) by repeated argmax -- wave 0 for list 1, wave 1 for list 2
  if (wave < 2) {
    const float* sv = soft_scratch + wave * N;
    int* top = wave == 0 ? top1 : top2;
    const int kk = wave == 0 ? k1 : k2;
    for (int j = 0; j < kk; ++j) {
      float mx = -INFINITY;
      int mi = 0x7fffffff;
      for (int n = lane; n < N; n += 64) {
        bool used = false;
        for (int u = 0; u < j; ++u) used |= top[u] == n;
        const float v = sv[n];
        if (!used && (v > mx || (v == mx && n < mi))) { mx = v; mi = n; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(mx, o);
        const int oi = __shfl_xor(mi, o);
        if (ov > mx || (ov == mx && oi < mi)) { mx = ov; mi = oi; }
      }
      if (mi == 0x7fffffff) mi = j < N ? j : 0;  // all-NaN scores (no other nouns): any valid index
      if (lane == 0) top[j] = mi;
      __builtin_amdgcn_wave_barrier();
      __threadfence_block();
    }
  }
  __syncthreads();
}

// one THREAD: Hybridgl_main.py:183-196 relation sums over the first k1 / k2 entries of the lists, softmax, blend with the
// coherence score, argmax -> the final index
__device__ __forceinline__ int score_blend_body(const long long* __restrict__ boxes, const float* __restrict__ gem, int N, int k1, int k2,
                                                float alpha, int rela, int has_other, const float* __restrict__ soft_scratch,
                                                const int* __restrict__ top1, const int* __restrict__ top2) {
  {
    const float* sc = soft_scratch;
    const float* sn = soft_scratch + N;
    // partial sums are fp32 in the reference (np.float64 + Tensor -> Tensor.__radd__ -> fp32)
    float ts[MAXK];
    for (int i = 0; i < k1; ++i) {
      float acc = 0.f;
      const int ii = top1[i];
      if (!has_other) {
        for (int j = 0; j < k1; ++j) {
          const int jj = top1[j];
          acc += relation_boxes_dev(boxes + 4 * ii, boxes + 4 * jj, sc[ii], sc[jj], rela);
        }
      } else {
        for (int j = 0; j < k2; ++j) {
          const int jj = top2[j];
          acc += relation_boxes_dev(boxes + 4 * ii, boxes + 4 * jj, sc[ii], sn[jj], rela);
        }
      }
      ts[i] = acc;
    }
    float tf[MAXK];
    float mx = -INFINITY;
    for (int i = 0; i < k1; ++i) { tf[i] = ts[i]; mx = fmaxf(mx, tf[i]); }
    float den = 0.f;
    for (int i = 0; i < k1; ++i) { tf[i] = expf(tf[i] - mx); den += tf[i]; }
    // torch.argmax's order: a NaN is larger than every number and the FIRST of equal maxima (or NaNs) wins -- a NaN coherence
    // score (an empty or full proposal mask, a constant heat-map: 0/0 in Hybridgl_main.py:203-223) among the top-k decides
    // the reference's answer (tests/golden/scoring_nan.npz)
    int best = 0;
    float bv = 0.f;
    for (int i = 0; i < k1; ++i) {
      const float v = (tf[i] / den) * (1.f - alpha) + alpha * gem[top1[i]];
      if (i == 0 || v > bv || (v != v && bv == bv)) { bv = v; best = i; }
    }
    return top1[best];
  }
}

__device__ __forceinline__ void score_sentence_body(
    const float* __restrict__ hybrid, const float* __restrict__ sent, const float* __restrict__ nphr,
    const float* __restrict__ others, int n_other, float r_mix,
    const long long* __restrict__ boxes, const float* __restrict__ gem, int N, int E,
    float logit_scale, int k1, int k2, float alpha, int rela, int has_other, int* __restrict__ idx,
    float* __restrict__ score_clip, float* __restrict__ score_neg, float* __restrict__ soft_scratch) {
  __shared__ int top1[MAXK], top2[MAXK];
  score_lists_body(hybrid, sent, nphr, others, n_other, r_mix, N, E, logit_scale, k1, k2, idx, score_clip, score_neg, soft_scratch,
                   top1, top2);
  if (threadIdx.x == 0) idx[1] = score_blend_body(boxes, gem, N, k1, k2, alpha, rela, has_other, soft_scratch, top1, top2);
}

__global__ __launch_bounds__(256) void score_sentence_kernel(
    const float* __restrict__ hybrid, const float* __restrict__ sent, const float* __restrict__ nphr,
    const float* __restrict__ others, int n_other, float r_mix,
    const long long* __restrict__ boxes, const float* __restrict__ gem, int N, int E,
    float logit_scale, int k1, int k2, float alpha, int rela, int has_other, int* __restrict__ idx,
    float* __restrict__ score_clip, float* __restrict__ score_neg, float* __restrict__ soft_scratch) {
  score_sentence_body(hybrid, sent, nphr, others, n_other, r_mix, boxes, gem, N, E, logit_scale, k1, k2, alpha, rela, has_other,
                      idx, score_clip, score_neg, soft_scratch);
}

// ---- the tail of whole REFS (all their sentences) in four launches: Hybridgl_main.py:153-230 ------------------------------
// (the device bodies; the kernels that run them over a table of refs follow, the host path is tail_launch below)
// The per-sentence launches above re-read the N mask planes for every sentence (83.6 MB per ref at N = 64, 640 x 640, three
// sentences) and cost ~15 launches per sentence with torch glue between them.  Here the pooling of ALL sentences' heat-maps is
// one launch (the mask planes come from HBM once: the other maps' workgroups find them in L2 / the Infinity Cache), the
// scoring of the sentences runs as one workgroup each in one launch, the IoU of
// both winners of every sentence in one launch, and the four accumulators of Hybridgl_main.py:52-55 are updated by the
// last block of that launch.  Arithmetic and reduction orders are those of the per-sentence kernels (bit-identical results).
constexpr int REF_MAXS = 16;       // sentences per row of a launch (a ref with more takes several rows: tail_push_rows)
constexpr int REF_MM_BLOCKS = 64;  // min / max partials per heat-map

struct RefSentences {
  const float* attn[REF_MAXS];
  const uint8_t* target[REF_MAXS];
  int sent_row[REF_MAXS], nphr_row[REF_MAXS], other_row0[REF_MAXS], n_other[REF_MAXS];
  int dirflag[REF_MAXS], rela[REF_MAXS], has_other[REF_MAXS];
  float black[REF_MAXS];
};

__device__ __forceinline__ void ref_minmax_body(const float* __restrict__ a, int s, long long n, float* __restrict__ part_mm) {
  float mn = INFINITY, mx = -INFINITY;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = a[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o));
    mx = fmaxf(mx, __shfl_xor(mx, o));
  }
  __shared__ float smn[4], smx[4];
  if ((threadIdx.x & 63) == 0) {
    smn[threadIdx.x >> 6] = mn;
    smx[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* p = part_mm + ((long long)s * REF_MM_BLOCKS + blockIdx.x) * 2;
    p[0] = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
    p[1] = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  }
}
// min / max are exact in any order: every wave folds the 64 partial pairs of a map itself (one pair per lane)
__device__ __forceinline__ void ref_fold_minmax(const float* __restrict__ part_mm, int s, int lane, float& mn, float& mx) {
  const float* p = part_mm + ((long long)s * REF_MM_BLOCKS + lane) * 2;
  mn = p[0];
  mx = p[1];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o));
    mx = fmaxf(mx, __shfl_xor(mx, o));
  }
}

// masked_pool_kernel for the S heat-maps of a ref in ONE launch: grid (pixel blocks, mask groups); the maps are looped INSIDE
// the workgroup (pool_block, four at a time).  History: a first version (round 3) kept four maps' tiles in registers with a
// double-precision sum per pixel and map -- 260 VGPRs, 8.5 k instructions, slower than three launches; rounds 4-5 made every
// (block, group, map) its own small workgroup and re-read the mask bytes per map from L2; the fp32 fma form of pool_block needs
// 16 VGPRs per map and fetches every mask byte once.  Partials in the layout of masked_pool_kernel.
// the S heat-maps of a ref over one FULL pixel block and one group of MG masks: the maps go through pool_block four at a time
// (the mask bytes of the block are fetched once per four maps: once for the three sentences of a RefCOCO ref)
// CH = maps per pass: 4, or 3 for the launches whose refs have at most three sentences (RefCOCO: 16 VGPRs fewer per map held
// -> 4 instead of 3 waves per SIMD)
template <int MG, int CH>
__device__ __forceinline__ void ref_masked_pool_body(int blk, const float* const* __restrict__ attn, const int* __restrict__ dirflag, int S, int mask_group,
                                                     const uint8_t* __restrict__ masks, int N, int H, int W,
                                                     const float* __restrict__ part_mm, double* __restrict__ part_sum,
                                                     unsigned* __restrict__ part_cnt, double* __restrict__ part_tot, int nparts) {
  const int lane = threadIdx.x & 63;
  const int n0 = mask_group * MG, n1 = min(N, n0 + MG);
  const bool wt = mask_group == 0;
  for (int s0 = 0; s0 < S; s0 += CH) {
    const int ns = min(CH, S - s0);
    PoolMap pm[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int sj = min(s0 + j, S - 1);
      float mn, mx;
      ref_fold_minmax(part_mm, sj, lane, mn, mx);
      pm[j].attn = attn[sj]; pm[j].dirflag = dirflag[sj]; pm[j].sidx = sj; pm[j].mn = mn; pm[j].range = mx - mn;
    }
    if (CH == 4 && ns == 4) {
      if constexpr (CH == 4) pool_block<4, true>(blk, pm, n0, n1, masks, N, H, W, wt, part_sum, part_cnt, part_tot, nparts);
    } else if (ns == 3) {
      const PoolMap p3[3] = {pm[0], pm[1], pm[2]};
      pool_block<3, true>(blk, p3, n0, n1, masks, N, H, W, wt, part_sum, part_cnt, part_tot, nparts);
    } else if (ns == 2) {
      const PoolMap p2[2] = {pm[0], pm[1]};
      pool_block<2, true>(blk, p2, n0, n1, masks, N, H, W, wt, part_sum, part_cnt, part_tot, nparts);
    } else {
      const PoolMap p1[1] = {pm[0]};
      pool_block<1, true>(blk, p1, n0, n1, masks, N, H, W, wt, part_sum, part_cnt, part_tot, nparts);
    }
  }
}
// ... and over the partial LAST block of the plane, one map at a time
template <int MG>
__device__ __forceinline__ void ref_masked_pool_last(int blk, const float* const* __restrict__ attn, const int* __restrict__ dirflag, int S, int mask_group,
                                                     const uint8_t* __restrict__ masks, int N, int H, int W,
                                                     const float* __restrict__ part_mm, double* __restrict__ part_sum,
                                                     unsigned* __restrict__ part_cnt, double* __restrict__ part_tot, int nparts) {
  const int lane = threadIdx.x & 63;
  const int n0 = mask_group * MG, n1 = min(N, n0 + MG);
  for (int sj = 0; sj < S; ++sj) {
    float mn, mx;
    ref_fold_minmax(part_mm, sj, lane, mn, mx);
    const PoolMap pm[1] = {{attn[sj], dirflag[sj], sj, mn, mx - mn}};
    pool_block<1, false>(blk, pm, n0, n1, masks, N, H, W, mask_group == 0, part_sum, part_cnt, part_tot, nparts);
  }
}

// the coherence scores gem [N] of sentence s of a row from the pooling partials (one workgroup; shared by ref_score_body and the
// sweep's scoring kernel: the same sums in the same order)
// attn / dirflag: the sentence's heat-map and direction; masks, part_mm: the row's -- read only for a mask that takes
// pool_outside_sum
__device__ __forceinline__ void ref_coherence_body(float black, int s, int N, int H, int W, const double* __restrict__ part_sum,
                                                   const unsigned* __restrict__ part_cnt, const double* __restrict__ part_tot, int nparts,
                                                   float* __restrict__ gem, const float* __restrict__ attn, int dirflag,
                                                   const uint8_t* __restrict__ masks, const float* __restrict__ part_mm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long HW = (long long)H * W;
  // coherence_final_kernel's reduction for this sentence's N masks.  One wave per mask, lanes stride over the per-wave
  // partials -- but a plain `for (b = lane; b < nparts; b += 64)` is one memory round trip per trip, and sixteen masks per
  // wave one after the other made this workgroup the longest kernel of the tail (130 us).  The total is summed ONCE per wave
  // (it is the same for every mask), and four masks' partials are fetched in batches of up to eight trips before they are
  // added -- in the same order as before: identical sums.
  constexpr int MR = 4, UB = 8;
  double tot = 0.0;
  for (int b0 = lane; b0 < nparts; b0 += 64 * UB) {
    double tv[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) tv[u] = part_tot[(long long)s * nparts + min(b0 + 64 * u, nparts - 1)];
#pragma unroll
    for (int u = 0; u < UB; ++u)
      if (b0 + 64 * u < nparts) tot += tv[u];
  }
  tot = wave_sum_d(tot);
  for (int nb = wave * MR; nb < N; nb += 4 * MR) {
    double sm[MR];
    unsigned long long c[MR];
#pragma unroll
    for (int i = 0; i < MR; ++i) { sm[i] = 0.0; c[i] = 0; }
    for (int b0 = lane; b0 < nparts; b0 += 64 * UB) {
      double sv[MR][UB];
      unsigned cv[MR][UB];
#pragma unroll
      for (int i = 0; i < MR; ++i) {
        const int n = min(nb + i, N - 1);
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const long long b = min(b0 + 64 * u, nparts - 1);
          sv[i][u] = part_sum[((long long)s * nparts + b) * N + n];
          cv[i][u] = part_cnt[b * N + n];
        }
      }
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int u = 0; u < UB; ++u)
          if (b0 + 64 * u < nparts) { sm[i] += sv[i][u]; c[i] += cv[i][u]; }
    }
#pragma unroll
    for (int i = 0; i < MR; ++i) {
      double smr = wave_sum_d(sm[i]);
      unsigned long long cr = c[i];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cr += __shfl_xor(cr, o);
      double outside = tot - smr;
      if (nb + i < N && pool_outside_direct(cr, HW)) {      // wave-uniform, as in coherence_final_kernel
        float mn, mx;
        ref_fold_minmax(part_mm, s, lane, mn, mx);
        outside = pool_outside_sum(attn, masks + (long long)(nb + i) * HW, HW, W, dirflag, mn, mx - mn);
      }
      if (lane == 0 && nb + i < N) {
        const double mean = tot / (double)HW;
        const double in_sum = smr / mean, out_sum = outside / mean;
        const double a = (double)(2.f - black) * in_sum / (double)cr;
        const double bterm = (double)black * out_sum / (double)(HW - (long long)cr);
        gem[nb + i] = (float)(a - bterm);
      }
    }
  }
}

// one workgroup per sentence: coherence_final_kernel's reduction for its N masks, then the sentence's scoring
__device__ __forceinline__ void ref_score_body(const RefSentences& rs, int s, bool first, const float* __restrict__ hybrid,
                                               const float* __restrict__ text, const long long* __restrict__ boxes, int N, int E, int H,
                                               int W, float logit_scale, float r_mix, int k1, int k2, float alpha,
                                               const double* __restrict__ part_sum, const unsigned* __restrict__ part_cnt,
                                               const double* __restrict__ part_tot, int nparts, const uint8_t* __restrict__ masks,
                                               const float* __restrict__ part_mm, float* __restrict__ gem_all,
                                               float* __restrict__ clip_all, float* __restrict__ neg_all, float* __restrict__ soft_all,
                                               int* __restrict__ idx_all, unsigned long long* __restrict__ iu_all,
                                               unsigned* __restrict__ done) {
  float* gem = gem_all + (long long)s * N;
  ref_coherence_body(rs.black[s], s, N, H, W, part_sum, part_cnt, part_tot, nparts, gem, rs.attn[s], rs.dirflag[s], masks, part_mm);
  if (threadIdx.x < 4) iu_all[4 * s + threadIdx.x] = 0ull;
  if (first && threadIdx.x == 0) *done = 0u;
  __syncthreads();
  __threadfence_block();
  score_sentence_body(hybrid, text + (long long)rs.sent_row[s] * E, text + (long long)rs.nphr_row[s] * E,
                      text + (long long)rs.other_row0[s] * E, rs.n_other[s], r_mix, boxes, gem, N, E, logit_scale, k1, k2, alpha,
                      rs.rela[s], rs.has_other[s], idx_all + 2 * s, clip_all + (long long)s * N, neg_all + (long long)s * N,
                      soft_all + (long long)s * (2 * N + 2 * E));
}

// Compute_IoU of both winners of every sentence: I / U of one block's share of a (mask, target) pair, reduced over the block
__device__ __forceinline__ void ref_iou_block(const uint8_t* __restrict__ p, const uint8_t* __restrict__ g, long long n, unsigned& Iout,
                                              unsigned& Uout) {
  unsigned I, U;
  iou_count_wave(p, g, n, I, U);
  __shared__ unsigned sI[4], sU[4];
  if ((threadIdx.x & 63) == 0) {
    sI[threadIdx.x >> 6] = I;
    sU[threadIdx.x >> 6] = U;
  }
  __syncthreads();
  Iout = (sI[0] + sI[1]) + (sI[2] + sI[3]);
  Uout = (sU[0] + sU[1]) + (sU[2] + sU[3]);
}

// ---- the kernels of the fused tail: the bodies above over a TABLE of rows (hgl_score_ref: the rows of one ref; hgl_score_group:
// of a group of refs) ---------------------------------------------------------------------------------------------------------
// Four launches per ref of ~31 MB each are latency-bound by construction (pooling 33 us per ref = 0.9 TB/s on its algorithmic
// bytes).  The grouped loop scores the refs of a group (16 images) back to back, so the kernels run over ALL of them at once: a
// table of per-row descriptors in device memory (shapes differ from ref to ref), grids sized by the largest row with the
// others' surplus blocks leaving at once, ~0.5 GB per pooling launch.  A block executes the bodies on its row's operands: the
// rows of a ref do not depend on what else the table holds.
constexpr int GRP_MAXR = 16;       // rows per launch (the host loops over chunks)
struct GroupRefDev {
  RefSentences rs;
  int S, N, H, W, k1, k2, nparts, nblk;
  const float *hybrid, *text;
  const long long* boxes;
  const uint8_t* masks;
  float* part_mm;
  double* part_sum;
  unsigned* part_cnt;
  double* part_tot;
  float *gem, *clip, *neg, *soft;
  int* idx;
  unsigned long long* iu;
};

__global__ __launch_bounds__(256) void grp_minmax_kernel(const GroupRefDev* __restrict__ tab) {
  const GroupRefDev& g = tab[blockIdx.z];
  const int s = blockIdx.y;
  if (s >= g.S) return;
  ref_minmax_body(g.rs.attn[s], s, (long long)g.H * g.W, g.part_mm);
}

// MG: masks per pooling workgroup (MASK_GROUP for hgl_score_ref, REF_MASK_GROUP for hgl_score_group: see above)
template <int MG, int CH>
__global__ __launch_bounds__(256) void grp_masked_pool_kernel(const GroupRefDev* __restrict__ tab) {
  const GroupRefDev& g = tab[blockIdx.z];
  const int nfull = (int)(((long long)g.H * g.W) / PIX_PER_BLOCK);
  if ((int)blockIdx.x >= nfull || (int)blockIdx.y * MG >= g.N) return;
  ref_masked_pool_body<MG, CH>(blockIdx.x, g.rs.attn, g.rs.dirflag, g.S, blockIdx.y, g.masks, g.N, g.H, g.W, g.part_mm, g.part_sum,
                               g.part_cnt, g.part_tot, g.nparts);
}
template <int MG>
__global__ __launch_bounds__(256) void grp_masked_pool_last_kernel(const GroupRefDev* __restrict__ tab) {
  const GroupRefDev& g = tab[blockIdx.z];
  const long long HW = (long long)g.H * g.W;
  if (HW % PIX_PER_BLOCK == 0 || (int)blockIdx.y * MG >= g.N) return;
  ref_masked_pool_last<MG>((int)(HW / PIX_PER_BLOCK), g.rs.attn, g.rs.dirflag, g.S, blockIdx.y, g.masks, g.N, g.H, g.W, g.part_mm,
                           g.part_sum, g.part_cnt, g.part_tot, g.nparts);
}

__global__ __launch_bounds__(256) void grp_score_kernel(const GroupRefDev* __restrict__ tab, int E, float logit_scale, float r_mix,
                                                        float alpha, unsigned* __restrict__ done) {
  const GroupRefDev& g = tab[blockIdx.y];
  const int s = blockIdx.x;
  if (s >= g.S) return;
  ref_score_body(g.rs, s, blockIdx.x == 0 && blockIdx.y == 0, g.hybrid, g.text, g.boxes, g.N, E, g.H, g.W, logit_scale, r_mix, g.k1, g.k2,
                 alpha, g.part_sum, g.part_cnt, g.part_tot, g.nparts, g.masks, g.part_mm, g.gem, g.clip, g.neg, g.soft, g.idx, g.iu, done);
}

// grid (blocks, 2 maxS, R): every block counts on `done` (those beyond their row's sentences do nothing else); the last one adds
// all sentences' sums of all rows to the running accumulators cum_I, cum_U, cum_I_final, cum_U_final (integers: order-free)
__global__ __launch_bounds__(256) void grp_iou_kernel(const GroupRefDev* __restrict__ tab, int R, unsigned long long* __restrict__ cum,
                                                      unsigned* __restrict__ done) {
  const GroupRefDev& g = tab[blockIdx.z];
  const int s = blockIdx.y >> 1, which = blockIdx.y & 1;
  unsigned I = 0, U = 0;
  const bool live = s < g.S;
  if (live) ref_iou_block(g.masks + (long long)g.idx[2 * s + which] * g.H * g.W, g.rs.target[s], (long long)g.H * g.W, I, U);
  __shared__ int last;
  if (threadIdx.x == 0) {
    if (live) {
      atomicAdd(&g.iu[4 * s + 2 * which], (unsigned long long)I);
      atomicAdd(&g.iu[4 * s + 2 * which + 1], (unsigned long long)U);
    }
    __threadfence();
    last = atomicAdd(done, 1u) == gridDim.x * gridDim.y * gridDim.z - 1;
  }
  __syncthreads();
  // the last block folds every (ref, sentence) counter into the four accumulators: one counter per THREAD, read with an
  // atomic (the other blocks' adds are device-scope atomics), summed through LDS -- integers: any order.  (Four threads walking
  // the R x S counters one after the other were 48 dependent atomic round trips: 80 of this launch's 102 us.)
  __shared__ unsigned long long acc[4];
  if (last && cum != nullptr) {
    if (threadIdx.x < 4) acc[threadIdx.x] = 0ull;
    __syncthreads();
    const int maxS = (int)gridDim.y >> 1;
    for (int e = threadIdx.x; e < R * maxS * 4; e += 256) {
      const int r = e / (maxS * 4), j = (e >> 2) % maxS, k = e & 3;
      if (j < tab[r].S) atomicAdd(&acc[k], atomicAdd(&tab[r].iu[4 * j + k], 0ull));
    }
    __syncthreads();
    if (threadIdx.x < 4) cum[threadIdx.x] += acc[threadIdx.x];
  }
}

// ---- the sweep: the tail of the same rows under C configurations (r, alpha, k1, k2) at once: hgl_score_group_sweep -----------
// Min / max and pooling do not depend on the configuration: they run once, through the launches above.  What replaces
// grp_score_kernel + grp_iou_kernel:
//   grp_iou_table_kernel     |mask_n & target_t| of EVERY proposal with every distinct target of the row, the areas of the
//                            proposals and of the targets, in one pass over the mask planes: a configuration's (I, U) is then a
//                            look-up (grp_iou_kernel reads a plane per (sentence, winner): C x S x 2 planes per ref for C
//                            configurations), and the best proposal of a sentence -- the ceiling -- comes with it;
//   grp_sweep_score_kernel   one workgroup per (sentence, distinct r): score_lists_body once, to the largest k1 / k2 any
//                            configuration of that r asks for, then one thread per configuration runs score_blend_body over its
//                            own prefixes of the lists.
constexpr int SWP_MAXC = 256;      // configurations per call: one thread of a scoring workgroup each
constexpr int SWP_MAXR = 32;       // distinct r among them: workgroups per sentence
constexpr int TAB_MG = 32;         // masks per workgroup of the table kernel
struct SweepRowDev {
  unsigned char k[SWP_MAXC][2];         // this ref's k1, k2 per configuration, clamped to N
  unsigned char kmax[SWP_MAXR][2];      // the largest of them per distinct r
  int tslot[REF_MAXS];                  // sentence -> index of its target among the row's distinct target pointers
  const uint8_t* tptr[REF_MAXS];        // the distinct targets
  int nt, cstride;                      // their number; sentences of the WHOLE ref (the stride of a configuration in idx / iu)
  int* idx;                             // [C, cstride, 2], at the row's first sentence
  unsigned long long* iu;               // [C, cstride, 4], likewise
  long long* ceiling;                   // [S,3] of the row
  // table (zeroed before the launch): I [nt][N], then area [N] (slot nt), and at (REF_MAXS + 1) * N the areas of the targets
  unsigned long long* tab;
  float* scratch;                       // per (sentence, r): gem, clip, neg [N] each and score_lists_body's 2 N + 2 E
};
struct SweepTab {
  SweepRowDev row[GRP_MAXR];
  float r[SWP_MAXR], alpha[SWP_MAXC];
  unsigned char rgrp[SWP_MAXC];         // configuration -> index of its r
  int C, nr;
};

// sixteen bytes of a plane at pixel p0 -> sixteen bits (byte != 0, as iou_count_wave counts); pixels beyond the plane are 0.
// full (wave-uniform): all sixteen lie inside -- one 16-byte load at any alignment, as pool_block's
__device__ __forceinline__ unsigned tab_bits(const uint8_t* __restrict__ plane, long long p0, long long HW, bool full) {
  unsigned w4[4] = {0u, 0u, 0u, 0u};
  if (full) {
    const pool_u32x4 mv = *(const pool_u32x4_u*)(plane + p0);
    w4[0] = mv.x; w4[1] = mv.y; w4[2] = mv.z; w4[3] = mv.w;
  } else {
#pragma unroll
    for (int e = 0; e < PX_LANE; ++e) {
      const unsigned byte = p0 + e < HW ? (unsigned)plane[min(p0 + e, HW - 1)] : 0u;
      w4[e >> 2] |= byte << (8 * (e & 3));
    }
  }
  unsigned bits = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned w = w4[q];
    const unsigned nz = ((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) >> 7) & 0x01010101u;      // as pool_block
    bits |= (((nz * 0x01020408u) >> 24) & 0xfu) << (4 * q);      // bits 0, 8, 16, 24 gathered into 24..27 (no two terms meet)
  }
  return bits;
}

// grid (pixel blocks, groups of TAB_MG masks, rows).  A workgroup holds PIX_PER_BLOCK pixels of its masks as bits (one VGPR
// per mask and lane), walks the row's distinct targets (and, as one more, the plane of all ones: the masks' areas) and adds its
// counts to the row's table: every mask byte is fetched once, whatever the number of sentences.  Integers: any order.
__global__ __launch_bounds__(256) void grp_iou_table_kernel(const GroupRefDev* __restrict__ tab, const SweepTab* __restrict__ swp) {
  const GroupRefDev& g = tab[blockIdx.z];
  const SweepRowDev& q = swp->row[blockIdx.z];
  const long long HW = (long long)g.H * g.W;
  const long long b0 = (long long)blockIdx.x * PIX_PER_BLOCK;
  const int n0 = blockIdx.y * TAB_MG, N = g.N;
  if (b0 >= HW || n0 >= N) return;      // (uniform; before any barrier)
  const int n1 = min(N, n0 + TAB_MG);
  const long long p0 = b0 + threadIdx.x * PX_LANE;
  const bool full = b0 + PIX_PER_BLOCK <= HW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned mb[TAB_MG];
#pragma unroll
  for (int j = 0; j < TAB_MG; ++j) {
    const unsigned b = tab_bits(g.masks + (long long)min(n0 + j, n1 - 1) * HW, p0, HW, full);
    mb[j] = n0 + j < n1 ? b : 0u;
  }
  __shared__ unsigned sm[4][TAB_MG + 1];
  const int nt = q.nt;
  for (int t = 0; t <= nt; ++t) {
    const unsigned tb = t < nt ? tab_bits(q.tptr[t], p0, HW, full) : 0xffffu;
    unsigned c[TAB_MG];
#pragma unroll
    for (int j = 0; j < TAB_MG; ++j) c[j] = (unsigned)__popc(mb[j] & tb);
#pragma unroll
    for (int j = 0; j < TAB_MG; ++j) c[j] = pool_sum_u(c[j]);
    const unsigned ta = pool_sum_u((unsigned)__popc(tb));
    if (lane == 63) {
#pragma unroll
      for (int j = 0; j < TAB_MG; ++j) sm[wave][j] = c[j];
      sm[wave][TAB_MG] = ta;
    }
    __syncthreads();
    const int x = threadIdx.x;
    if (x <= TAB_MG) {
      const unsigned v = (sm[0][x] + sm[1][x]) + (sm[2][x] + sm[3][x]);
      if (x < TAB_MG) {
        if (n0 + x < n1 && v != 0u) atomicAdd(&q.tab[(long long)t * N + n0 + x], (unsigned long long)v);
      } else if (t < nt && blockIdx.y == 0 && v != 0u) {
        atomicAdd(&q.tab[(REF_MAXS + 1ll) * N + t], (unsigned long long)v);
      }
    }
    __syncthreads();
  }
}

// the order of the ceiling: a's I / U above b's, compared exactly as I_a U_b > I_b U_a; the lower index wins a tie (U = 0 has
// been replaced by 1 by the caller: I is 0 then and the pair ranks as ratio 0)
__device__ __forceinline__ bool ceil_better(unsigned long long Ia, unsigned long long Ua, int na, unsigned long long Ib,
                                            unsigned long long Ub, int nb) {
  const unsigned long long l = Ia * Ub, r = Ib * Ua;
  return l > r || (l == r && na < nb);
}

// grid (maxS, distinct r, rows), after grp_iou_table_kernel on the stream.  Every block counts on `done` (zeroed before the
// launch); the last one adds the column sums of all rows' iu [C, S, 4] to cum [C, 4] and the ceilings' (I, U) to cum_ceiling.
__global__ __launch_bounds__(256) void grp_sweep_score_kernel(const GroupRefDev* __restrict__ tab, const SweepTab* __restrict__ swp, int R,
                                                              int E, float logit_scale, unsigned long long* __restrict__ cum,
                                                              unsigned long long* __restrict__ cum_ceiling,
                                                              unsigned* __restrict__ done) {
  const GroupRefDev& g = tab[blockIdx.z];
  const SweepRowDev& q = swp->row[blockIdx.z];
  const int s = blockIdx.x, rg = blockIdx.y, t = threadIdx.x, C = swp->C;
  __shared__ int top1[MAXK], top2[MAXK];
  __shared__ int pure;
  __shared__ unsigned long long cI[4], cU[4];
  __shared__ int cn[4];
  if (s < g.S) {
    const int N = g.N;
    float* gem = q.scratch + ((long long)s * gridDim.y + rg) * (5ll * N + 2ll * E);
    float* clip = gem + N;
    float* neg = clip + N;
    float* soft = neg + N;
    ref_coherence_body(g.rs.black[s], s, N, g.H, g.W, g.part_sum, g.part_cnt, g.part_tot, g.nparts, gem, g.rs.attn[s], g.rs.dirflag[s],
                       g.masks, g.part_mm);
    __syncthreads();
    __threadfence_block();
    score_lists_body(g.hybrid, g.text + (long long)g.rs.sent_row[s] * E, g.text + (long long)g.rs.nphr_row[s] * E,
                     g.text + (long long)g.rs.other_row0[s] * E, g.rs.n_other[s], swp->r[rg], N, E, logit_scale, q.kmax[rg][0],
                     q.kmax[rg][1], &pure, clip, neg, soft, top1, top2);
    const unsigned long long* Itab = q.tab + (long long)q.tslot[s] * N;
    const unsigned long long* area = q.tab + (long long)q.nt * N;
    const unsigned long long tarea = q.tab[(REF_MAXS + 1ll) * N + q.tslot[s]];
    if (t < C && swp->rgrp[t] == rg) {      // one thread per configuration of this r
      const int fin = score_blend_body(g.boxes, gem, N, q.k[t][0], q.k[t][1], swp->alpha[t], g.rs.rela[s], g.rs.has_other[s], soft,
                                       top1, top2);
      const int pu = pure;
      int* io = q.idx + ((long long)t * q.cstride + s) * 2;
      io[0] = pu;
      io[1] = fin;
      unsigned long long* uo = q.iu + ((long long)t * q.cstride + s) * 4;
      const unsigned long long Ip = Itab[pu], If = Itab[fin];
      uo[0] = Ip;
      uo[1] = area[pu] + tarea - Ip;
      uo[2] = If;
      uo[3] = area[fin] + tarea - If;
    }
    if (rg == 0) {      // the ceiling of the sentence: the proposal of the largest I / U
      unsigned long long bI = 0ull, bU = 1ull;
      int bn = 0x7fffffff;
      for (int n = t; n < N; n += 256) {
        const unsigned long long I = Itab[n], U = area[n] + tarea - I, Uc = U != 0ull ? U : 1ull;
        if (ceil_better(I, Uc, n, bI, bU, bn)) { bI = I; bU = Uc; bn = n; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long oI = __shfl_xor(bI, o), oU = __shfl_xor(bU, o);
        const int on = __shfl_xor(bn, o);
        if (ceil_better(oI, oU, on, bI, bU, bn)) { bI = oI; bU = oU; bn = on; }
      }
      if ((t & 63) == 0) { cI[t >> 6] = bI; cU[t >> 6] = bU; cn[t >> 6] = bn; }
      __syncthreads();
      if (t == 0) {
        for (int w = 1; w < 4; ++w)
          if (ceil_better(cI[w], cU[w], cn[w], bI, bU, bn)) { bI = cI[w]; bU = cU[w]; bn = cn[w]; }
        q.ceiling[3 * s + 0] = bn;
        q.ceiling[3 * s + 1] = (long long)bI;
        q.ceiling[3 * s + 2] = (long long)(area[bn] + tarea - bI);
      }
    }
  }
  __shared__ int last;
  __threadfence();
  __syncthreads();
  if (t == 0) last = atomicAdd(done, 1u) == gridDim.x * gridDim.y * gridDim.z - 1;
  __syncthreads();
  if (!last) return;
  // the last block: every other block's stores came before its count on `done` (fence, then the atomic); read them behind a
  // fence of our own, with device-scope loads.  One thread per configuration walks the (row, sentence) entries: independent loads
  __threadfence();
  if (cum != nullptr && t < C) {
    unsigned long long a[4] = {0ull, 0ull, 0ull, 0ull};
    for (int r = 0; r < R; ++r) {
      const SweepRowDev& w = swp->row[r];
      const int S = tab[r].S;
      for (int j = 0; j < S; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k)
          a[k] += __hip_atomic_load(&w.iu[((long long)t * w.cstride + j) * 4 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) cum[4 * t + k] += a[k];
  }
  if (cum_ceiling != nullptr) {
    __shared__ unsigned long long acc[2];
    if (t < 2) acc[t] = 0ull;
    __syncthreads();
    for (int e = t; e < R * REF_MAXS; e += 256) {
      const int r = e / REF_MAXS, j = e % REF_MAXS;
      if (j < tab[r].S) {
        const long long* cl = swp->row[r].ceiling + 3 * j;
        atomicAdd(&acc[0], (unsigned long long)__hip_atomic_load(cl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        atomicAdd(&acc[1], (unsigned long long)__hip_atomic_load(cl + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      }
    }
    __syncthreads();
    if (t < 2) cum_ceiling[t] += acc[t];
  }
}

// ---- image synthesis: local (mean-filled) and global (blurred background) views ----
__global__ __launch_bounds__(256) void synth_views_kernel(
    const uint8_t* __restrict__ sam_img, const uint8_t* __restrict__ blurred,
    const float* __restrict__ image_norm, const uint8_t* __restrict__ masks, int N, int H, int W,
    int res, float* __restrict__ local_imgs, float* __restrict__ global_imgs) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long total = (long long)N * res * res;
  if (i >= total) return;
  const int ox = (int)(i % res), oy = (int)((i / res) % res), n = (int)(i / ((long long)res * res));
  const float sy = (float)H / (float)res, sx = (float)W / (float)res;
  float fy = fmaf(sy, oy + 0.5f, -0.5f), fx = fmaf(sx, ox + 0.5f, -0.5f);  // one fma, as ATen
  fy = fy < 0.f ? 0.f : fy;
  fx = fx < 0.f ? 0.f : fx;
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
  const float ly1 = fy - y0, lx1 = fx - x0, ly0 = 1.f - ly1, lx0 = 1.f - lx1;
  const long long HW = (long long)H * W;
  const uint8_t* m = masks + (long long)n * HW;
  const long long t00 = (long long)y0 * W + x0, t01 = (long long)y0 * W + x1;
  const long long t10 = (long long)y1 * W + x0, t11 = (long long)y1 * W + x1;
  const bool m00 = m[t00] != 0, m01 = m[t01] != 0, m10 = m[t10] != 0, m11 = m[t11] != 0;
  const float clip_mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};   // Hybridgl_main.py:93
  const float in_mean[3] = {0.485f, 0.456f, 0.406f};                   // Hybridgl_main.py:117
  const float in_std[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* im = image_norm + (long long)c * HW;
    const float l00 = m00 ? im[t00] : clip_mean[c], l01 = m01 ? im[t01] : clip_mean[c];
    const float l10 = m10 ? im[t10] : clip_mean[c], l11 = m11 ? im[t11] : clip_mean[c];
    const float lv = ly0 * (lx0 * l00 + lx1 * l01) + ly1 * (lx0 * l10 + lx1 * l11);
    const float g00 = (float)(m00 ? sam_img[t00 * 3 + c] : blurred[t00 * 3 + c]) / 255.f;
    const float g01 = (float)(m01 ? sam_img[t01 * 3 + c] : blurred[t01 * 3 + c]) / 255.f;
    const float g10 = (float)(m10 ? sam_img[t10 * 3 + c] : blurred[t10 * 3 + c]) / 255.f;
    const float g11 = (float)(m11 ? sam_img[t11 * 3 + c] : blurred[t11 * 3 + c]) / 255.f;
    const float gv = ly0 * (lx0 * g00 + lx1 * g01) + ly1 * (lx0 * g10 + lx1 * g11);
    const long long o = (((long long)n * 3 + c) * res + oy) * res + ox;
    local_imgs[o] = lv;
    global_imgs[o] = (gv - in_mean[c]) / in_std[c];
  }
}

// ---- the reference's free helpers as standalone kernels (utils.py:135-161 gen_dir_mask, :240-268 relation_boxes) ----
// The fused tail (coherence_scores, score_sentence) does not call these; they exist so that code written against
// the reference's utils.py finds the same functions, evaluated by the same device arithmetic.
__global__ __launch_bounds__(256) void gen_dir_mask_kernel(int dirflag, int H, int W, float* __restrict__ out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= (long long)H * W) return;
  out[i] = dir_weight(dirflag, (int)(i % W), W);
}

__global__ __launch_bounds__(256) void relation_boxes_kernel(const long long* __restrict__ bi, const long long* __restrict__ bj,
                                                             const float* __restrict__ si, const float* __restrict__ sj, int n,
                                                             int rela, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = relation_boxes_dev(bi + 4 * i, bj + 4 * i, si[i], sj[i], rela);
}

// ---- blurred background of the global views (Hybridgl_main.py:99 cv2.GaussianBlur(img, (15,15), 0)) ----------
// OpenCV is a third-party package that is absent offline and its 8-bit fixed-point kernel is unpinned
// (SURVEY.md 8f-2); this is the package's own definition (hybridgl_amd/synth.py box_blur_u8: separable Gaussian with
// OpenCV's sigma rule, reflect-101 borders, double accumulation in tap order, round half up), evaluated with the same
// double operations in the same order so that device and host agree bit for bit.
struct BlurTaps { double w[31]; int k; };

__device__ __forceinline__ int reflect101(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return i;
}

__global__ __launch_bounds__(256) void blur_v_kernel(const uint8_t* __restrict__ img, int H, int W, int C, BlurTaps t,
                                                     double* __restrict__ tmp) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  const long long total = (long long)H * W * C;
  if (i >= total) return;
  const long long wc = (long long)W * C;
  const int y = (int)(i / wc);
  const long long rest = i - (long long)y * wc;
  const int r = t.k / 2;
  double a = 0.0;
  for (int j = 0; j < t.k; ++j) {
    const int yy = reflect101(y + j - r, H);
    const double p = (double)img[(long long)yy * wc + rest];
    a = j == 0 ? __dmul_rn(t.w[0], p) : __dadd_rn(a, __dmul_rn(t.w[j], p));
  }
  tmp[i] = a;
}

__global__ __launch_bounds__(256) void blur_h_kernel(const double* __restrict__ tmp, int H, int W, int C, BlurTaps t,
                                                     uint8_t* __restrict__ out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  const long long total = (long long)H * W * C;
  if (i >= total) return;
  const int c = (int)(i % C);
  const int x = (int)((i / C) % W);
  const long long y = i / ((long long)W * C);
  const int r = t.k / 2;
  double a = 0.0;
  for (int j = 0; j < t.k; ++j) {
    const int xx = reflect101(x + j - r, W);
    const double p = tmp[(y * W + xx) * C + c];
    a = j == 0 ? __dmul_rn(t.w[0], p) : __dadd_rn(a, __dmul_rn(t.w[j], p));
  }
  double v = floor(__dadd_rn(a, 0.5));
  v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
  out[i] = (uint8_t)v;
}

// ---- cv2.GaussianBlur on uint8 (OpenCV 4.x bit-exact path, smooth.simd.hpp fixedSmoothInvoker): both passes in
// integer arithmetic with 8.8 fixed-point taps that sum to 256 -- the row pass gives sum(src * kx) <= 255 * 256 in 16
// bits, the column pass sum(ky * row) in 32 bits, rounded once: (v + 2^15) >> 16.  Reflect-101 borders.
struct BlurTapsQ8 { uint16_t x[31], y[31]; int k; };

__global__ __launch_bounds__(256) void blur_q8_h_kernel(const uint8_t* __restrict__ img, int H, int W, int C, BlurTapsQ8 t,
                                                        uint16_t* __restrict__ tmp) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  const long long total = (long long)H * W * C;
  if (i >= total) return;
  const int c = (int)(i % C);
  const int x = (int)((i / C) % W);
  const long long y = i / ((long long)W * C);
  const int r = t.k / 2;
  unsigned a = 0;
  for (int j = 0; j < t.k; ++j) a += (unsigned)t.x[j] * img[(y * W + reflect101(x + j - r, W)) * C + c];
  tmp[i] = (uint16_t)a;
}

__global__ __launch_bounds__(256) void blur_q8_v_kernel(const uint16_t* __restrict__ tmp, int H, int W, int C, BlurTapsQ8 t,
                                                        uint8_t* __restrict__ out) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  const long long total = (long long)H * W * C;
  if (i >= total) return;
  const long long wc = (long long)W * C;
  const int y = (int)(i / wc);
  const long long rest = i - (long long)y * wc;
  const int r = t.k / 2;
  unsigned a = 0;
  for (int j = 0; j < t.k; ++j) a += (unsigned)t.y[j] * tmp[(long long)reflect101(y + j - r, H) * wc + rest];
  const unsigned v = (a + 32768u) >> 16;
  out[i] = (uint8_t)(v > 255u ? 255u : v);
}

// Both passes in one launch: a workgroup owns a BLUR_TH x BLUR_TW pixel tile, stages the tile and its halo (k / 2 rows and
// columns each side, reflect-101 at the image border) in LDS as bytes, runs the row pass into 16-bit LDS sums and the column pass
// out of them: the image is fetched from HBM once (the halos of neighbouring tiles hit in L2) and no 16-bit intermediate image
// is written and read back (the two-launch form above: every tap of every pixel through the cache, 5.6x the image fetched).
// Same integer arithmetic, same bits.  A thread owns one byte column of the tile in every phase and walks the rows (no
// division inside the loops; the loads of consecutive rows are independent); the taps sit in LDS (indexed from the kernel
// arguments every tap of every row was a scalar load).  Small tiles on purpose: the work of an image is tiny and a thread's
// chain of rows x taps is what the launch takes -- 8 x 32 tiles give 1200 workgroups for 480 x 640.
constexpr int BLUR_TH = 8, BLUR_TW = 32, BLUR_RMAX = 15, BLUR_CMAX = 4, BLUR_NT = 128;
__global__ __launch_bounds__(BLUR_NT) void blur_q8_tile_kernel(const uint8_t* __restrict__ img, int H, int W, int C, BlurTapsQ8 t,
                                                               uint8_t* __restrict__ out) {
  __shared__ uint8_t src[(BLUR_TH + 2 * BLUR_RMAX) * (BLUR_TW + 2 * BLUR_RMAX) * BLUR_CMAX];
  __shared__ uint16_t rsum[(BLUR_TH + 2 * BLUR_RMAX) * BLUR_TW * BLUR_CMAX];
  __shared__ unsigned tapx[32], tapy[32];
  // XCD-aware tile map: workgroups go to the eight XCDs round-robin, each XCD has its own L2 -- with the plain 2-D grid the
  // neighbours of a tile sat on other XCDs and every L2 fetched the shared halo rows for itself (7.6 MB moved per 2.5 MB
  // image).  Here XCD x works through one contiguous run of the row-major tile list: a horizontal band of the image.
  const int gx = (W + BLUR_TW - 1) / BLUR_TW, ntiles = gx * ((H + BLUR_TH - 1) / BLUR_TH), per = (ntiles + 7) >> 3;
  const int tile = (int)(blockIdx.x & 7u) * per + (int)(blockIdx.x >> 3);
  if ((int)(blockIdx.x >> 3) >= per || tile >= ntiles) return;      // (uniform; before any barrier)
  const int ty = tile / gx;
  const int r = t.k / 2, x0 = (tile - ty * gx) * BLUR_TW, y0 = ty * BLUR_TH;
  const int rows = BLUR_TH + 2 * r, cols = BLUR_TW + 2 * r, rowb = cols * C, outb = BLUR_TW * C;
  if (threadIdx.x < 31) { tapx[threadIdx.x] = t.x[threadIdx.x]; tapy[threadIdx.x] = t.y[threadIdx.x]; }
  for (int cb = threadIdx.x; cb < rowb; cb += BLUR_NT) {
    const int xx = cb / C, c = cb - xx * C;
    const uint8_t* const col = img + (long long)reflect101(min(x0 - r + xx, W - 1 + r), W) * C + c;
#pragma unroll 8
    for (int yy = 0; yy < rows; ++yy)
      src[yy * rowb + cb] = col[(long long)reflect101(min(y0 - r + yy, H - 1 + r), H) * W * C];
  }
  __syncthreads();
  for (int ob = threadIdx.x; ob < outb; ob += BLUR_NT) {
#pragma unroll 2
    for (int yy = 0; yy < rows; ++yy) {
      const uint8_t* s0 = src + yy * rowb + ob;
      unsigned a = 0;
      for (int j = 0; j < t.k; ++j) a += tapx[j] * s0[j * C];
      rsum[yy * outb + ob] = (uint16_t)a;
    }
  }
  __syncthreads();
  for (int ob = threadIdx.x; ob < outb; ob += BLUR_NT) {
    if (x0 + ob / C >= W) continue;
    const int ny = min(BLUR_TH, H - y0);
#pragma unroll 2
    for (int yy = 0; yy < ny; ++yy) {
      const uint16_t* s0 = rsum + yy * outb + ob;
      unsigned a = 0;
      for (int j = 0; j < t.k; ++j) a += tapy[j] * s0[j * outb];
      const unsigned v = (a + 32768u) >> 16;
      out[((long long)(y0 + yy) * W + x0) * C + ob] = (uint8_t)(v > 255u ? 255u : v);
    }
  }
}

}  // namespace

extern "C" {

int hgl_calculate_score(const float* img, const float* txt, int N, int T, int E, float logit_scale,
                        float* logits, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(img && txt && logits && N > 0 && T > 0 && E > 0, "calculate_score: bad arguments");
  const int pairs = N * T;
  hipLaunchKernelGGL(calc_score_kernel, dim3((pairs + 3) / 4), dim3(256), 0, (hipStream_t)stream, img, txt, N, T, E, logit_scale, logits);
  return hgl_check_launch("calculate_score");
}

static inline int coh_nblk(int H, int W) {
  return (int)(((long long)H * W + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK);
}
static inline int coh_nparts(int H, int W) { return coh_nblk(H, W) * 4; }

size_t hgl_coherence_workspace_bytes(int N, int H, int W) {
  const size_t nb = coh_nparts(H, W);
  return 256 + hgl_align_up(nb * N * sizeof(double), 256) + hgl_align_up(nb * N * sizeof(unsigned), 256) +
         hgl_align_up(nb * sizeof(double), 256);
}

int hgl_coherence_scores(const float* imgattn, const uint8_t* masks, int N, int H, int W, int dirflag,
                         float black, float* score, void* workspace, size_t workspace_bytes,
                         void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(imgattn && masks && score && N > 0 && H > 0 && W > 0, "coherence: bad arguments");
  HGL_REQUIRE(dirflag >= 0 && dirflag <= 3, "coherence: bad dirflag %d", dirflag);
  if (!workspace || workspace_bytes < hgl_coherence_workspace_bytes(N, H, W)) {
    hgl_set_error("coherence: workspace too small (%zu < %zu)", workspace_bytes, hgl_coherence_workspace_bytes(N, H, W));
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nb = coh_nparts(H, W);
  HglArena ar(workspace, workspace_bytes);
  int* stats = ar.take<int>(64);
  double* psum = ar.take<double>((size_t)nb * N);
  unsigned* pcnt = ar.take<unsigned>((size_t)nb * N);
  double* ptot = ar.take<double>(nb);
  const long long HW = (long long)H * W;
  hipLaunchKernelGGL(init_stats_kernel, dim3(1), dim3(1), 0, st, stats);
  hipLaunchKernelGGL(minmax_kernel, dim3(256), dim3(256), 0, st, imgattn, HW, stats);
  {
    const int nfull = (int)(((long long)H * W) / PIX_PER_BLOCK), ngrp = (N + MASK_GROUP - 1) / MASK_GROUP;
    if (nfull > 0)
      hipLaunchKernelGGL(masked_pool_kernel<true>, dim3(nfull, ngrp), dim3(256), 0, st, imgattn, masks, N, H, W, dirflag, stats, psum, pcnt, ptot, 0);
    if (coh_nblk(H, W) > nfull)
      hipLaunchKernelGGL(masked_pool_kernel<false>, dim3(1, ngrp), dim3(256), 0, st, imgattn, masks, N, H, W, dirflag, stats, psum, pcnt, ptot, nfull);
  }
  hipLaunchKernelGGL(coherence_final_kernel, dim3((N + 3) / 4), dim3(256), 0, st, psum, pcnt, ptot, nb, N, HW, black, score, imgattn, masks, W, dirflag, stats);
  return hgl_check_launch("coherence_scores");
}

int hgl_iou(const uint8_t* pred, const uint8_t* gt, long long HW, int64_t* out_IU, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(pred && gt && out_IU && HW > 0, "iou: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(out_IU, 0, 2 * sizeof(int64_t), st) != hipSuccess) {
    hgl_set_error("iou: memset failed");
    return HGL_ELAUNCH;
  }
  long long blocks = (HW / 16 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(iou_kernel, dim3((unsigned)blocks), dim3(256), 0, st, pred, gt, HW, (unsigned long long*)out_IU);
  return hgl_check_launch("iou");
}

int hgl_iou_select(const uint8_t* masks, const int32_t* idx, int which, const uint8_t* gt,
                   long long HW, int64_t* out_IU, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(masks && idx && gt && out_IU && HW > 0 && which >= 0, "iou_select: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(out_IU, 0, 2 * sizeof(int64_t), st) != hipSuccess) {
    hgl_set_error("iou_select: memset failed");
    return HGL_ELAUNCH;
  }
  long long blocks = (HW / 16 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 512) blocks = 512;
  hipLaunchKernelGGL(iou_select_kernel, dim3((unsigned)blocks), dim3(256), 0, st, masks, (const int*)idx, which, gt, HW, (unsigned long long*)out_IU);
  return hgl_check_launch("iou_select");
}

size_t hgl_score_sentence_workspace_bytes(int N, int E) {
  return hgl_align_up(((size_t)2 * N + 2 * (size_t)E) * sizeof(float), 256);
}

int hgl_score_sentence(const float* hybrid, const float* sentence_feat, const float* noun_phrase_feat,
                       const float* other_noun_feats, int n_other, float r,
                       const int64_t* boxes, const float* gem_score, int N, int E, float logit_scale,
                       int k1, int k2, float alpha, int relaword, int has_other_nouns, int32_t* idx,
                       float* score_clip, float* score_neg, void* workspace, size_t workspace_bytes,
                       void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(hybrid && sentence_feat && noun_phrase_feat && boxes && gem_score && idx && score_clip && score_neg, "score_sentence: null argument");
  HGL_REQUIRE(n_other >= 0 && (n_other == 0 || other_noun_feats), "score_sentence: other_noun_feats missing");
  HGL_REQUIRE(N > 0 && E > 0, "score_sentence: bad shape");
  // Hybridgl_main.py:178-181: k clamps to the number of masks
  if (k1 > N) k1 = N;
  if (k2 > N) k2 = N;
  HGL_REQUIRE(k1 >= 1 && k1 <= MAXK && k2 >= 1 && k2 <= MAXK, "score_sentence: k1,k2 must be in [1,%d]", MAXK);
  HGL_REQUIRE(relaword >= 0 && relaword <= 7, "score_sentence: bad relaword %d", relaword);
  if (!workspace || workspace_bytes < hgl_score_sentence_workspace_bytes(N, E)) {
    hgl_set_error("score_sentence: workspace too small");
    return HGL_EWORKSPACE;
  }
  float* pool = (float*)workspace;
  hipLaunchKernelGGL(score_sentence_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, hybrid, sentence_feat, noun_phrase_feat, other_noun_feats, n_other, r, (const long long*)boxes, gem_score, N, E, logit_scale, k1, k2, alpha, relaword, has_other_nouns, (int*)idx, score_clip, score_neg, pool);
  return hgl_check_launch("score_sentence");
}

static size_t ref_ws_layout(int S, int N, int E, int H, int W, size_t* off) {
  const size_t nparts = coh_nparts(H, W);
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += hgl_align_up(bytes, 256); return at; };
  off[0] = take((size_t)S * REF_MM_BLOCKS * 2 * sizeof(float));          // part_mm
  off[1] = take((size_t)S * nparts * N * sizeof(double));                 // part_sum
  off[2] = take(nparts * (size_t)N * sizeof(unsigned));                   // part_cnt
  off[3] = take((size_t)S * nparts * sizeof(double));                     // part_tot
  off[4] = take((size_t)S * (2 * (size_t)N + 2 * (size_t)E) * sizeof(float));   // soft-max + text scratch per sentence
  off[5] = take((size_t)3 * S * N * sizeof(float));                       // gem / clip / neg when the caller does not want them
  off[6] = take(256);                                                     // done counter
  return o;
}

// ---- the one host path of the fused tail: hgl_score_ref and hgl_score_group ---------------------------------------------------
// Both entries hand over a list of ROWS.  A row is an HglGroupRef that holds at most REF_MAXS sentences: a ref of S <= 16
// sentences as it is, a ref of more as ceil(S / 16) rows that share its hybrid / text / boxes / masks, each with its chunk of the
// sentences and the output pointers moved to that chunk.  Up to GRP_MAXR rows go through one set of launches.
}  // extern "C"
namespace {
struct TailCall {
  std::vector<HglGroupRef> rows;
  int E;
  float logit_scale, r, alpha;
  int64_t* cum;
  hipStream_t st;
  int mask_group;      // masks per pooling workgroup: MASK_GROUP (hgl_score_ref) or REF_MASK_GROUP (hgl_score_group)
};

// hgl_score_group_sweep: what the rows of a TailCall carry besides (rows[i] belongs to TailCall::rows[i]; the rows' idx / iu
// are the sweep's [C,S,2] / [C,S,4] arrays at the row's first sentence)
struct SweepRowHost {
  const int32_t* k;       // HOST [C,2]: the ref's k1, k2 per configuration
  int S_total;            // sentences of the whole ref
  int64_t* ceiling;       // [S,3] of the row
};
struct SweepCall {
  const HglSweepConfig* cfg;
  int C, nr;
  float r[SWP_MAXR];                    // the distinct r (by bit pattern), in order of first appearance
  unsigned char rgrp[SWP_MAXC];
  std::vector<SweepRowHost> rows;
  int64_t* cum_ceiling;
};

// the sweep's part of a launch's workspace, behind the tail's own: SweepTab, then what is zeroed before every launch (the
// counter of finished blocks and the rows' tables), then the rows' scoring scratch
size_t sweep_ws_layout(const HglGroupRef* rows, int n, int E, int nr, size_t* tab_off, size_t* scratch_off, size_t* zero_end) {
  size_t o = hgl_align_up(sizeof(SweepTab), 256) + 256;
  for (int i = 0; i < n; ++i) {
    if (tab_off) tab_off[i] = o;
    o += hgl_align_up(((REF_MAXS + 1) * (size_t)rows[i].N + REF_MAXS) * sizeof(unsigned long long), 256);
  }
  if (zero_end) *zero_end = o;
  for (int i = 0; i < n; ++i) {
    if (scratch_off) scratch_off[i] = o;
    o += hgl_align_up((size_t)rows[i].S * nr * (5 * (size_t)rows[i].N + 2 * (size_t)E) * sizeof(float), 256);
  }
  return o;
}

// everything an entry requires of a ref; clamps k1 / k2 to the number of masks in place (Hybridgl_main.py:178-181).
// who: "score_ref" or "score_group: ref 3"
int tail_check_ref(HglGroupRef& q, int E, const char* who) {
  HGL_REQUIRE(q.hybrid && q.text && q.boxes && q.masks && q.sentences && q.idx && q.iu, "%s: null argument", who);
  HGL_REQUIRE(q.N > 0 && E > 0 && q.H > 0 && q.W > 0 && q.S > 0 && q.T > 0, "%s: bad shape", who);
  if (q.k1 > q.N) q.k1 = q.N;
  if (q.k2 > q.N) q.k2 = q.N;
  HGL_REQUIRE(q.k1 >= 1 && q.k1 <= MAXK && q.k2 >= 1 && q.k2 <= MAXK, "%s: k1,k2 must be in [1,%d]", who, MAXK);
  for (int s = 0; s < q.S; ++s) {
    const HglSentence& t = q.sentences[s];
    HGL_REQUIRE(t.imgattn && t.target, "%s: sentence %d has no heat-map / target", who, s);
    HGL_REQUIRE(t.sentence_row >= 0 && t.sentence_row < q.T && t.noun_phrase_row >= 0 && t.noun_phrase_row < q.T,
                "%s: sentence %d: text row out of range", who, s);
    HGL_REQUIRE(t.n_other >= 0 && (t.n_other == 0 || (t.other_row0 >= 0 && t.other_row0 + t.n_other <= q.T)),
                "%s: sentence %d: other-noun rows out of range", who, s);
    HGL_REQUIRE(t.dirflag >= 0 && t.dirflag <= 3 && t.relaword >= 0 && t.relaword <= 7, "%s: sentence %d: bad dirflag / relaword", who, s);
  }
  return HGL_OK;
}

void tail_fill_sentences(RefSentences& rs, const HglSentence* sent, int S) {
  for (int j = 0; j < S; ++j) {
    const HglSentence& t = sent[j];
    rs.attn[j] = t.imgattn; rs.target[j] = t.target;
    rs.sent_row[j] = t.sentence_row; rs.nphr_row[j] = t.noun_phrase_row;
    rs.other_row0[j] = t.n_other > 0 ? t.other_row0 : 0; rs.n_other[j] = t.n_other;
    rs.dirflag[j] = t.dirflag; rs.rela[j] = t.relaword; rs.has_other[j] = t.has_other_nouns; rs.black[j] = t.black;
  }
}

// the rows of a ref
void tail_push_rows(std::vector<HglGroupRef>& rows, const HglGroupRef& q) {
  for (int s0 = 0; s0 < q.S; s0 += REF_MAXS) {
    HglGroupRef row = q;
    row.sentences = q.sentences + s0;
    row.S = q.S - s0 < REF_MAXS ? q.S - s0 : REF_MAXS;
    row.idx = q.idx ? q.idx + 2 * s0 : nullptr;
    row.iu = q.iu ? q.iu + 4 * s0 : nullptr;
    row.score_clip = q.score_clip ? q.score_clip + (long long)s0 * q.N : nullptr;
    row.score_neg = q.score_neg ? q.score_neg + (long long)s0 * q.N : nullptr;
    row.gem_score = q.gem_score ? q.gem_score + (long long)s0 * q.N : nullptr;
    rows.push_back(row);
  }
}

// workspace of one launch: the descriptor table and the done counter, then one ref_ws_layout per row
size_t tail_ws_layout(const HglGroupRef* rows, int n, int E, size_t* row_off) {
  size_t o = hgl_align_up((size_t)GRP_MAXR * sizeof(GroupRefDev), 256) + 256;
  for (int i = 0; i < n; ++i) {
    size_t off[7];
    if (row_off) row_off[i] = o;
    o += ref_ws_layout(rows[i].S, rows[i].N, E, rows[i].H, rows[i].W, off);
  }
  return o;
}
// ... and of a call: its launches run one after the other on the stream and share it
// (sweep_nr > 0: a sweep over that many distinct r -- every launch's sweep_ws_layout behind its tail_ws_layout)
size_t tail_ws_bytes(const std::vector<HglGroupRef>& rows, int E, int sweep_nr = 0) {
  size_t total = 0;
  for (size_t r0 = 0; r0 < rows.size(); r0 += GRP_MAXR) {
    const int rc = (int)(rows.size() - r0 < GRP_MAXR ? rows.size() - r0 : GRP_MAXR);
    size_t n = tail_ws_layout(rows.data() + r0, rc, E, nullptr);
    if (sweep_nr > 0) n = hgl_align_up(n, 256) + sweep_ws_layout(rows.data() + r0, rc, E, sweep_nr, nullptr, nullptr, nullptr);
    total = n > total ? n : total;
  }
  return total;
}

// Pinned staging slots of the descriptor table (a slot is reused only after the copy out of it has completed): one ring PER DEVICE (an event belongs to the device it was
// created on), a slot is held (busy) by one host thread from the moment it is picked until its event has been recorded behind
// the upload, and every event call is checked -- a failed record must not leave a slot looking reusable.
struct GrpStage {
  static constexpr int SLOTS = 8, DEVS = 64;
  struct Ring {
    void* buf[SLOTS] = {nullptr};
    hipEvent_t ev[SLOTS];
    bool used[SLOTS] = {false};     // the event has been recorded at least once
    bool busy[SLOTS] = {false};     // picked by a thread that has not recorded yet
    int next = 0;
  };
  Ring ring[DEVS];
  std::mutex mu;
  std::condition_variable freed;
};
GrpStage g_grp_stage;

// picks a slot of the current device's ring (waits while all eight are held by other threads); < 0 on error
int grp_stage_acquire(int* dev_out, void** host) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= GrpStage::DEVS) {
    hgl_set_error("scoring tail: cannot tell the current device");
    return -1;
  }
  GrpStage::Ring& rg = g_grp_stage.ring[dev];
  int slot = -1;
  {
    std::unique_lock<std::mutex> lk(g_grp_stage.mu);
    for (;;) {
      for (int i = 0; i < GrpStage::SLOTS && slot < 0; ++i) {
        const int c = (rg.next + i) % GrpStage::SLOTS;
        if (!rg.busy[c]) slot = c;
      }
      if (slot >= 0) break;
      g_grp_stage.freed.wait(lk);
    }
    rg.busy[slot] = true;
    rg.next = (slot + 1) % GrpStage::SLOTS;
  }
  bool ok = true;
  if (!rg.buf[slot]) {       // only the holder of a busy slot touches its buffer and event
    ok = hipHostMalloc(&rg.buf[slot], GRP_MAXR * sizeof(GroupRefDev) + sizeof(SweepTab), hipHostMallocDefault) == hipSuccess;      // (a sweep's table rides behind the rows')
    if (ok && hipEventCreateWithFlags(&rg.ev[slot], hipEventDisableTiming) != hipSuccess) {
      (void)hipHostFree(rg.buf[slot]);
      rg.buf[slot] = nullptr;
      ok = false;
    }
    if (!ok) hgl_set_error("scoring tail: cannot allocate the pinned descriptor slot");
  } else if (rg.used[slot]) {
    ok = hipEventSynchronize(rg.ev[slot]) == hipSuccess;      // the upload that last read this slot: eight calls ago
    if (!ok) hgl_set_error("scoring tail: waiting for a descriptor slot failed");
  }
  if (!ok) {
    (void)hipGetLastError();
    std::lock_guard<std::mutex> lk(g_grp_stage.mu);
    rg.busy[slot] = false;
    g_grp_stage.freed.notify_one();
    return -1;
  }
  *dev_out = dev;
  *host = rg.buf[slot];
  return slot;
}

// records the slot's event behind the upload on `st` and hands the slot back; false when the record failed (the caller then
// synchronises the stream itself before the slot can be rewritten)
bool grp_stage_release(int dev, int slot, hipStream_t st) {
  GrpStage::Ring& rg = g_grp_stage.ring[dev];
  bool ok = hipEventRecord(rg.ev[slot], st) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    ok = hipStreamSynchronize(st) == hipSuccess;      // no event to wait on later: make the upload complete now
  }
  std::lock_guard<std::mutex> lk(g_grp_stage.mu);
  rg.used[slot] = ok ? true : rg.used[slot];     // a failed record left the earlier event (if any) in place, and the stream was drained
  rg.busy[slot] = false;
  g_grp_stage.freed.notify_one();
  return ok;
}
// the pooling launches of the rows of a table, MG masks per workgroup; CH = 3 when no row has more than three sentences
template <int MG>
void tail_launch_pool(const GroupRefDev* tab, int rc, int maxS, int max_nblk, int maxN, bool any_partial, hipStream_t st) {
  const int max_groups = (maxN + MG - 1) / MG;
  if (maxS <= 3)
    hipLaunchKernelGGL((grp_masked_pool_kernel<MG, 3>), dim3(max_nblk, max_groups, rc), dim3(256), 0, st, tab);
  else
    hipLaunchKernelGGL((grp_masked_pool_kernel<MG, 4>), dim3(max_nblk, max_groups, rc), dim3(256), 0, st, tab);
  if (any_partial)
    hipLaunchKernelGGL(grp_masked_pool_last_kernel<MG>, dim3(1, max_groups, rc), dim3(256), 0, st, tab);
}

// checked rows -> launches.  who: the entry's name, for its messages
// sw: the call is a sweep -- after the pooling, the IoU table and the sweep's scoring instead of grp_score_kernel / grp_iou_kernel
int tail_launch(const TailCall& c, void* workspace, size_t workspace_bytes, const char* who, const SweepCall* sw = nullptr) {
  const size_t need = tail_ws_bytes(c.rows, c.E, sw ? sw->nr : 0);
  if (!workspace || workspace_bytes < need) {
    hgl_set_error("%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
    return HGL_EWORKSPACE;
  }
  char* base = (char*)workspace;
  const int R = (int)c.rows.size();
  for (int r0 = 0; r0 < R; r0 += GRP_MAXR) {
    const int rc = R - r0 < GRP_MAXR ? R - r0 : GRP_MAXR;
    size_t row_off[GRP_MAXR];
    tail_ws_layout(c.rows.data() + r0, rc, c.E, row_off);
    // the descriptor table, built in a pinned slot and copied in front of the workspace on the stream
    void* host_v = nullptr;
    int stage_dev = 0;
    const int slot = grp_stage_acquire(&stage_dev, &host_v);
    if (slot < 0) return HGL_ELAUNCH;
    GroupRefDev* host = (GroupRefDev*)host_v;
    int maxS = 0, max_nblk = 0, maxN = 0;
    bool any_partial = false;      // a row whose plane does not end on a block boundary: the pooling's second, small launch
    long long max_iou_blocks = 1;
    for (int i = 0; i < rc; ++i) {
      const HglGroupRef& q = c.rows[r0 + i];
      GroupRefDev& d = host[i];
      memset(&d, 0, sizeof(d));
      tail_fill_sentences(d.rs, q.sentences, q.S);
      d.S = q.S; d.N = q.N; d.H = q.H; d.W = q.W; d.k1 = q.k1; d.k2 = q.k2;
      d.nparts = coh_nparts(q.H, q.W);
      d.nblk = coh_nblk(q.H, q.W);
      d.hybrid = q.hybrid; d.text = q.text; d.boxes = (const long long*)q.boxes; d.masks = q.masks;
      size_t off[7];
      ref_ws_layout(q.S, q.N, c.E, q.H, q.W, off);
      char* rb = base + row_off[i];
      d.part_mm = (float*)(rb + off[0]);
      d.part_sum = (double*)(rb + off[1]);
      d.part_cnt = (unsigned*)(rb + off[2]);
      d.part_tot = (double*)(rb + off[3]);
      d.soft = (float*)(rb + off[4]);
      float* spare = (float*)(rb + off[5]);
      d.gem = q.gem_score ? q.gem_score : spare;
      d.clip = q.score_clip ? q.score_clip : spare + (long long)q.S * q.N;
      d.neg = q.score_neg ? q.score_neg : spare + 2ll * q.S * q.N;
      d.idx = (int*)q.idx;
      d.iu = (unsigned long long*)q.iu;
      maxS = q.S > maxS ? q.S : maxS;
      maxN = q.N > maxN ? q.N : maxN;
      max_nblk = d.nblk > max_nblk ? d.nblk : max_nblk;
      any_partial = any_partial || ((long long)q.H * q.W) % PIX_PER_BLOCK != 0;
      long long blocks = ((long long)q.H * q.W / 16 + 1023) / 1024;      // four 16-byte words per thread
      blocks = blocks < 1 ? 1 : (blocks > 32 ? 32 : blocks);
      max_iou_blocks = blocks > max_iou_blocks ? blocks : max_iou_blocks;
    }
    const GroupRefDev* tab = (const GroupRefDev*)base;
    unsigned* done = (unsigned*)(base + hgl_align_up((size_t)GRP_MAXR * sizeof(GroupRefDev), 256));
    bool uploaded = hipMemcpyAsync(base, host, (size_t)rc * sizeof(GroupRefDev), hipMemcpyHostToDevice, c.st) == hipSuccess;
    char* sbase = nullptr;        // the sweep's part of the workspace, its table built in the same pinned slot
    size_t zero_end = 0;
    if (sw) {
      SweepTab* ht = (SweepTab*)(host + GRP_MAXR);
      memset(ht, 0, sizeof(*ht));
      ht->C = sw->C; ht->nr = sw->nr;
      memcpy(ht->r, sw->r, sizeof(ht->r));
      memcpy(ht->rgrp, sw->rgrp, sizeof(ht->rgrp));
      for (int j = 0; j < sw->C; ++j) ht->alpha[j] = sw->cfg[j].alpha;
      sbase = base + hgl_align_up(tail_ws_layout(c.rows.data() + r0, rc, c.E, nullptr), 256);
      size_t tab_off[GRP_MAXR], scratch_off[GRP_MAXR];
      sweep_ws_layout(c.rows.data() + r0, rc, c.E, sw->nr, tab_off, scratch_off, &zero_end);
      for (int i = 0; i < rc; ++i) {
        const HglGroupRef& q = c.rows[r0 + i];
        const SweepRowHost& h = sw->rows[r0 + i];
        SweepRowDev& d = ht->row[i];
        for (int j = 0; j < sw->C; ++j)
          for (int e = 0; e < 2; ++e) {
            const int k = h.k[2 * j + e] > q.N ? q.N : h.k[2 * j + e];      // validated by the entry
            d.k[j][e] = (unsigned char)k;
            unsigned char& m = d.kmax[sw->rgrp[j]][e];
            m = m > k ? m : (unsigned char)k;
          }
        for (int j = 0; j < q.S; ++j) {      // a target pointer is counted once
          int at = 0;
          while (at < d.nt && d.tptr[at] != q.sentences[j].target) ++at;
          if (at == d.nt) d.tptr[d.nt++] = q.sentences[j].target;
          d.tslot[j] = at;
        }
        d.cstride = h.S_total;
        d.idx = (int*)q.idx;
        d.iu = (unsigned long long*)q.iu;
        d.ceiling = (long long*)h.ceiling;
        d.tab = (unsigned long long*)(sbase + tab_off[i]);
        d.scratch = (float*)(sbase + scratch_off[i]);
      }
      uploaded = uploaded && hipMemcpyAsync(sbase, ht, sizeof(SweepTab), hipMemcpyHostToDevice, c.st) == hipSuccess;
    }
    if (!grp_stage_release(stage_dev, slot, c.st) || !uploaded) {
      hgl_set_error("%s: descriptor upload failed", who);
      return HGL_ELAUNCH;
    }
    hipLaunchKernelGGL(grp_minmax_kernel, dim3(REF_MM_BLOCKS, maxS, rc), dim3(256), 0, c.st, tab);
    if (c.mask_group == MASK_GROUP)
      tail_launch_pool<MASK_GROUP>(tab, rc, maxS, max_nblk, maxN, any_partial, c.st);
    else
      tail_launch_pool<REF_MASK_GROUP>(tab, rc, maxS, max_nblk, maxN, any_partial, c.st);
    if (sw) {
      const size_t zero0 = hgl_align_up(sizeof(SweepTab), 256);
      if (hipMemsetAsync(sbase + zero0, 0, zero_end - zero0, c.st) != hipSuccess) {
        hgl_set_error("%s: memset failed", who);
        return HGL_ELAUNCH;
      }
      const SweepTab* stab = (const SweepTab*)sbase;
      hipLaunchKernelGGL(grp_iou_table_kernel, dim3(max_nblk, (maxN + TAB_MG - 1) / TAB_MG, rc), dim3(256), 0, c.st, tab, stab);
      hipLaunchKernelGGL(grp_sweep_score_kernel, dim3(maxS, sw->nr, rc), dim3(256), 0, c.st, tab, stab, rc, c.E, c.logit_scale,
                         (unsigned long long*)c.cum, (unsigned long long*)sw->cum_ceiling, (unsigned*)(sbase + zero0));
      continue;
    }
    hipLaunchKernelGGL(grp_score_kernel, dim3(maxS, rc), dim3(256), 0, c.st, tab, c.E, c.logit_scale, c.r, c.alpha, done);
    hipLaunchKernelGGL(grp_iou_kernel, dim3((unsigned)max_iou_blocks, 2 * maxS, rc), dim3(256), 0, c.st, tab, rc,
                       (unsigned long long*)c.cum, done);
  }
  return hgl_check_launch(who);
}
}  // namespace

extern "C" {

size_t hgl_score_ref_workspace_bytes(int S, int N, int E, int H, int W) {
  HglGroupRef q;
  memset(&q, 0, sizeof(q));
  q.S = S; q.N = N; q.H = H; q.W = W;
  std::vector<HglGroupRef> rows;
  tail_push_rows(rows, q);
  return tail_ws_bytes(rows, E);
}

int hgl_score_ref(const float* hybrid, const float* text, int T, const int64_t* boxes, const uint8_t* masks, int N, int E,
                  int H, int W, const HglSentence* sentences, int S, float logit_scale, float r, int k1, int k2, float alpha,
                  int32_t* idx, int64_t* iu, int64_t* cum, float* score_clip, float* score_neg, float* gem_score,
                  void* workspace, size_t workspace_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HglGroupRef q = {hybrid, text, T, boxes, masks, N, H, W, sentences, S, k1, k2, idx, iu, score_clip, score_neg, gem_score};
  HGL_TRY(tail_check_ref(q, E, "score_ref"));
  TailCall c = {{}, E, logit_scale, r, alpha, cum, (hipStream_t)stream, MASK_GROUP};
  tail_push_rows(c.rows, q);
  return tail_launch(c, workspace, workspace_bytes, "score_ref");
}

size_t hgl_score_group_workspace_bytes(const HglGroupRef* refs, int R, int E) {
  if (!refs || R <= 0 || E <= 0) return 0;
  std::vector<HglGroupRef> rows;
  for (int i = 0; i < R; ++i) tail_push_rows(rows, refs[i]);
  return tail_ws_bytes(rows, E);
}

int hgl_score_group(const HglGroupRef* refs, int R, int E, float logit_scale, float r, float alpha, int64_t* cum, void* workspace,
                    size_t workspace_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(refs && R > 0 && E > 0, "score_group: bad arguments");
  TailCall c = {{}, E, logit_scale, r, alpha, cum, (hipStream_t)stream, REF_MASK_GROUP};
  for (int i = 0; i < R; ++i) {
    char who[40];
    snprintf(who, sizeof(who), "score_group: ref %d", i);
    HglGroupRef q = refs[i];
    HGL_TRY(tail_check_ref(q, E, who));
    tail_push_rows(c.rows, q);
  }
  return tail_launch(c, workspace, workspace_bytes, "score_group");
}

}  // extern "C"
namespace {
// the checks of the sweep entry on its configurations; fills the distinct r and every configuration's group
int sweep_check_configs(SweepCall& sw) {
  HGL_REQUIRE(sw.C >= 1 && sw.C <= SWP_MAXC, "score_group_sweep: %d configurations (1 .. %d)", sw.C, SWP_MAXC);
  HGL_REQUIRE(sw.cfg, "score_group_sweep: null argument");
  sw.nr = 0;
  for (int j = 0; j < sw.C; ++j) {
    int at = 0;
    while (at < sw.nr && memcmp(&sw.r[at], &sw.cfg[j].r, sizeof(float)) != 0) ++at;
    if (at == sw.nr) {
      HGL_REQUIRE(sw.nr < SWP_MAXR, "score_group_sweep: more than %d distinct r", SWP_MAXR);
      sw.r[sw.nr++] = sw.cfg[j].r;
    }
    sw.rgrp[j] = (unsigned char)at;
  }
  return HGL_OK;
}
}  // namespace
extern "C" {

size_t hgl_score_group_sweep_workspace_bytes(const HglGroupRef* refs, int R, int E, const HglSweepConfig* configs, int C) {
  if (!refs || R <= 0 || E <= 0) return 0;
  SweepCall sw = {};
  sw.cfg = configs; sw.C = C;
  if (sweep_check_configs(sw) != HGL_OK) return 0;
  std::vector<HglGroupRef> rows;
  for (int i = 0; i < R; ++i) tail_push_rows(rows, refs[i]);
  return tail_ws_bytes(rows, E, sw.nr);
}

int hgl_score_group_sweep(const HglGroupRef* refs, const HglSweepRef* sweep, int R, int E, float logit_scale,
                          const HglSweepConfig* configs, int C, int64_t* cum, int64_t* cum_ceiling, void* workspace,
                          size_t workspace_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(refs && sweep && R > 0 && E > 0, "score_group_sweep: bad arguments");
  SweepCall sw = {};
  sw.cfg = configs; sw.C = C; sw.cum_ceiling = cum_ceiling;
  HGL_TRY(sweep_check_configs(sw));
  TailCall c = {{}, E, logit_scale, 0.f, 0.f, cum, (hipStream_t)stream, REF_MASK_GROUP};
  for (int i = 0; i < R; ++i) {
    char who[48];
    snprintf(who, sizeof(who), "score_group_sweep: ref %d", i);
    HglGroupRef q = refs[i];
    // the ref's own k1 / k2 / idx / iu / score rows are not part of this entry: the sweep's outputs stand in their place
    q.idx = sweep[i].idx; q.iu = sweep[i].iu; q.k1 = q.k2 = 1;
    q.score_clip = q.score_neg = q.gem_score = nullptr;
    HGL_REQUIRE(sweep[i].k && sweep[i].ceiling, "%s: null argument", who);
    HGL_TRY(tail_check_ref(q, E, who));
    for (int j = 0; j < 2 * C; ++j) {
      const int k = sweep[i].k[j] > q.N ? q.N : sweep[i].k[j];
      HGL_REQUIRE(k >= 1 && k <= MAXK, "%s: configuration %d: k1,k2 must be in [1,%d]", who, j / 2, MAXK);
    }
    const size_t first = c.rows.size();
    tail_push_rows(c.rows, q);
    for (size_t rix = first; rix < c.rows.size(); ++rix) {
      HglGroupRef& row = c.rows[rix];
      const long long s0 = row.sentences - q.sentences;
      // tail_push_rows moved idx / iu by the row's first sentence within ONE configuration: what the sweep's layout needs too
      sw.rows.push_back({sweep[i].k, q.S, sweep[i].ceiling + 3 * s0});
    }
  }
  return tail_launch(c, workspace, workspace_bytes, "score_group_sweep", &sw);
}

int hgl_gen_dir_mask(int dirflag, int H, int W, float* out, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(out && H > 0 && W > 0 && dirflag >= 0 && dirflag <= 3, "gen_dir_mask: bad arguments");
  hipLaunchKernelGGL(gen_dir_mask_kernel, dim3((unsigned)(((long long)H * W + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     dirflag, H, W, out);
  return hgl_check_launch("gen_dir_mask");
}

int hgl_relation_boxes(const int64_t* boxes_i, const int64_t* boxes_j, const float* score_i, const float* score_j, int n,
                       int relaword, float* out, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(boxes_i && boxes_j && score_i && score_j && out && n > 0, "relation_boxes: bad arguments");
  HGL_REQUIRE(relaword >= 0 && relaword <= 7, "relation_boxes: bad relaword %d", relaword);
  hipLaunchKernelGGL(relation_boxes_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const long long*)boxes_i,
                     (const long long*)boxes_j, score_i, score_j, n, relaword, out);
  return hgl_check_launch("relation_boxes");
}

size_t hgl_gaussian_blur_u8_workspace_bytes(int H, int W, int C) { return hgl_align_up((size_t)H * W * C * sizeof(double), 256); }

int hgl_gaussian_blur_u8(const uint8_t* img, int H, int W, int C, const double* taps, int k, uint8_t* out, void* workspace,
                         size_t workspace_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(img && out && taps && H > 0 && W > 0 && C > 0, "gaussian_blur_u8: bad arguments");
  HGL_REQUIRE(k >= 1 && k <= 31 && (k & 1) && k / 2 < H && k / 2 < W, "gaussian_blur_u8: kernel size %d unsupported for %dx%d", k, H, W);
  if (!workspace || workspace_bytes < hgl_gaussian_blur_u8_workspace_bytes(H, W, C)) {
    hgl_set_error("gaussian_blur_u8: workspace too small");
    return HGL_EWORKSPACE;
  }
  BlurTaps t;
  t.k = k;
  for (int i = 0; i < 31; ++i) t.w[i] = i < k ? taps[i] : 0.0;
  const long long total = (long long)H * W * C;
  const unsigned blocks = (unsigned)((total + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(blur_v_kernel, dim3(blocks), dim3(256), 0, st, img, H, W, C, t, (double*)workspace);
  hipLaunchKernelGGL(blur_h_kernel, dim3(blocks), dim3(256), 0, st, (const double*)workspace, H, W, C, t, out);
  return hgl_check_launch("gaussian_blur_u8");
}

int hgl_gaussian_blur_u8_q8(const uint8_t* img, int H, int W, int C, const uint16_t* taps_x, const uint16_t* taps_y, int k,
                            uint8_t* out, void* workspace, size_t workspace_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(img && out && taps_x && taps_y && H > 0 && W > 0 && C > 0, "gaussian_blur_u8_q8: bad arguments");
  HGL_REQUIRE(k >= 1 && k <= 31 && (k & 1) && k / 2 < H && k / 2 < W, "gaussian_blur_u8_q8: kernel size %d unsupported for %dx%d", k, H, W);
  if (!workspace || workspace_bytes < (size_t)H * W * C * sizeof(uint16_t)) {
    hgl_set_error("gaussian_blur_u8_q8: workspace too small");
    return HGL_EWORKSPACE;
  }
  BlurTapsQ8 t;
  t.k = k;
  unsigned sx = 0, sy = 0;
  for (int i = 0; i < 31; ++i) {
    t.x[i] = i < k ? taps_x[i] : 0;
    t.y[i] = i < k ? taps_y[i] : 0;
    sx += t.x[i];
    sy += t.y[i];
  }
  HGL_REQUIRE(sx == 256 && sy == 256, "gaussian_blur_u8_q8: the 8.8 fixed-point taps must sum to 256 (got %u, %u)", sx, sy);
  const long long total = (long long)H * W * C;
  const unsigned blocks = (unsigned)((total + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  if (C <= BLUR_CMAX) {      // (the workspace stays part of the signature: wider pixels take the two-launch form)
    const int ntiles = ((W + BLUR_TW - 1) / BLUR_TW) * ((H + BLUR_TH - 1) / BLUR_TH);
    hipLaunchKernelGGL(blur_q8_tile_kernel, dim3((unsigned)(8 * ((ntiles + 7) / 8))), dim3(BLUR_NT), 0, st, img, H, W, C, t, out);
    return hgl_check_launch("gaussian_blur_u8_q8");
  }
  hipLaunchKernelGGL(blur_q8_h_kernel, dim3(blocks), dim3(256), 0, st, img, H, W, C, t, (uint16_t*)workspace);
  hipLaunchKernelGGL(blur_q8_v_kernel, dim3(blocks), dim3(256), 0, st, (const uint16_t*)workspace, H, W, C, t, out);
  return hgl_check_launch("gaussian_blur_u8_q8");
}

int hgl_synthesize_views(const uint8_t* sam_img, const uint8_t* blurred, const float* image_norm,
                         const uint8_t* masks, int N, int H, int W, int res, float* local_imgs,
                         float* global_imgs, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(sam_img && blurred && image_norm && masks && local_imgs && global_imgs, "synthesize_views: null argument");
  HGL_REQUIRE(N > 0 && H > 0 && W > 0 && res > 0, "synthesize_views: bad shape");
  const long long total = (long long)N * res * res;
  hipLaunchKernelGGL(synth_views_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sam_img, blurred, image_norm, masks, N, H, W, res, local_imgs, global_imgs);
  return hgl_check_launch("synthesize_views");
}

}  // extern "C"
