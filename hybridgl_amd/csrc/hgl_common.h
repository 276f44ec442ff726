// Internal declarations shared by the HIP translation units of libhybridgl.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include <atomic>
#include <type_traits>
#include "../../include/hybridgl.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#ifdef __HIPCC__
// fp32 -> fp16 (hi, lo) with hi + lo == x up to the rounding of lo.  x must reach BOTH conversions as the same,
// already rounded fp32 value: when x is the result of a multiply / fma the compiler may otherwise fold that
// arithmetic into one of the conversions (single rounding from the exact product) and not the other, so that on
// ties the stored hi and the hi subtracted for lo are different fp16 neighbours and hi + lo misses x by 2*|lo|
// (measured: 0.1 % of attention rows off by up to 8e-5 relative).  The empty asm makes x opaque.
//
// Range: |x| > 65504 does not fit fp16 (hi = inf, lo = x - inf = -inf, and the MFMA sum is NaN).  The splits of values
// that are not bounded by construction -- GEMM outputs (epilogues with a split output, the attention's Q / K / V staging,
// the skinny kernel's A operand, the generic split kernel) -- go through the 4-argument form, which also folds |x| into a
// per-thread running maximum (one v_max per element, no branch); hgl_split_commit() at the end of the thread counts the
// thread in a per-translation-unit device counter when that maximum left the range.  hgl_split_overflow_count() sums the
// counters: the run then contains inf / NaN AND the host is told (hybridgl_amd raises and points at HYBRIDGL_PRECISION=f32)
// -- never silently.  LayerNorm outputs (|y| <= sqrt(D) |w| + |b|), normalised pixels, probabilities and convex
// combinations of already-checked values use the 3-argument form.  Weights are pre-scaled by a power of two and cannot
// overflow; activations of the trained CLIP / SAM models stay two to three orders of magnitude below the limit.
static __device__ __attribute__((unused)) unsigned int hgl_tu_split_overflow;
__device__ __forceinline__ void hgl_split_hi_lo(float x, _Float16& hi, _Float16& lo) {
  asm volatile("" : "+v"(x));
  hi = (_Float16)x;
  lo = (_Float16)(x - (float)hi);
}
__device__ __forceinline__ void hgl_split_hi_lo(float x, _Float16& hi, _Float16& lo, float& amax) {
  asm volatile("" : "+v"(x));
  amax = fmaxf(amax, fabsf(x));      // a NaN is ignored here (maxNum) and stays a NaN in hi / lo
  hi = (_Float16)x;
  lo = (_Float16)(x - (float)hi);
}
__device__ __forceinline__ void hgl_split_commit(float amax) {
  if (__builtin_expect(amax > 65504.0f, 0)) atomicAdd(&hgl_tu_split_overflow, 1u);
}
// host-side reader of this translation unit's counter (define once in every .hip that commits)
#define HGL_DEFINE_SPLIT_OVERFLOW_READER(name)                                                        \
  unsigned long long name(int reset) {                                                                \
    unsigned int v = 0;                                                                               \
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(hgl_tu_split_overflow), sizeof(v)) != hipSuccess) return 0; \
    if (reset && v) {                                                                                 \
      const unsigned int z = 0;                                                                       \
      (void)hipMemcpyToSymbol(HIP_SYMBOL(hgl_tu_split_overflow), &z, sizeof(z));                      \
    }                                                                                                 \
    return v;                                                                                         \
  }                                                                                                   \
  int name##_peek(unsigned int* dst, hipStream_t st) {                                                \
    return hipMemcpyFromSymbolAsync(dst, HIP_SYMBOL(hgl_tu_split_overflow), sizeof(unsigned int), 0,  \
                                    hipMemcpyDeviceToHost, st) == hipSuccess ? 0 : -1;                \
  }
// ---- activations of the GEMM epilogues ------------------------------------------------------------------------------
// nn.GELU (erf form; segment_anything/modeling/common.py:13-24 MLPBlock, mask_decoder.py:76-80): 0.5 x (1 + erf(x / sqrt 2)).
// The library erff costs ~40 VALU instructions (branches on |x|); in a GEMM write-out -- where the matrix pipe of that
// workgroup idles -- and in the fused decoder kernels that is the dominant cost (SAM's mlp.lin1: 168 M evaluations per
// block and group of images).  Here: erfc(t) = 2^(-t P(t)) on t = min(|x| / sqrt 2, 4) with a degree-7 minimax fit of P
// (|erf error| <= 1.0e-7 over the whole axis, the size of one float rounding of erf itself; one v_exp_f32, 8 fma); for x < 0
// 1 + erf(x) is erfc(|x|) itself, no subtraction.  |GELU error| <= 2.5e-7 max(1, |x|) (tests/test_gpu_primitives.py).
__device__ __forceinline__ float hgl_gelu_erf(float x) {
  const float t = fminf(fabsf(x) * 0.70710678118654752440f, 4.0f);
  float p = 4.582141628e-05f;
  p = fmaf(p, t, -4.491848231e-04f);
  p = fmaf(p, t, 1.500873244e-03f);
  p = fmaf(p, t, 7.568532601e-04f);
  p = fmaf(p, t, -2.823902667e-02f);
  p = fmaf(p, t, 1.484753788e-01f);
  p = fmaf(p, t, 9.184176326e-01f);
  p = fmaf(p, t, 1.627908468e+00f);
  float q = __builtin_amdgcn_exp2f(-(p * t));   // erfc(t)
  // beyond the clamp erfc(4) = 1.5e-8 would stay: on the negative side that is an error of 7.7e-9 |x| that grows without bound
  // (x = -1e4 -> -7.7e-5 where nn.GELU gives -0); erfc(t) < 2^-24 for t > 4, so 0 is the correctly rounded factor there
  q = fabsf(x) > 5.65685424949238f ? 0.f : q;
  return 0.5f * x * (x < 0.f ? q : 2.0f - q);
}
// QuickGELU (clip/model.py:198-200): x * sigmoid(1.702 x) with the hardware exponential and reciprocal (1 ulp each)
// instead of an IEEE division sequence
__device__ __forceinline__ float hgl_quick_gelu(float x) {
  return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.702f * 1.4426950408889634f * x));
}
#endif  // __HIPCC__ (device helpers: the host-only sources of the library include this header too)

unsigned long long hgl_split_overflow_gemm(int reset);
int hgl_split_overflow_gemm_peek(unsigned int* dst, hipStream_t st);
int hgl_split_overflow_attention_peek(unsigned int* dst, hipStream_t st);
unsigned long long hgl_split_overflow_attention(int reset);

void hgl_set_error(const char* fmt, ...);
int hgl_check_launch(const char* what);  // hipGetLastError -> HGL_ELAUNCH
int hgl_require_device();                // HGL_ENODEVICE when no GPU is visible

#define HGL_REQUIRE(cond, ...)          \
  do {                                  \
    if (!(cond)) {                      \
      hgl_set_error(__VA_ARGS__);       \
      return HGL_EINVAL;                \
    }                                   \
  } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the (function, device) pair: remembered per device at every call
// site, the result checked (a process that uses a second GPU would otherwise launch there with the default 64 KiB limit and
// fail in the launch).  KERNEL: a parenthesised function expression; use inside a function that returns an hgl status.
#define HGL_RESERVE_LDS(KERNEL, BYTES, WHAT)                                                                        \
  do {                                                                                                              \
    static std::atomic<bool> hgl_lds_set_[64];       /* zero-initialised; set after the attribute call returned */       \
    int hgl_dev_ = 0;                                                                                               \
    if (hipGetDevice(&hgl_dev_) != hipSuccess || hgl_dev_ < 0 || hgl_dev_ >= 64) hgl_dev_ = 0;                      \
    if (!hgl_lds_set_[hgl_dev_].load(std::memory_order_acquire)) {                                                  \
      if (hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(BYTES)) != hipSuccess) { \
        hgl_set_error("%s: cannot reserve %d bytes of LDS", WHAT, (int)(BYTES));                                    \
        return HGL_ELAUNCH;                                                                                         \
      }                                                                                                             \
      hgl_lds_set_[hgl_dev_].store(true, std::memory_order_release);                                                \
    }                                                                                                               \
  } while (0)

#define HGL_TRY(expr)            \
  do {                           \
    int _rc = (expr);            \
    if (_rc != HGL_OK) return _rc; \
  } while (0)

// ---- environment switches
// The product library reads exactly four HGL_* variables, each an A/B switch between two paths that give the same bits and
// each flipped by a -m gpu test (tests/test_abi.py checks the library's strings against this list):
//   HGL_ATTN_PP=0            long unmasked sequences on the tile kernel instead of the ping-pong kernel
//   HGL_X3_TERMS=3           the third split product kept for fp16-valued weights
//   HGL_SAM_POST_SEP=0       the per-pixel post-processing kernel instead of the shared-table one
//   HGL_ATTN_PS_CLIPBLOCKS   which CLIP residual blocks take the pre-split attention (0 never, 1 default, 2 also 197 tokens)
// Everything else that used to be an environment variable (tile-shape experiments, knock-outs for timing) exists only in the
// diagnostic twin `make diag` builds with -DHGL_DIAG (libhybridgl_diag.so, never loaded by the package): there
// HGL_DIAG_SWITCH reads the variable, here it IS its default and the compiler drops the other branch.
const char* hgl_env_str(const char* name);
int hgl_env_int(const char* name, int dflt);
#ifdef HGL_DIAG
#define HGL_DIAG_SWITCH(NAME, DFLT) hgl_env_int(NAME, DFLT)
#else
#define HGL_DIAG_SWITCH(NAME, DFLT) (DFLT)
#endif

static inline size_t hgl_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Bump allocator over the caller-provided workspace.
struct HglArena {
  char* base;
  size_t cap;
  size_t off;
  bool dry;  // size query: no base
  HglArena(void* b, size_t c) : base((char*)b), cap(c), off(0), dry(b == nullptr) {}
  template <typename T>
  T* take(size_t n) {
    size_t bytes = hgl_align_up(n * sizeof(T), 256);
    size_t o = off;
    off += bytes;
    if (dry) return nullptr;
    return (T*)(base + o);
  }
  bool ok() const { return dry || off <= cap; }
};

// ---- internal launchers (each returns HGL_*) -------------------------------
int hgl_launch_layernorm(const float* x, const float* w, const float* b, float* y, int rows, int D,
                         float eps, hipStream_t st);
// ---- GEMM: one call descriptor, one route, one launch (gemm_f16x3.hip; the fp32 tile kernel lives in gemm.hip) ----
// C = act(A @ W^T + bias) + R.  A caller says WHAT product it wants in named fields; hgl_gemm_route says WHICH kernel family
// serves it.
struct HglGemm {
  int M = 0, N = 0, K = 0, act = HGL_ACT_NONE;
  // A, one of two forms.  fp32 rows of lda floats, `batch` matrices sA apart ...
  const float* A = nullptr;
  int lda = 0, batch = 1;
  long long sA = 0;
  // ... or the fp16 hi | lo planes (lda in halfs; amap: row m is read from row amap[m])
  const void *Ah = nullptr, *Al = nullptr;
  const int* amap = nullptr;
  // the weight [N, K] as fp32 (rows of ldw floats, batch stride sW); the pointer is also the key of its registered fp16 split
  const float* W = nullptr;
  int ldw = 0;
  long long sW = 0;
  const float* bias = nullptr;
  // residual (may alias the output): rows of ldr floats, batch stride sR; rmod > 0: row m adds row m % rmod (a table shared
  // by every batch of rmod rows)
  const float* R = nullptr;
  int ldr = 0, rmod = 0;
  long long sR = 0;
  // output: fp32 C, or (C == nullptr, plane-form A) the fp16 hi | lo pair; rows of ldc, batch stride sC; cmap: output and
  // residual row m live at row cmap[m]
  float* C = nullptr;
  void *Ch = nullptr, *Cl = nullptr;
  int ldc = 0;
  long long sC = 0;
  const int* cmap = nullptr;
  // plane-form A: scratch for partial sums (16-byte aligned).  ksplit > 1: split-K in that many slices (needs ksplit * M * N
  // floats); ksplit 0 / 1: the launcher may cut the rows into whole rounds of the persistent tiling + a split-K tail
  float* part = nullptr;
  size_t part_bytes = 0;
  int ksplit = 0;
  // fp32 A with a registered weight in the split-fp16 modes: up to this many rows take the small-tile kernel
  int skinny_max_m = 1024;
};
// a dense nn.Linear on fp32 rows: C [M, N] = act(A [M, K] W^T + bias) (+ R, rows of N floats)
inline HglGemm hgl_gemm_linear(const float* A, const float* W, const float* bias, float* C, int M, int N, int K,
                               int act = HGL_ACT_NONE, const float* R = nullptr) {
  HglGemm d;
  d.M = M, d.N = N, d.K = K, d.act = act;
  d.A = A, d.lda = K, d.W = W, d.ldw = K, d.bias = bias;
  d.R = R, d.ldr = R ? N : 0, d.C = C, d.ldc = N;
  return d;
}
// the same with A as dense fp16 hi | lo planes (rows of K halfs) and a registered W
inline HglGemm hgl_gemm_planes(const void* Ah, const void* Al, const float* W, const float* bias, float* C, int M, int N, int K,
                               int act = HGL_ACT_NONE, const float* R = nullptr) {
  HglGemm d = hgl_gemm_linear(nullptr, W, bias, C, M, N, K, act, R);
  d.Ah = Ah, d.Al = Al;
  return d;
}
// planes in, planes out: the write-out splits (the next GEMM or the attention reads the pair)
inline HglGemm hgl_gemm_planes_split(const void* Ah, const void* Al, const float* W, const float* bias, void* Ch, void* Cl, int M,
                                     int N, int K, int act = HGL_ACT_NONE) {
  HglGemm d = hgl_gemm_planes(Ah, Al, W, bias, nullptr, M, N, K, act);
  d.Ch = Ch, d.Cl = Cl;
  return d;
}
// The kernel family that serves a descriptor.  A pure function of the descriptor, the precision state, the split-weight
// registry, hgl_gemm_f16x3_select and the switches; it enqueues nothing and sets no error.
enum HglGemmRoute {
  HGL_GEMM_NONE = 0,       // no kernel serves the descriptor (no operand; plane-form A without a registered weight)
  // fp32 A
  HGL_GEMM_F32,            // the fp32 MFMA tile kernel (gemm.hip)
  HGL_GEMM_SKINNY,         // split modes, registered weight, one batch of <= skinny_max_m rows: 32 x 32 tiles, K over four waves
  // A as fp16 hi | lo planes
  HGL_GEMM_X3_STAGED,      // register-staged 128 x 128 tiles: few tiles, any N / leading dimensions, planes of 4 GB and more
  HGL_GEMM_X3_PINGPONG,    // persistent 256 x 256 ping-pong tiles (planes of 4 GB and more: in row chunks, named by the first)
  HGL_GEMM_X3_BALANCED,    // ping-pong over the rows that fill whole rounds + split-K over the last row tiles
  HGL_GEMM_X3_SPLITK       // ksplit > 1: K slices of the ping-pong tiling + the reduce pass
};
HglGemmRoute hgl_gemm_route(const HglGemm& d);
// validates (the requirements of the family the route chose), looks the weight up once and launches; "no kernel serves the
// descriptor" is an error
int hgl_launch_gemm(const HglGemm& d, hipStream_t st);
// between gemm_f16x3.hip and gemm.hip only: the fp32 tile launch of a validated descriptor
int hgl_launch_gemm_f32_tiles(const HglGemm& d, hipStream_t st);
// the activation of an epilogue as a compile-time constant: f(std::integral_constant<int, HGL_ACT_*>{}) -> an hgl status
template <class F>
inline int hgl_with_act(int act, F&& f) {
  switch (act) {
    case HGL_ACT_QUICKGELU: return f(std::integral_constant<int, HGL_ACT_QUICKGELU>{});
    case HGL_ACT_GELU: return f(std::integral_constant<int, HGL_ACT_GELU>{});
    case HGL_ACT_RELU: return f(std::integral_constant<int, HGL_ACT_RELU>{});
    default: return f(std::integral_constant<int, HGL_ACT_NONE>{});
  }
}
// ---- attention: one call descriptor, one route, one launch (attention.hip; the plane-form kernels live in attention_ps.hip) ----
// A caller says WHAT attention it wants in named fields; hgl_attention_route says WHICH kernel family serves it.
struct HglAttn {
  int B = 0, H = 0, Sq = 0, Sk = 0, hd = 0;
  float scale = 1.0f;
  // operands, one of two forms.  fp32 q / k / v: rows of ldq / ldk / ldv floats, batch strides sqb / skb / svb ...
  const float *q = nullptr, *k = nullptr, *v = nullptr;
  int ldq = 0, ldk = 0, ldv = 0;
  long long sqb = 0, skb = 0, svb = 0;
  // ... or the fp16 hi | lo planes of a packed qkv (Sq == Sk): row (b * sb + s), columns qcol / kcol / vcol + head * hd, rows of
  // ld halfs
  const void *qkv_hi = nullptr, *qkv_lo = nullptr;
  int ld = 0, qcol = 0, kcol = 0, vcol = 0;
  long long sb = 0;
  // output: fp32 `out`, or (out == nullptr, split-fp16 modes) the fp16 hi | lo pair; rows of ldo, batch stride sob
  float* out = nullptr;
  void *out_hi = nullptr, *out_lo = nullptr;
  int ldo = 0;
  long long sob = 0;
  int mask_kind = HGL_MASK_NONE;
  const uint8_t* keep = nullptr;    // HGL_MASK_CLS_KEEP: keep bytes of batches keep_b0 .. keep_b0 + keep_n (keep_n 0: all B)
  int keep_b0 = 0, keep_n = 0;
  // decomposed rel-pos bias: the terms as tensors [B*H, Sq, kh] / [B*H, Sq, kw] ...
  const float *rel_h = nullptr, *rel_w = nullptr;
  int kh = 0, kw = 0;
  // ... or the windowed blocks' tables [27, 80] (14 x 14 windows at head dim 80: the kernel computes the terms itself)
  const float *tab_h = nullptr, *tab_w = nullptr;
  // part != nullptr: the chunked few-query form (the decoder's token -> image attention).  part: scratch of at least
  // hgl_attention_fewq_part_bytes(B, Sk) bytes; kv_group > 1: batches b of one group share the keys / values of set b / kv_group
  float* part = nullptr;
  size_t part_bytes = 0;
  int kv_group = 1;
};
// the packed [B, S, 3D] qkv of a transformer block (q | k | v at columns 0, D, 2D; D = H * hd) as fp32, scale 1 / sqrt(hd),
// output rows of D floats.  The caller names the output (out, or out_hi / out_lo) and what else differs.
inline HglAttn hgl_attn_packed(const float* qkv, int B, int H, int S, int hd) {
  const int D = H * hd;
  HglAttn d;
  d.B = B, d.H = H, d.Sq = S, d.Sk = S, d.hd = hd, d.scale = 1.0f / sqrtf((float)hd);
  d.q = qkv, d.k = qkv + D, d.v = qkv + 2 * D;
  d.ldq = d.ldk = d.ldv = 3 * D;
  d.sqb = d.skb = d.svb = (long long)S * 3 * D;
  d.ldo = D, d.sob = (long long)S * D;
  return d;
}
// the same tensor as the fp16 hi | lo planes the in-projection's write-out emits
inline HglAttn hgl_attn_packed_planes(const void* hi, const void* lo, int B, int H, int S, int hd) {
  const int D = H * hd;
  HglAttn d;
  d.B = B, d.H = H, d.Sq = S, d.Sk = S, d.hd = hd, d.scale = 1.0f / sqrtf((float)hd);
  d.qkv_hi = hi, d.qkv_lo = lo;
  d.ld = 3 * D, d.qcol = 0, d.kcol = D, d.vcol = 2 * D, d.sb = S;
  d.ldo = D, d.sob = (long long)S * D;
  return d;
}
// The kernel family that serves a descriptor.  A pure function of the descriptor, the precision state (hgl_split_layout(),
// hgl_split_terms()), the split-weight registry (the windowed tables) and the switches; it enqueues nothing and sets no error.
enum HglAttnRoute {
  HGL_ATTN_NONE = 0,       // no kernel serves the descriptor
  // fp32 q / k / v (attention.hip)
  HGL_ATTN_FEWQ_CHUNKED,   // `part` given: 8 heads of 16, up to 7 queries, keys in chunks of 256
  HGL_ATTN_WIN14,          // tables given: 14 x 14 windows at head dim 80, the rel-pos terms computed in the kernel
  HGL_ATTN_FEWQ,           // head dim 16, up to 8 queries over >= 1024 keys
  HGL_ATTN_SMALLK,         // head dim 16, up to 8 keys
  HGL_ATTN_F32,            // fp32 mode: the fp32 tile kernel
  HGL_ATTN_PINGPONG,       // long unmasked sequences: one 8-wave workgroup per 256 queries
  HGL_ATTN_REL14,          // head dim 80, 14 x 14 rel-pos terms as tensors
  HGL_ATTN_DUAL,           // head dim 64, 129..256 queries: one 4-wave workgroup per item, two query tiles per wave
  HGL_ATTN_WIDE,           // 129..256 queries: one 8-wave workgroup per item
  HGL_ATTN_TILE,           // one 4-wave workgroup per 128 queries
  // q | k | v as fp16 hi | lo planes (attention_ps.hip)
  HGL_ATTN_PS_WIN,         // 14 x 14 windows at head dim 80, the registered tables
  HGL_ATTN_PS_RELT,        // rel-pos terms as tensors
  HGL_ATTN_PS_CLIP,        // head dim 64, 129..256 tokens: the un-pipelined kernel, two query tiles per wave
  HGL_ATTN_PS_PLAIN        // the pipelined persistent kernel
};
HglAttnRoute hgl_attention_route(const HglAttn& d);
// validates (the requirements of the family the route chose) and launches; "no kernel serves the descriptor" is an error
int hgl_launch_attention(const HglAttn& d, hipStream_t st);
size_t hgl_attention_fewq_part_bytes(int B, int Sk);
// between attention.hip and attention_ps.hip only: the plane-form half of the route and of the launch, and the ONE lookup of the
// windowed blocks' tables in the split-weight registry (both [27, 80], registered at scale 2^0: the halves the kernels' own
// split gives, bit for bit; t = h hi, h lo, w hi, w lo)
bool hgl_attention_rel_tables(const float* tab_h, const float* tab_w, const void* t[4]);
HglAttnRoute hgl_attention_route_planes(const HglAttn& d);
int hgl_launch_attention_planes(const HglAttn& d, HglAttnRoute route, hipStream_t st);

// CLIP glue (clip_glue.hip)
int hgl_launch_im2col_patch(const float* img, int N, int res, int patch, float* cols, hipStream_t st);
int hgl_launch_im2col_patch_split(const float* img, int N, int res, int patch, void* hi, void* lo, hipStream_t st);
int hgl_launch_assemble_lnpre(const float* tok, const float* cls, const float* pos, const float* lw,
                              const float* lb, float* x, int B, int S, int D, hipStream_t st);
int hgl_launch_mask_resize(const uint8_t* masks, int N, int Hm, int Wm, int g, float* pm,
                           uint8_t* keep, hipStream_t st);
// out[n,s,:] = a[n,s,:]*ca + cb * b[n,s,:] * (s==0 ? 1 : pm[n,s-1]) ; pm may be null, a may be null
int hgl_launch_mix(float* out, const float* a, float ca, const float* b, float cb, const float* pm,
                   int N, int S, int D, hipStream_t st);
int hgl_launch_gather_rows(const float* x, long long row_stride, int rows, int D, float* y,
                           hipStream_t st);
int hgl_launch_add_inplace(float* y, const float* x, long long n, hipStream_t st);
int hgl_launch_text_embed(const int32_t* tokens, const float* emb, const float* pos, float* x, int B,
                          int S, int ctx, int D, int vocab, int32_t* eot, hipStream_t st);
int hgl_launch_gather_eot(const float* x, const int32_t* eot, int B, int S, int D, float* y,
                          hipStream_t st);
int hgl_launch_zero_positions(float* x, int B, int S, int D, const int32_t* pos, int n, hipStream_t st);

// CLIP transformer pieces shared by clip_api.hip and gem_api.hip
struct HglBlockBufs {
  float* H;    // [M, D]   LN output / attention output
  float* QKV;  // [M, 3D]
  float* F;    // [M, 4D]
};
// Everything that is decided about the launches of one residual block, once per block call
struct HglClipBlockRoute {
  bool x3;       // the split-fp16 path: every GEMM operand activation exists only as fp16 hi | lo planes
  bool planes;   // the in-projection writes q | k | v as planes and the attention runs on them (attention_ps.hip)
  int ks;        // split-K factor of mlp.c_proj (1: the row-balanced launch)
};
// what the caller runs of the block: all of it (planes where the route serves them); all of it, reading q | k | v as fp32
// after the in-projection (GEM's self-self attention: no planes); or the in-projection alone (the CLS-row block, GEM without
// its original stream: no planes, and mlp.c_proj is not the block's: ks stays 1)
enum HglClipBlockUse { HGL_BLOCK_WHOLE, HGL_BLOCK_FP32_QKV, HGL_BLOCK_QKV_ONLY };
HglClipBlockRoute hgl_clip_block_route(const HglResBlockW& w, const HglBlockBufs& bf, int B, int S, int D, int heads, int mask_kind,
                                       HglClipBlockUse use);
int hgl_clip_run_block(const HglResBlockW& w, float* X, int B, int S, int D, int heads, const HglBlockBufs& bf,
                       int mask_kind, const uint8_t* keep, int keep_b0, int keep_n, hipStream_t st);
int hgl_clip_block_qkv(const HglResBlockW& w, const HglClipBlockRoute& r, const float* X, int M, int D, const HglBlockBufs& bf,
                       hipStream_t st);
int hgl_clip_block_rest(const HglResBlockW& w, const HglClipBlockRoute& r, float* X, int B, int S, int D, int heads,
                        const HglBlockBufs& bf, int mask_kind, const uint8_t* keep, int keep_b0, int keep_n, hipStream_t st);
int hgl_clip_embed_images(const HglClipVisionW* w, const float* imgs, int n_img, float* X, float* cols, float* tok,
                          hipStream_t st);
bool hgl_valid_vision(const HglClipVisionW* w);

// ---- optional per-kernel-class timing with HIP events on the launch stream (bench roofline) ----
enum HglProfClass { HGL_PROF_GEMM = 0, HGL_PROF_ATTN = 1, HGL_PROF_OTHER = 2, HGL_PROF_GEMM_X3 = 3, HGL_PROF_GEMM_X3G = 4, HGL_PROF_GEMM_X3_FEW = 5, HGL_PROF_NCLASS = 6 };
struct HglProfScope {
  int slot;
  hipStream_t st;
  HglProfScope(int cls, double flops, double bytes, hipStream_t s);
  ~HglProfScope();
};

// SAM glue (sam_glue.hip)
int hgl_launch_sam_preprocess(const uint8_t* img, int h, int w, int S, float* out, hipStream_t st);
int hgl_launch_win_partition(const float* H, int g, int ws, int nw, int D, float* Hw, hipStream_t st);
int hgl_launch_win_unpartition_add(float* X, int g, int ws, int nw, int D, const float* P, hipStream_t st);
int hgl_launch_relpos_gather(const float* T, int B, int heads, int S, int size, int L, int use_w,
                             float* rel, hipStream_t st);
int hgl_launch_relpos_direct(const float* qkv, int ldq, int B, int heads, int S, int size, int hd,
                             const float* Rh, const float* Rw, float* rel_h, float* rel_w, hipStream_t st);
int hgl_launch_relpos_split(const void* q_hi, const void* q_lo, int ldq, int B, int heads, int S, int size, int hd,
                            const float* Rh, const float* Rw, float* rel_h, float* rel_w, hipStream_t st);
int hgl_launch_im2col3x3(const float* in, int g, int C, float* cols, hipStream_t st);
int hgl_launch_add_rows_bcast(const float* a, long long a_bstride, const float* pe, long long rows_elems,
                              int B, float* out, hipStream_t st);
int hgl_launch_pe(const float* coords01, const float* G, int n, int F, int mode, const float* pos_embed,
                  const float* not_a_point, float* out, hipStream_t st);
int hgl_launch_build_tokens(const float* iou_tok, const float* mask_tok, const float* sparse, int P, int C, int T,
                            float* tokens, hipStream_t st);
int hgl_launch_mask_downscaling(const float* in, int P, int g, const float* c1w, const float* c1b, const float* n1w, const float* n1b,
                                const float* c2w, const float* c2b, const float* n2w, const float* n2b, const float* c3w,
                                const float* c3b, float* out, hipStream_t st);
int hgl_launch_win_maps(int g, int ws, int nw, int nb, int* pad_of, int* tok_of, int* pad_list, int* pad_count, hipStream_t st);
int hgl_launch_fill_rows(float* dst, int ld, const int* rows, const int* nrows, int max_rows, const float* v, int N,
                         hipStream_t st);
int hgl_launch_fill_rows_split(void* hi, void* lo, int ld, const int* rows, const int* nrows, int max_rows, const float* v,
                               int N, hipStream_t st);
int hgl_launch_ln_gelu64(float* x, const float* w, const float* b, long long rows, float eps, void* hi, void* lo,
                         hipStream_t st);
int hgl_launch_ln256_pe_split(float* x, const float* w, const float* b, const float* pe, int pe_rows, long long rows,
                              float eps, int write_f32, void* kh, void* kl, void* ph, void* pl, hipStream_t st);
int hgl_launch_hyper_logits(const float* u2, const float* hyper, int P, int g, int row0, float* low_res, hipStream_t st);
int hgl_launch_pe_labeled(const float* coords01, const int32_t* labels, const float* G, int n, int F, const float* not_a_point,
                          const float* const* point_embed, float* out, hipStream_t st);
// fused decoder stages (sam_decoder_fused.hip)
// token -> image attention of the mask decoder on the raw image-token planes (sam_decoder_t2i.hip)
int hgl_launch_t2i_fold_q(const float* q1, const float* Wk, float scale, float* Qk, int P, hipStream_t st);
// ns = hgl_t2i_key_ranges(P, HW): 1 -> out = the attended rows [P*56, 256]; 8 (prompt batches of <= 128) -> out = key-range partials
// of hgl_t2i_part_bytes(P, HW) bytes, which hgl_launch_t2i_unfold_v (same ns) puts together
int hgl_t2i_key_ranges(int P, int HW);
size_t hgl_t2i_part_bytes(int P, int HW);
int hgl_launch_t2i_raw_attn(const void* Qh, const void* Ql, const float* bias, const void* Kh, const void* Kl, int P, int HW,
                            float* out, int ns, hipStream_t st);
int hgl_launch_i2t_prep(const float* k1, const float* v1, const float* Wq, const float* bq, const float* Wo, float scale, void* Kh,
                        void* Kl, float* cb, void* Uh, void* Ul, int P, hipStream_t st);
unsigned long long hgl_split_overflow_decoder(int reset);
int hgl_split_overflow_decoder_peek(unsigned int* dst, hipStream_t st);
int hgl_launch_dec_i2t_fold(const void* Xh, const void* Xl, const void* Kh, const void* Kl, const float* pek, const float* cb,
                            const void* Uh, const void* Ul, const float* bo, const float* ln_w, const float* ln_b, float eps, int P,
                            int HW, void* out_hi, void* out_lo, hipStream_t st);
int hgl_launch_t2i_unfold_v(const float* A, int ns, const float* Wv, const float* bv, float* att, int P, hipStream_t st);
int hgl_launch_dec_tail(const void* src_hi, const void* src_lo, const float* up0_w, const float* up0_b, const float* ln_w,
                        const float* ln_b, const float* up3_w, const float* up3_b, const float* hyper, int row0, int P, int g,
                        float eps, float* low_res, const uint8_t* skip, hipStream_t st);
int hgl_launch_dec_i2t(const float* q, int ldq, long long q_bstride, const float* k1, const float* v1, const float* out_w,
                       const float* out_b, const float* R, long long r_bstride, const float* ln_w, const float* ln_b, float eps,
                       float scale, int P, int HW, float* out32, void* out_hi, void* out_lo, hipStream_t st,
                       int per_set = 1);   // > 1: prompts p of one set share the queries / residual rows of set p / per_set

// split-fp16 GEMM path (gemm_f16x3.hip)
int hgl_precision();
// the fp16 hi | lo plane layout is in use (HGL_PREC_F16X3 and HGL_PREC_F16): split weights registered, split producers and
// consumers on the encoder path
bool hgl_split_layout();
// products per split-operand product: 3 (f16x3: lo*hi + hi*lo + hi*hi) or 1 (f16: hi*hi; no lo plane is written or read).
// HglSplitTermsScope pins 3 for the host code in its scope (the SAM decoder keeps its f16x3 arithmetic in f16 mode).
int hgl_split_terms();
struct HglSplitTermsScope {
  explicit HglSplitTermsScope(int terms);
  ~HglSplitTermsScope();
  int prev;
};
bool hgl_has_split_weight(const float* W);
bool hgl_get_split_weight(const float* W, const void** hi, const void** lo, int* scale_log2, int* N, int* K);
int hgl_launch_split_f16(const float* x, float scale, void* hi, void* lo, long long n, hipStream_t st);
int hgl_launch_layernorm_split(const float* x, const float* w, const float* b, void* hi, void* lo, int rows, int D,
                               float eps, hipStream_t st);
int hgl_launch_layernorm_split_maps(const float* x, const float* w, const float* b, void* hi, void* lo, int rows, int D,
                                    float eps, const int* smap, const int* dmap, hipStream_t st);
int hgl_gemm_f16x3_splitk_factor(int M, int N, int K);
int hgl_launch_win_partition_split(const float* H, int g, int ws, int nw, int D, void* hi, void* lo, hipStream_t st);
// true when the split-fp16 path applies to a GEMM with this weight and reduction length
static inline bool hgl_use_x3(const float* W, int K) { return hgl_split_layout() && (K % 64) == 0 && hgl_has_split_weight(W); }

// ---- the activation operand of the encoder blocks -----------------------------------------------------------------------
// What a block step reads or writes: the fp32 rows of a scratch buffer, or -- the split-fp16 modes -- the fp16 hi | lo planes
// that alias the same bytes (hi at the buffer's start, lo `elems` halfs behind it).  Exactly one form is set.  A block is
// written ONCE over operands; its route (HglClipBlockRoute, EncBlockRoute in sam_api.hip) says which form each operand has and
// what else differs.  (f16 mode: lo is still named; the launchers that take a null lo plane get it at their call site.)
struct HglAct {
  float* f32 = nullptr;
  uint16_t *hi = nullptr, *lo = nullptr;
};
inline HglAct hgl_act(float* buf, size_t elems, bool split) {
  HglAct a;
  if (split) a.hi = (uint16_t*)buf, a.lo = a.hi + elems;
  else a.f32 = buf;
  return a;
}
// y = LayerNorm(x) into an operand
inline int hgl_launch_layernorm_act(const float* x, const float* w, const float* b, const HglAct& y, int rows, int D, float eps,
                                    hipStream_t st) {
  return y.hi ? hgl_launch_layernorm_split(x, w, b, y.hi, y.lo, rows, D, eps, st) : hgl_launch_layernorm(x, w, b, y.f32, rows, D, eps, st);
}
// the im2col matrix of a patch embedding into an operand
inline int hgl_launch_im2col_patch_act(const float* img, int N, int res, int patch, const HglAct& cols, hipStream_t st) {
  return cols.hi ? hgl_launch_im2col_patch_split(img, N, res, patch, cols.hi, cols.lo, st) : hgl_launch_im2col_patch(img, N, res, patch, cols.f32, st);
}
// a dense nn.Linear from an operand to fp32 C: hgl_gemm_planes or hgl_gemm_linear ...
inline HglGemm hgl_gemm_act(const HglAct& A, const float* W, const float* bias, float* C, int M, int N, int K, int act = HGL_ACT_NONE,
                            const float* R = nullptr) {
  return A.hi ? hgl_gemm_planes(A.hi, A.lo, W, bias, C, M, N, K, act, R) : hgl_gemm_linear(A.f32, W, bias, C, M, N, K, act, R);
}
// ... and to an operand: planes out (hgl_gemm_planes_split; the input is then planes as well), or the above on C.f32
inline HglGemm hgl_gemm_act(const HglAct& A, const float* W, const float* bias, const HglAct& C, int M, int N, int K,
                            int act = HGL_ACT_NONE) {
  HglGemm d = hgl_gemm_act(A, W, bias, C.f32, M, N, K, act);
  d.Ch = C.hi, d.Cl = C.lo;
  return d;
}
// The MLP half of a transformer block, x <- x + proj(act(fc(ln(x)))) on M rows of D floats, through the operands H [M, D] and
// F [M, 4D].  part / part_bytes: scratch for the partial sums of proj; ks: its split-K factor (HglGemm::ksplit: 0 / 1 leave the
// cut to the launcher) -- both decided by the caller's route; the fp32 form of proj reads neither.
struct HglMlp {
  const float *ln_w, *ln_b, *fc_w, *fc_b, *proj_w, *proj_b;
  float eps;
  int act;
};
inline int hgl_mlp_half(const HglMlp& w, float* X, const HglAct& H, const HglAct& F, int M, int D, float* part, size_t part_bytes,
                        int ks, hipStream_t st) {
  HGL_TRY(hgl_launch_layernorm_act(X, w.ln_w, w.ln_b, H, M, D, w.eps, st));
  HGL_TRY(hgl_launch_gemm(hgl_gemm_act(H, w.fc_w, w.fc_b, F, M, 4 * D, D, w.act), st));
  HglGemm proj = hgl_gemm_act(F, w.proj_w, w.proj_b, X, M, D, 4 * D, HGL_ACT_NONE, X);
  proj.part = part, proj.part_bytes = part_bytes, proj.ksplit = ks;
  return hgl_launch_gemm(proj, st);
}
// A linear on fp32 values whose weight may have a registered split.  d: the GEMM on the fp32 rows d.A (lda == K), n values in
// all.  split: produce(a) writes the values as the fp16 hi | lo planes a into the dead buffer `scratch` and the GEMM reads those
// (hgl_gemm_planes); else produce(a) writes them to a.f32 == d.A -- or finds them there -- and d runs as it is.
template <class Produce>
inline int hgl_linear_split_or_not(HglGemm d, bool split, float* scratch, size_t n, Produce&& produce, hipStream_t st) {
  const HglAct a = hgl_act(split ? scratch : const_cast<float*>(d.A), n, split);
  HGL_TRY(produce(a));
  if (split) d.A = nullptr, d.Ah = a.hi, d.Al = a.lo;
  return hgl_launch_gemm(d, st);
}
// the same where the values exist as the fp32 rows d.A: the split producer is hgl_launch_split_f16
inline int hgl_linear_split_or_not(const HglGemm& d, bool split, float* scratch, size_t n, hipStream_t st) {
  const float* x = d.A;
  return hgl_linear_split_or_not(
      d, split, scratch, n, [=](const HglAct& a) { return a.hi ? hgl_launch_split_f16(x, 1.0f, a.hi, a.lo, (long long)n, st) : HGL_OK; }, st);
}
// a device-to-device copy on the stream, checked: `what` names the call and the copy in the error
inline int hgl_copy_d2d(void* dst, const void* src, size_t bytes, const char* what, hipStream_t st) {
  if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    hgl_set_error("%s failed", what);
    return HGL_ELAUNCH;
  }
  return HGL_OK;
}
