// The steps of one (query tile, key tile) pair of the split-fp16 MFMA attention kernels, each ONCE: attn_x3_kernel,
// attn_x3pp_kernel, attn_x3q_kernel (attention.hip) and attn_ps_kernel (attention_ps.hip) are different schedules -- staging,
// barriers, ping-pong groups, LDS-DMA -- around these calls, which is why their results are bit-identical on the same
// operands.  attn_psp_kernel interleaves its soft-max with the next tile's QK^T chain by hand and keeps that segment and its
// permlane32 write-out (the two second copies, marked below); it takes the tile map, the masks, QK^T of its first tile, the
// transposing read and the P V products from here.
//
// Layout shared by all of them (swapped QK^T): a wave owns 32 queries, lane (r, h) = (lane & 31, lane >> 5) owns query r;
// score register e of a 32-key tile is key (e & 3) + 8 * (e >> 2) + 4 * h; lanes l and l ^ 32 hold the two key halves.
// Form matters here: scalars and pointers by value, register arrays by reference, address arithmetic inside the branch
// that uses it -- so that a kernel compiles to what its own copy of the step compiled to.
#pragma once
#include "hgl_common.h"

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef __fp16 fp16x4v __attribute__((__vector_size__(4 * sizeof(__fp16))));

constexpr int NEG_BIG_BITS = 0xff800000;  // -inf

__device__ __forceinline__ void split4(const f32x4 v, h16x4& hi, h16x4& lo, float& amax) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    _Float16 a, c;
    hgl_split_hi_lo(v[e], a, c, amax);
    hi[e] = a;
    lo[e] = c;
  }
}

// ds_read_b64_tr_b16 (EXEC must be all ones at the call): a 16-lane group fetches a 4-row x 16-column block of halfs and each
// lane receives its column of the 4 rows
__device__ __forceinline__ h16x4 attn_tr4(const _Float16* p) {
  typedef __attribute__((address_space(3))) fp16x4v lds_v;
  const fp16x4v v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_v*)p);
  h16x4 r;
  __builtin_memcpy(&r, &v, 8);
  return r;
}
// transposed-read addressing of a V tile with row pitch VP halfs: lane = 16*grp + 4*q + p supplies row q, columns 4p..4p+3 of
// its group's block; groups 0/1 carry d columns 0-15 / 16-31 for h = 0, groups 2/3 the same for h = 1
template <int VP>
__device__ __forceinline__ int attn_tr_off(const int lane, const int h) {
  return (((lane >> 2) & 3) + 4 * h) * VP + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
}

// XCD-aware tile map: work units go to the eight XCDs round-robin in linear order.  Unit L -> (item, slot) so that XCD
// c = L & 7 works through the items c, c + 8, ... and the G consecutive slots of an XCD belong to ONE item (the query blocks
// of a head, which stream the same keys and values: one L2 fetches them).  The caller decides when the map applies.
__device__ __forceinline__ void attn_xcd_item(const unsigned L, const unsigned G, int& item, int& bx) {
  const unsigned c = L & 7u, j = L >> 3;
  const unsigned jg = j / G;
  bx = (int)(j - jg * G);
  item = (int)(jg * 8u + c);
}

// Q fragments from fp32 rows: lane (r, h) element j of k-step s = Q[q][16s + 8h + j] as the fp16 hi / lo pair.  ALL raw
// pieces are requested before the first one is split (hgl_split_hi_lo's opaque asm keeps a load from moving across it: one
// round trip per piece otherwise); qp points at a valid row also when !qvalid (no branch around the loads), whose fragments
// are then zero.  PRESCALE: q is multiplied by `scale` before the split (attn_x3q_kernel; the others keep the scale in the
// exponent's constant and feed the unscaled fragments to the rel-pos products as well).
template <int KS, int TERMS, bool PRESCALE>
__device__ __forceinline__ void attn_load_split_q(const float* qp, const int h, const bool qvalid, const float scale,
                                                  h16x8 (&qh)[KS], h16x8 (&ql)[KS], float& amax) {
  f32x4 qraw[KS][2];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int half = 0; half < 2; ++half)
      qraw[s][half] = *(const f32x4*)(qp + 16 * s + 8 * h + 4 * half);
  __builtin_amdgcn_sched_barrier(0);
  if (!qvalid) {
#pragma unroll
    for (int s = 0; s < KS; ++s) qraw[s][0] = qraw[s][1] = f32x4{0, 0, 0, 0};
  }
#pragma unroll
  for (int s = 0; s < KS; ++s) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const f32x4 v = qraw[s][half];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        _Float16 hi, lo;
        hgl_split_hi_lo(PRESCALE ? v[e] * scale : v[e], hi, lo, amax);
        qh[s][4 * half + e] = hi;
        if constexpr (TERMS != 1) ql[s][4 * half + e] = lo;
      }
    }
  }
}

// S^T += K Q^T of a 32-key tile: krow = the lane's staged key row [hi (HD) | lo (HD) | ...] + 8 * h.  Three products per
// k-step, small terms first (lo*hi, hi*lo, hi*hi); TERMS == 1: hi*hi only.
template <int HD, int TERMS>
__device__ __forceinline__ void attn_qk_tile(const _Float16* krow, const h16x8 (&qh)[HD / 16], const h16x8 (&ql)[HD / 16], f32x16& s) {
#pragma unroll
  for (int c = 0; c < HD / 16; ++c) {
    const h16x8 kh8 = *(const h16x8*)(krow + 16 * c);
    const h16x8 kl8 = *(const h16x8*)(krow + HD + 16 * c);
    if constexpr (TERMS != 1) {
      s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl8, qh[c], s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh8, ql[c], s, 0, 0, 0);
    }
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh8, qh[c], s, 0, 0, 0);
  }
}

// the tile that crosses the end of the sequence (uniform): keys >= Sk get -inf
__device__ __forceinline__ void attn_mask_tail(f32x16& s, const int kbase, const int Sk, const int h) {
  if (kbase + 32 > Sk) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int kg = kbase + (e & 3) + 8 * (e >> 2) + 4 * h;
      s[e] = kg >= Sk ? __int_as_float(NEG_BIG_BITS) : s[e];
    }
  }
}

// CLS-keep mask (make_attn_mask: only query 0 is restricted) of the tile that owns query 0 -- the caller's uniform condition:
// keepL[key - 1] != 0 keeps the key; the 32 keys' flags are gathered by one ballot.  qi: this lane's query.
__device__ __forceinline__ void attn_mask_cls_keep(f32x16& s, const uint8_t* keepL, const int kbase, const int Sk, const int lane,
                                                   const int h, const int qi) {
  const int kk = kbase + (lane & 31);
  const unsigned kb = kk >= 1 && kk < Sk ? keepL[kk - 1] : 1u;
  const unsigned bits = (unsigned)__builtin_amdgcn_ballot_w64(kb != 0) >> (4 * h);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const bool kept = (bits >> ((e & 3) + 8 * (e >> 2))) & 1u;
    s[e] = (qi == 0 && !kept) ? __int_as_float(NEG_BIG_BITS) : s[e];
  }
}

// the lane's maximum of its 16 scores (attn_x3_kernel folds this into its per-element mask loop where it masks)
__device__ __forceinline__ float attn_tile_max(const f32x16 s) {
  float mx = __int_as_float(NEG_BIG_BITS);
#pragma unroll
  for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[e]);
  return mx;
}

// Online soft-max of a tile.  mx: the lane's maximum of s.  exp(x - m) = exp2(fma(s, sl2e, -m * sl2e)): the scores are in
// units of 1 / sl2e log2 (sl2e = scale * log2 e for unscaled q . k, log2 e for pre-scaled q).
// Lazy rescaling: the running maximum follows the scores only when some query of the wave would otherwise see probabilities
// above 2^8 (rescale_thr = 5.5 nats in the scores' units; uniform branch).  Until then alpha == 1 and the 16 * DT multiplies
// of O are skipped; p <= 256 keeps its full relative precision in fp32 and in the fp16 hi + lo pair.
// P: hi by one packed round-toward-zero conversion (any rounding works: lo is the exact remainder, rounded to nearest);
// TERMS == 1: hi only, rounded to nearest.
// SECOND COPY: attn_psp_kernel's segment A (attention_ps.hip, valu_g) spells the same operations out as 19 groups between
// the next tile's matrix instructions, with the half exchange by v_permlane32_swap -- a different instruction order on purpose.
// A change of the threshold, the rescaling or the P rounding here has to be made there as well.
template <int DT, int TERMS>
__device__ __forceinline__ void attn_softmax_tile(const f32x16 s, float mx, const float sl2e, const float rescale_thr, float& m_run,
                                                  float& l_run, f32x16 (&o)[DT], h16x8 (&ph)[2], h16x8 (&pl)[2]) {
  const float NEG_INF = __int_as_float(NEG_BIG_BITS);
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  const float m_cand = fmaxf(m_run, mx);
  float m_new = m_run;
  if (__builtin_amdgcn_ballot_w64(m_cand > m_run + rescale_thr)) {
    m_new = m_cand;
    const float m_use0 = (m_new == NEG_INF) ? 0.f : m_new;   // all keys so far masked: keep everything at zero
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_use0) * sl2e);
    l_run *= alpha;
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[d][e] *= alpha;
    m_run = m_new;
  }
  const float mneg = -((m_new == NEG_INF) ? 0.f : m_new) * sl2e;
  float rs = 0.f;
#pragma unroll
  for (int e = 0; e < 16; e += 2) {
    const float p0 = __builtin_amdgcn_exp2f(fmaf(s[e], sl2e, mneg));
    const float p1 = __builtin_amdgcn_exp2f(fmaf(s[e + 1], sl2e, mneg));
    rs += p0;
    rs += p1;
    if constexpr (TERMS == 1) {
      ph[e >> 3][e & 7] = (_Float16)p0; ph[e >> 3][(e & 7) + 1] = (_Float16)p1;
    } else {
      const h16x2 hi2 = __builtin_bit_cast(h16x2, __builtin_amdgcn_cvt_pkrtz(p0, p1));
      ph[e >> 3][e & 7] = hi2[0]; ph[e >> 3][(e & 7) + 1] = hi2[1];
      pl[e >> 3][e & 7] = (_Float16)(p0 - (float)hi2[0]);
      pl[e >> 3][(e & 7) + 1] = (_Float16)(p1 - (float)hi2[1]);
    }
  }
  l_run += rs;
}

// O^T += V^T P^T of a tile: the P^T registers 8 s2 .. 8 s2 + 7 are the B operand of k-step s2 (keys 16 s2 + 8 (j >> 2) + 4 h
// + (j & 3)); the A operand is two transposing reads of four consecutive keys from the row-major V planes (pitch VP halfs).
// off = the tile's first row * VP + attn_tr_off.  A k-step whose keys all lie at or beyond sk_end is skipped (uniform; P = 0).
template <int DT, int VP, int TERMS>
__device__ __forceinline__ void attn_pv_tile(const _Float16* Vh, const _Float16* Vl, const int off0, const int kbase, const int sk_end,
                                             const h16x8 (&ph)[2], const h16x8 (&pl)[2], f32x16 (&o)[DT]) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    if (kbase + 16 * s2 >= sk_end) break;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      const int off = off0 + (16 * s2) * VP + d * 32;
      const h16x4 vh0 = attn_tr4(Vh + off), vh1 = attn_tr4(Vh + off + 8 * VP);
      const h16x4 vl0 = attn_tr4(Vl + off), vl1 = attn_tr4(Vl + off + 8 * VP);
      h16x8 vh8, vl8;
#pragma unroll
      for (int e = 0; e < 4; ++e) { vh8[e] = vh0[e]; vh8[4 + e] = vh1[e]; vl8[e] = vl0[e]; vl8[4 + e] = vl1[e]; }
      if constexpr (TERMS != 1) {
        o[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl8, ph[s2], o[d], 0, 0, 0);
        o[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh8, pl[s2], o[d], 0, 0, 0);
      }
      o[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh8, ph[s2], o[d], 0, 0, 0);
    }
  }
}

// Write-out of a query tile: the two key halves' sums, 1 / l, then the lane's four consecutive d of accumulator group g as
// fp32 (out != nullptr) or as the fp16 hi / lo pair, the operand form of the following f16x3 projection (out_lo may be
// absent).  The row's address is formed inside the branch of the lanes that store.
// SECOND COPY: attn_psp_kernel normalises and splits the same way but pairs the two lanes of a row through v_permlane32_swap
// into 16-byte stores (attention_ps.hip, its write-out: 148 of the windowed launch's 768 us went into 8-byte stores).
template <int HD, int DT>
__device__ __forceinline__ void attn_write_out(const f32x16 (&o)[DT], const float l_run, const bool qvalid, float* out, _Float16* out_hi,
                                               _Float16* out_lo, const int b, const long long sob, const int qi, const int ldo,
                                               const int hh, const int h) {
  const float l_tot = l_run + __shfl_xor(l_run, 32);
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
  if (qvalid) {
    const long long oo = b * sob + (long long)qi * ldo + hh * HD;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dd = d * 32 + 8 * g + 4 * h;
        if (dd < HD) {
          f32x4 w;
#pragma unroll
          for (int e = 0; e < 4; ++e) w[e] = o[d][4 * g + e] * inv;
          if (out) {
            *(f32x4*)(out + oo + dd) = w;
          } else {
            h16x4 hi, lo;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              _Float16 a2, c2;
              hgl_split_hi_lo(w[e], a2, c2);
              hi[e] = a2;
              lo[e] = c2;
            }
            *(h16x4*)(out_hi + oo + dd) = hi;
            if (out_lo) *(h16x4*)(out_lo + oo + dd) = lo;
          }
        }
      }
    }
  }
}
