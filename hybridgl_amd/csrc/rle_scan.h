// Device pieces that the RLE kernels of rle.hip and rle_poly.hip share: one copy of each decision.  Workgroups of RLE_THREADS =
// 256 threads = 4 waves throughout.
#ifndef HGL_RLE_SCAN_H
#define HGL_RLE_SCAN_H
#include "hgl_common.h"

namespace {

constexpr int RLE_THREADS = 256;

// the workgroup-wide sum of v; lds: 4 elements
template <typename T>
__device__ __forceinline__ T rle_block_sum(T v, T* lds) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();      // the previous use of lds is over
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

// the last g with v[g] <= key (v non-decreasing, v[0] <= key): the image that owns entry / tile `key`; images without entries
// share their successor's value and are passed over
template <typename T>
__device__ __forceinline__ int rle_group_find(const T* v, int G, T key) {
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (v[mid] <= key) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// One chunk of the counts of a mask: every thread of the workgroup brings the transitions T of one word of the mask's pixel
// stream (bit b set: the pixel at run-order position p0 + b differs from its predecessor; 0 for a thread without a word), the
// words of a chunk in run order over the threads.  An exclusive sum-scan of the pop-counts gives the rank of every word's first
// transition, an exclusive max-scan of "position of my last transition" the position of the last earlier one, both carried from
// chunk to chunk in rank_base / last_base (0, 0 before the first chunk), and every transition writes its own
// slot[k] = p_k - p_(k-1).  wsum, wmax: 4 words of LDS each.  The caller writes the last count, H*W - last_base, after the
// last chunk.
__device__ __forceinline__ void rle_counts_chunk(unsigned long long T, unsigned p0, uint32_t* __restrict__ slot, unsigned& rank_base,
                                                 unsigned& last_base, unsigned* wsum, unsigned* wmax) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned cnt = __popcll(T);
  const unsigned mine = T ? p0 + (63u - (unsigned)__clzll((long long)T)) : 0u;
  unsigned isum = cnt, imax = mine;      // inclusive scans within the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned a = __shfl_up(isum, d, 64), b = __shfl_up(imax, d, 64);
    if (lane >= d) { isum += a; imax = imax > b ? imax : b; }
  }
  unsigned emax = __shfl_up(imax, 1, 64);
  if (lane == 0) emax = 0;
  __syncthreads();      // the previous chunk's reads of wsum / wmax are over
  if (lane == 63) { wsum[wave] = isum; wmax[wave] = imax; }
  __syncthreads();
  unsigned k = rank_base + isum - cnt, prev = last_base > emax ? last_base : emax;
  unsigned tot = 0, top = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) { k += wsum[w]; prev = prev > wmax[w] ? prev : wmax[w]; }
    tot += wsum[w];
    top = top > wmax[w] ? top : wmax[w];
  }
  while (T) {
    const unsigned p = p0 + (unsigned)__builtin_ctzll(T);
    T &= T - 1ull;
    slot[k++] = p - prev;      // k < transitions < n_counts <= slot_words
    prev = p;
  }
  rank_base += tot;
  last_base = last_base > top ? last_base : top;
}

}  // namespace

#endif  // HGL_RLE_SCAN_H
