// Pieces that the RLE kernels of rle.hip, rle_poly.hip and rle_clean.hip share: one copy of each decision.  Workgroups of
// RLE_THREADS = 256 threads = 4 waves throughout.  Device: the block reductions, the image search, the scan that writes counts,
// and the run writer rle_write_runs over any column plane (the encoder, the merge and the clean-up all end in it).  Host: the
// carve of a staged set in a workspace (rle_stage_ws) and, with external linkage in rle.hip, rle_stage_set, which fills it.
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

// the workgroup-wide maximum of v (rle_block_sum's shape)
__device__ __forceinline__ unsigned rle_block_max(unsigned v, unsigned* lds) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned o = __shfl_xor(v, d, 64);
    v = v > o ? v : o;
  }
  __syncthreads();      // the previous use of lds is over
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const unsigned a = lds[0] > lds[1] ? lds[0] : lds[1], b = lds[2] > lds[3] ? lds[2] : lds[3];
  return a > b ? a : b;
}

// the transitions of word q of a mask's column plane P (q = x*HW64 + j); *C receives the word itself
__device__ __forceinline__ unsigned long long rle_transitions(const unsigned long long* P, unsigned q, int H, int HW64,
                                                              unsigned long long* C) {
  const int j = (int)(q % (unsigned)HW64);
  const int nb = H - 64 * j < 64 ? H - 64 * j : 64;
  const unsigned long long valid = nb == 64 ? ~0ull : ((1ull << nb) - 1ull);
  unsigned long long carry = 0;
  if (q > 0) {
    const int jp = j > 0 ? j - 1 : HW64 - 1;
    const int nbp = H - 64 * jp < 64 ? H - 64 * jp : 64;
    carry = (P[q - 1] >> (nbp - 1)) & 1ull;
  }
  const unsigned long long c = P[q];
  *C = c;
  return (c ^ ((c << 1) | carry)) & valid;
}

// n <= 32 pixels of column x from row y on, out of the column's 64-bit words (y + n <= H)
__device__ __forceinline__ uint32_t rle_column_bits(const unsigned long long* col, int y, int n) {
  const int j = y >> 6, o = y & 63;
  unsigned long long v = col[j] >> o;
  if (o + n > 64) v |= col[j + 1] << (64 - o);
  return (uint32_t)v & (n == 32 ? 0xffffffffu : ((1u << n) - 1u));
}

// The run writer: what the slot and the table row of one H x W mask hold, out of its column plane P (W * HW64 words, padding bits
// 0).  The whole workgroup calls it; red, wsum, wmax: 4 words of LDS each.  ONE copy: the encoder's plane comes from
// rle_columns_kernel, the merge's from the vote of its own workgroup (rle_merge_kernel), the clean-up's from the staged set as
// its passes rewrote it (rle_clean_kernel).
__device__ __forceinline__ void rle_write_runs(const unsigned long long* P, int H, int W, int HW64, uint32_t* slot, long long slot_words,
                                               int32_t* row, unsigned* red, unsigned* wsum, unsigned* wmax) {
  const int t = threadIdx.x;
  const unsigned Q = (unsigned)W * (unsigned)HW64;
  const unsigned HW = (unsigned)H * (unsigned)W;      // < 2^31 (checked by the host entry)

  // ---- sweep 1: how many counts, how many foreground pixels -> what the slot holds
  unsigned trans = 0, area = 0;
  for (unsigned q = t; q < Q; q += RLE_THREADS) {
    unsigned long long c;
    trans += __popcll(rle_transitions(P, q, H, HW64, &c));
    area += __popcll(c);
  }
  trans = rle_block_sum(trans, red);
  area = rle_block_sum(area, red);
  const unsigned n_counts = trans + 1u;
  const unsigned plane_words = (HW + 31u) / 32u;
  const int form = (long long)n_counts <= slot_words ? 0 : ((long long)plane_words <= slot_words ? 1 : 2);
  if (t == 0) { row[0] = (int32_t)n_counts; row[1] = form; row[2] = (int32_t)area; row[3] = 0; }
  if (form == 2) return;
  if (form == 1) {
    // the bit plane in run order: 32 pixels per word, LSB first; a word may span several columns when H < 32
    for (unsigned w = t; w < plane_words; w += RLE_THREADS) {
      const unsigned p = 32u * w;
      int x = (int)(p / (unsigned)H), y = (int)(p % (unsigned)H), filled = 0;
      uint32_t out = 0;
      while (filled < 32 && x < W) {
        const int n = 32 - filled < H - y ? 32 - filled : H - y;
        out |= rle_column_bits(P + (size_t)x * HW64, y, n) << filled;
        filled += n;
        y += n;
        if (y == H) { y = 0; ++x; }
      }
      slot[w] = out;
    }
    return;
  }
  // ---- sweep 2 (form 0): 256 words at a time, rank and previous position carried from chunk to chunk
  unsigned rank_base = 0, last_base = 0;      // counts written so far; position of the last transition so far (0: none)
  for (unsigned base = 0; base < Q; base += RLE_THREADS) {
    const unsigned q = base + t;
    unsigned long long T = 0, c;
    unsigned p0 = 0;
    if (q < Q) {
      T = rle_transitions(P, q, H, HW64, &c);
      p0 = (q / (unsigned)HW64) * (unsigned)H + 64u * (q % (unsigned)HW64);
    }
    rle_counts_chunk(T, p0, slot, rank_base, last_base, wsum, wmax);      // rle_scan.h; k < trans < n_counts <= slot_words
  }
  if (t == 0) slot[trans] = HW - last_base;
}

// run starts of one set: [S] arrays of slot_words + 1 words
inline size_t rle_starts_bytes(int S, long long slot_words) { return hgl_align_up((size_t)S * (size_t)(slot_words + 1) * sizeof(uint32_t), 256); }
inline size_t rle_status_bytes(int S) { return hgl_align_up((size_t)S * 4 * sizeof(int32_t), 256); }

// A set staged for the kernels that read planes, in the workspace: run starts, status, boxes (when wanted) and the column words
// of every entry (rle.hip, C and D).  rle_stage_ws carves it at *p and moves *p behind it.
constexpr size_t RLE_NO_BOXES = ~(size_t)0;
struct RleStageWs {
  size_t E, status, boxes, plane;      // boxes: RLE_NO_BOXES when not wanted
};
inline RleStageWs rle_stage_ws(size_t* p, int S, long long slot_words, long long plane_words, bool boxes) {
  RleStageWs w;
  w.E = *p;
  *p += rle_starts_bytes(S, slot_words);
  w.status = *p;
  *p += rle_status_bytes(S);
  w.boxes = boxes ? *p : RLE_NO_BOXES;
  if (boxes) *p += rle_status_bytes(S);
  w.plane = *p;
  *p += hgl_align_up((size_t)plane_words * sizeof(unsigned long long), 256);
  return w;
}

}  // namespace

// rle.hip's staging (rle_stage_launch: the starts kernel without boxes, the plane kernel) of a set of G images into the three
// arrays of a carve without boxes, which lie in one workspace: two launches on `stream`, none for S = 0.  Defined in rle.hip,
// whose kernels they are; called by rle_clean.hip.
struct RleSet;
void rle_stage_set(const uint32_t* slots, long long slot_words, const int32_t* table, int S, const RleSet& set, uint32_t* E,
                   int32_t* status, unsigned long long* plane, void* stream);
// The same two kernels over a paint list (RlePick, rle_group.h): one row of run starts, one status row and one plane per list
// position, read from the entry the position names (status code 3 and an empty plane when it names none).  Two launches, K > 0.
// Defined in rle.hip; called by rle_paint.hip.
struct RlePick;
void rle_stage_picked(const uint32_t* slots, long long slot_words, const int32_t* table, int K, const RlePick& pick, uint32_t* E,
                      int32_t* status, unsigned long long* plane, void* stream);

#endif  // HGL_RLE_SCAN_H
