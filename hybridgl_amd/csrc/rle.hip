// Run-length encoding of device masks, selected by a DEVICE index tensor (hgl_rle_encode_device).
//
// The records the mask generator hands out in its RLE modes and the evaluator's winning masks are column-major run
// lengths (utils/amg.py:107-136 mask_to_rle_pytorch, refer/external/maskApi.c rleEncode): runs over p = x*H + y, the first
// count = leading zeros (0 when pixel (0,0) is set), runs continue across column boundaries, the last count ends at H*W.
// hgl_rle_encode_mask (gtmask.cpp) is the host form of the same arithmetic; here the masks never leave the device as
// pixels -- only runs (or, for a mask with more runs than its slot holds, one bit per pixel) cross to the host.
//
// Two launches, no atomics, no host synchronisation; every selected entry owns its slot and its table row.
//
//   1. rle_columns_kernel   the masks are row-major, the runs column-major.  Lane x of a wave walks 64 rows of column x: every
//      row is read coalesced across the lanes (1 or 4 bytes per lane) and sets one bit of the lane's own 64-bit column word.
//      The column words, every column padded to whole 64-bit words, go to the workspace in run order: word x*HW64 + j holds
//      the pixels y = 64j .. 64j+63 of column x (bits beyond H are 0).  No LDS transpose, no strided byte walk.
//   2. rle_runs_kernel      one workgroup per selected mask.  A pixel starts a run where it differs from its predecessor in run
//      order: T = C ^ ((C << 1) | carry_in), masked to the valid bits of the word; carry_in is the last valid pixel of the
//      previous word (0 before the first pixel, so a mask that starts with foreground has a transition at p = 0 and
//      counts[0] = 0).  A first sweep pop-counts T (the number of counts is transitions + 1) and C (the area) and so decides
//      what the slot holds; the second sweep takes the words 256 at a time: an exclusive sum-scan of the pop-counts gives the
//      rank of every word's first transition, an exclusive max-scan of "position of my last transition" the position of the
//      last earlier one, both carried from chunk to chunk, and every transition writes its own counts[k] = p_k - p_(k-1).
//
// Slot forms (table row = n_counts, form, area, 0): 0 = the n_counts counts (whenever they fit), 1 = the column-major bit
// plane (bit p % 32 of word p / 32; whenever the counts do not fit but ceil(H*W/32) words do), 2 = neither fits, nothing
// written, 3 = the index is outside [0, N), nothing read or written.  Words beyond what the form defines keep their bytes.
#include "hgl_common.h"

namespace {

constexpr int RLE_THREADS = 256;

// the mask of entry s, or -1 when its index is outside [0, N) (the host never sees the indices)
__device__ __forceinline__ long long rle_pick(const long long* sel, int s, int N) {
  const long long n = sel ? sel[s] : (long long)s;
  return (n < 0 || n >= (long long)N) ? -1 : n;
}

// V columns per lane (4: one aligned 32-bit load per row when W % 4 == 0), 64 rows per wave, 4 waves = 4 row tiles per block
template <int V>
__global__ __launch_bounds__(RLE_THREADS) void rle_columns_kernel(const uint8_t* __restrict__ masks, int N, int H, int W,
                                                                  const long long* __restrict__ sel, int HW64, int col_tiles,
                                                                  int row_tiles, unsigned long long* __restrict__ plane) {
  const unsigned tile = blockIdx.x;
  const int s = (int)(tile / (unsigned)(col_tiles * row_tiles));
  const int rem = (int)(tile % (unsigned)(col_tiles * row_tiles));
  const long long n = rle_pick(sel, s, N);
  if (n < 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = (rem / col_tiles) * 4 + wave;
  const int x = ((rem % col_tiles) * 64 + lane) * V;
  if (j >= HW64 || x >= W) return;      // no barrier and no cross-lane operation below
  const int y0 = j * 64;
  const int rows = H - y0 < 64 ? H - y0 : 64;
  const uint8_t* src = masks + (size_t)n * H * W + (size_t)y0 * W + x;
  unsigned long long c[V];
#pragma unroll
  for (int k = 0; k < V; ++k) c[k] = 0;
#pragma unroll 8
  for (int r = 0; r < rows; ++r) {
    if (V == 4) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(src + (size_t)r * W);
#pragma unroll
      for (int k = 0; k < V; ++k) c[k] |= (unsigned long long)(((v >> (8 * k)) & 0xffu) != 0) << r;
    } else {
      c[0] |= (unsigned long long)(src[(size_t)r * W] != 0) << r;
    }
  }
  unsigned long long* dst = plane + (size_t)s * W * HW64 + (size_t)x * HW64 + j;
#pragma unroll
  for (int k = 0; k < V; ++k) dst[(size_t)k * HW64] = c[k];      // x + k < W: W % 4 == 0 on the 4-column path
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

__device__ __forceinline__ unsigned rle_block_sum(unsigned v, unsigned* lds) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();      // the previous use of lds is over
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

// n <= 32 pixels of column x from row y on, out of the column's 64-bit words (y + n <= H)
__device__ __forceinline__ uint32_t rle_column_bits(const unsigned long long* col, int y, int n) {
  const int j = y >> 6, o = y & 63;
  unsigned long long v = col[j] >> o;
  if (o + n > 64) v |= col[j + 1] << (64 - o);
  return (uint32_t)v & (n == 32 ? 0xffffffffu : ((1u << n) - 1u));
}

__global__ __launch_bounds__(RLE_THREADS) void rle_runs_kernel(const unsigned long long* __restrict__ plane, int N, int H, int W,
                                                               const long long* __restrict__ sel, int HW64,
                                                               uint32_t* __restrict__ slots, long long slot_words,
                                                               int32_t* __restrict__ table) {
  __shared__ unsigned red[4];
  __shared__ unsigned wsum[4], wmax[4];
  const int s = blockIdx.x, t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  int32_t* row = table + (size_t)s * 4;
  if (rle_pick(sel, s, N) < 0) {
    if (t == 0) { row[0] = 0; row[1] = 3; row[2] = 0; row[3] = 0; }
    return;
  }
  const unsigned long long* P = plane + (size_t)s * W * HW64;
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
  uint32_t* slot = slots + (size_t)s * (size_t)slot_words;
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
      slot[k++] = p - prev;      // k < trans < n_counts <= slot_words
      prev = p;
    }
    rank_base += tot;
    last_base = last_base > top ? last_base : top;
  }
  if (t == 0) slot[trans] = HW - last_base;
}

}  // namespace

extern "C" {

size_t hgl_rle_encode_workspace_bytes(int S, int H, int W) {
  if (S <= 0 || H <= 0 || W <= 0) return 0;
  return hgl_align_up((size_t)S * (size_t)W * (size_t)((H + 63) / 64) * sizeof(unsigned long long), 256);
}

int hgl_rle_encode_device(const uint8_t* masks, int N, int H, int W, const int64_t* sel, int S, uint32_t* slots,
                          long long slot_words, int32_t* table, void* ws, size_t ws_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(masks && slots && table && N > 0 && H > 0 && W > 0 && S > 0 && slot_words >= 0, "rle_encode_device: bad arguments");
  HGL_REQUIRE(sel || S <= N, "rle_encode_device: without an index tensor S (%d) must not exceed N (%d)", S, N);
  HGL_REQUIRE((long long)N * H * W < (1ll << 31), "rle_encode_device: batch too large (N*H*W must be < 2^31)");
  const int HW64 = (H + 63) / 64;
  const bool wide = (W % 4 == 0) && (((uintptr_t)masks & 3u) == 0);
  const int col_tiles = (W + (wide ? 255 : 63)) / (wide ? 256 : 64), row_tiles = (HW64 + 3) / 4;
  const long long tiles = (long long)S * col_tiles * row_tiles;
  HGL_REQUIRE(tiles < (1ll << 31), "rle_encode_device: too many entries (%d) for one launch", S);
  if (!ws || ws_bytes < hgl_rle_encode_workspace_bytes(S, H, W)) {
    hgl_set_error("rle_encode_device: workspace too small");
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* plane = (unsigned long long*)ws;
  const long long* sel64 = (const long long*)sel;
  if (wide)
    hipLaunchKernelGGL(rle_columns_kernel<4>, dim3((unsigned)tiles), dim3(RLE_THREADS), 0, st, masks, N, H, W, sel64, HW64,
                       col_tiles, row_tiles, plane);
  else
    hipLaunchKernelGGL(rle_columns_kernel<1>, dim3((unsigned)tiles), dim3(RLE_THREADS), 0, st, masks, N, H, W, sel64, HW64,
                       col_tiles, row_tiles, plane);
  hipLaunchKernelGGL(rle_runs_kernel, dim3((unsigned)S), dim3(RLE_THREADS), 0, st, (const unsigned long long*)plane, N, H, W,
                     sel64, HW64, slots, slot_words, table);
  return hgl_check_launch("rle_encode_device");
}

}  // extern "C"
