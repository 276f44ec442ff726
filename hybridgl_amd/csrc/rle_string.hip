// COCO's compressed RLE strings written and read on the device (hgl_rle_to_strings_device, hgl_rle_from_strings_device): the
// device forms of refer/external/maskApi.c rleToString (:203-216) and rleFrString (:217-230), the last two functions of that
// API that an encoded set met on the host only.  gtmask.cpp hgl_rle_to_string / hgl_rle_from_string are the sequential host
// forms and the yardstick; the arithmetic of a count and of a character group is written once, in rle_string.h, and shared in
// letter with the sanitizer harness.  One workgroup of RLE_THREADS per entry throughout; no atomics.
//
// Writing, three launches whatever S is:
//   1. lengths   every count's group length (its own value and the count two places earlier, read from the slot), summed
//                over the entry -> offsets[s]; the entry's status: 0 counts in the slot, 1 bit plane, 2 no mask.
//   2. scan      ONE workgroup turns the S lengths into offsets in place, 256 at a time with a carry; offsets[S] = the total.
//   3. write     256 counts at a time: an exclusive scan of the group lengths with a carry places every group, and its thread
//                writes its 1 .. 7 characters.  An entry that does not lie wholly inside [0, cap) gets status 3 and no byte.
//   THE HAZARD.  Neighbouring entries are written by different workgroups at arbitrary byte alignment, so no store wider than
//   a byte may cover a byte of another entry's extent.  Every store of step 3 is a byte store (global_store_byte): a group is
//   1 .. 7 characters at any alignment, and a thread owns exactly its group's bytes.
//
// Reading, one launch whatever S is:
//   sweep 1      the bytes 256 at a time: how many bytes end a group (the entry's n_counts), whether a byte is the eighth of
//                its group (long), whether the last byte continues (truncated).
//   sweep 2      an exclusive scan of "ends a group" with a carry gives every group its count index m; the thread of the
//                ending byte reads back the at most seven bytes of its group (they may lie in the chunk before) and writes the
//                raw difference x_m to slot[m].
//   sweep 3      the un-delta in place, 256 counts at a time: a stride-2 running sum (the odd chain, and the even chain from
//                index 2 on) with two carries.
#include "hgl_common.h"
#include "rle_scan.h"       // RLE_THREADS, rle_block_sum
#include "rle_string.h"

namespace {

// the workgroup-wide exclusive sum-scan of v in thread order; *total receives the sum.  lds: 4 elements
template <typename T>
__device__ __forceinline__ T rstr_block_scan(T v, T* lds, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T a = __shfl_up(inc, d, 64);
    if (lane >= d) inc += a;
  }
  __syncthreads();      // the previous use of lds is over
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  T before = inc - v, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) before += lds[w];
    tot += lds[w];
  }
  *total = tot;
  return before;
}

// what an entry of the set is to the writer: 0 its counts are in the slot, 1 its bit plane is, 2 it holds no mask
__device__ __forceinline__ int rstr_entry_code(const int32_t* row, long long slot_words) {
  const int n = row[0], form = row[1];
  if (form == 1) return 1;
  return (form == 0 && n >= 0 && (long long)n <= slot_words) ? 0 : 2;
}

// ---- writing, step 1
__global__ __launch_bounds__(RLE_THREADS) void rle_strlengths_kernel(const uint32_t* __restrict__ slots, long long slot_words,
                                                                   const int32_t* __restrict__ table, long long* __restrict__ offsets,
                                                                   int32_t* __restrict__ status) {
  __shared__ unsigned long long red[4];
  const int s = blockIdx.x, t = threadIdx.x;
  const int32_t* row = table + (size_t)s * 4;
  const int code = rstr_entry_code(row, slot_words);      // uniform over the workgroup
  unsigned long long len = 0;
  if (code == 0) {
    const uint32_t* slot = slots + (size_t)s * (size_t)slot_words;
    const long long n = row[0];      // <= slot_words
    for (long long i = t; i < n; i += RLE_THREADS) len += (unsigned)rstr_length(rstr_delta(slot, i));
    len = rle_block_sum(len, red);
  }
  if (t == 0) {
    offsets[s] = (long long)len;      // the scan turns lengths into offsets
    status[s] = code;
  }
}

// ---- writing, step 2: offsets[0 .. S) hold lengths; afterwards offsets[s] = the sum of the lengths before s, offsets[S] the total
__global__ __launch_bounds__(RLE_THREADS) void rle_stroffsets_kernel(long long* __restrict__ offsets, int S) {
  __shared__ long long lds[4];
  const int t = threadIdx.x;
  long long carry = 0;
  for (int base = 0; base < S; base += RLE_THREADS) {
    const int s = base + t;
    const long long len = s < S ? offsets[s] : 0ll;
    long long tot;
    const long long before = rstr_block_scan(len, lds, &tot);
    if (s < S) offsets[s] = carry + before;
    carry += tot;
  }
  if (t == 0) offsets[S] = carry;
}

// ---- writing, step 3
__global__ __launch_bounds__(RLE_THREADS) void rle_strwrite_kernel(const uint32_t* __restrict__ slots, long long slot_words,
                                                                 const int32_t* __restrict__ table, const long long* __restrict__ offsets,
                                                                 uint8_t* __restrict__ bytes, long long cap, int32_t* __restrict__ status) {
  __shared__ unsigned lds[4];
  const int s = blockIdx.x, t = threadIdx.x;
  const int32_t* row = table + (size_t)s * 4;
  if (rstr_entry_code(row, slot_words) != 0) return;      // uniform; status[s] is step 1's
  const long long begin = offsets[s], end = offsets[s + 1];      // 0 <= begin <= end: sums of lengths
  if (end > cap) {      // the string is good but does not lie wholly inside [0, cap): no byte of it
    if (t == 0) status[s] = 3;
    return;
  }
  const uint32_t* slot = slots + (size_t)s * (size_t)slot_words;
  const long long n = row[0];
  uint8_t* out = bytes + begin;
  unsigned long long pos = 0;      // characters of the counts before this chunk
  for (long long base = 0; base < n; base += RLE_THREADS) {
    const long long i = base + t;
    long long x = 0;
    unsigned k = 0;
    if (i < n) {
      x = rstr_delta(slot, i);
      k = (unsigned)rstr_length(x);
    }
    unsigned tot;
    const unsigned before = rstr_block_scan(k, lds, &tot);
    // pos + before + k <= end - begin: the same lengths that step 1 summed.  BYTE stores: see the hazard at the top
    for (unsigned j = 0; j < k; ++j) out[pos + before + j] = rstr_char(x, (int)j, (int)k);
    pos += tot;
  }
}

// ---- reading
__global__ __launch_bounds__(RLE_THREADS) void rle_strread_kernel(const uint8_t* __restrict__ bytes, long long total_bytes,
                                                                const long long* __restrict__ offsets, uint32_t* __restrict__ slots,
                                                                long long slot_words, int32_t* __restrict__ table,
                                                                int32_t* __restrict__ status) {
  __shared__ unsigned red[4], lds[4];
  __shared__ uint32_t wtot[4][2];
  const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int32_t* row = table + (size_t)s * 4;
  int32_t* stat = status + (size_t)s * 4;
  auto refuse = [&](int code, int n_counts) {      // the slot stays untouched; the decoders see "no mask"
    if (t == 0) {
      row[0] = n_counts; row[1] = 2; row[2] = 0; row[3] = 0;
      stat[0] = code; stat[1] = n_counts; stat[2] = 0; stat[3] = 0;
    }
  };
  const long long b0 = offsets[s], b1 = offsets[s + 1];
  if (b0 < 0 || b0 > b1 || b1 > total_bytes) { refuse(4, 0); return; }      // uniform over the workgroup
  const uint8_t* str = bytes + b0;
  const long long L = b1 - b0;      // < 2^31 (total_bytes is, checked by the host entry)

  // ---- sweep 1
  unsigned ends = 0, is_long = 0;
  for (long long p = t; p < L; p += RLE_THREADS) {
    ends += rstr_more(str[p]) ? 0u : 1u;
    is_long |= rstr_long_at(str, p) ? 1u : 0u;
  }
  ends = rle_block_sum(ends, red);
  is_long = rle_block_sum(is_long, red);
  if (is_long) { refuse(3, 0); return; }
  if (L > 0 && rstr_more(str[L - 1])) { refuse(2, 0); return; }
  if ((long long)ends > slot_words) { refuse(1, (int)ends); return; }
  if (t == 0) {
    row[0] = (int)ends; row[1] = 0; row[2] = 0; row[3] = 0;
    stat[0] = 0; stat[1] = (int)ends; stat[2] = 0; stat[3] = 0;
  }
  uint32_t* slot = slots + (size_t)s * (size_t)slot_words;

  // ---- sweep 2: the raw differences
  unsigned rank = 0;      // groups that end before this chunk
  for (long long base = 0; base < L; base += RLE_THREADS) {
    const long long p = base + t;
    const unsigned e = (p < L && !rstr_more(str[p])) ? 1u : 0u;
    unsigned tot;
    const unsigned before = rstr_block_scan(e, lds, &tot);
    if (e) {
      const int k = rstr_group_length(str, p);      // no long group: the group begins at p - k + 1 >= 0
      slot[rank + before] = rstr_group_value(str + (p - k + 1), k);      // rank + before < ends <= slot_words
    }
    rank += tot;
  }
  __syncthreads();      // every x_m is in the slot (the workgroup's own global stores, visible to it behind the barrier)

  // ---- sweep 3: counts[i] = x_i + counts[i-2] for i > 2, as two running sums; RLE_THREADS is even, so a thread keeps the
  // parity of its index from chunk to chunk
  uint32_t carry = 0;      // this thread's chain (t & 1) before the chunk
  for (long long base = 0; base < (long long)ends; base += RLE_THREADS) {
    const long long i = base + t;
    const uint32_t v = i < (long long)ends ? rstr_chain_term(i, slot[i]) : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int d = 2; d < 64; d <<= 1) {
      const uint32_t a = __shfl_up(inc, d, 64);
      if (lane >= d) inc += a;
    }
    __syncthreads();      // the previous chunk's reads of wtot are over
    if (lane >= 62) wtot[wave][lane & 1] = inc;
    __syncthreads();
    uint32_t sum = carry + inc, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) sum += wtot[w][t & 1];
      tot += wtot[w][t & 1];
    }
    if (i < (long long)ends && i != 0) slot[i] = sum;      // slot[0] = x_0 stays
    carry += tot;
  }
}

}  // namespace

extern "C" {

int hgl_rle_to_strings_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S, uint8_t* bytes,
                              long long cap, int64_t* offsets, int32_t* status, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(S >= 0 && offsets && cap >= 0 && (cap == 0 || bytes) && (S == 0 || (slots && table && status)),
              "rle_to_strings_device: bad arguments");
  HGL_REQUIRE(slot_words >= 0, "rle_to_strings_device: slot_words %lld", slot_words);
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets are 64-bit");
  hipStream_t st = (hipStream_t)stream;
  if (S > 0) {
    hipLaunchKernelGGL(rle_strlengths_kernel, dim3((unsigned)S), dim3(RLE_THREADS), 0, st, slots, slot_words, table, (long long*)offsets,
                       status);
    HGL_TRY(hgl_check_launch("rle_to_strings_device (lengths)"));
  }
  hipLaunchKernelGGL(rle_stroffsets_kernel, dim3(1), dim3(RLE_THREADS), 0, st, (long long*)offsets, S);      // S = 0: offsets[0] = 0
  HGL_TRY(hgl_check_launch("rle_to_strings_device (offsets)"));
  if (S > 0) {
    hipLaunchKernelGGL(rle_strwrite_kernel, dim3((unsigned)S), dim3(RLE_THREADS), 0, st, slots, slot_words, table,
                       (const long long*)offsets, bytes, cap, status);
    HGL_TRY(hgl_check_launch("rle_to_strings_device (write)"));
  }
  return HGL_OK;
}

int hgl_rle_from_strings_device(const uint8_t* bytes, long long total_bytes, const int64_t* offsets, int S, uint32_t* slots,
                                long long slot_words, int32_t* table, int32_t* status, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(S >= 0 && total_bytes >= 0 && (total_bytes == 0 || bytes) && (S == 0 || (offsets && slots && table && status)),
              "rle_from_strings_device: bad arguments");
  HGL_REQUIRE(total_bytes < (1ll << 31), "rle_from_strings_device: %lld bytes (the limit is 2^31 - 1)", total_bytes);
  HGL_REQUIRE(slot_words >= 0, "rle_from_strings_device: slot_words %lld", slot_words);
  if (S == 0) return HGL_OK;      // nothing to read, nothing to launch
  hipLaunchKernelGGL(rle_strread_kernel, dim3((unsigned)S), dim3(RLE_THREADS), 0, (hipStream_t)stream, bytes, total_bytes,
                     (const long long*)offsets, slots, slot_words, table, status);
  return hgl_check_launch("rle_from_strings_device");
}

}  // extern "C"
