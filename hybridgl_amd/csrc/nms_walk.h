// The steps of a greedy NMS that do not depend on what overlaps: the ranking order and the serial step of the walk over 64-row
// blocks of suppression words.  One copy of each, inlined into the box NMS (sam_nms.hip) and the mask NMS on encoded sets
// (rle.hip: hgl_rle_nms_device).
#ifndef HGL_NMS_WALK_H
#define HGL_NMS_WALK_H
#include "hgl_common.h"

namespace {

// The ranking order of every NMS kernel: descending score, the original index breaks ties, and a NaN score ranks ABOVE
// every number (where torch.sort(descending=True) -- batched_nms's argsort, automatic_mask_generator.py:251-257 -- puts it).
// A total order: ranks by counting never collide, order[] has no holes below the number of valid candidates.  (With a plain
// `sj > sc || (sj == sc && j < i)` two NaN scores -- an f16x3 overflow with the thresholds open -- both got rank 0.)
__device__ __forceinline__ bool nms_before(float sj, int j, float si, int i) {
  const bool nj = sj != sj, ni = si != si;
  if (nj || ni) return nj && (!ni || j < i);
  return sj > si || (sj == si && j < i);
}

// The walk's serial step, by one wave: lane l holds d, the diagonal word of row 64 rb + l (0 from row n on), and every lane
// rem, the removed bits of the block so far.  Row by row, a row that is not removed is kept and removes what its word names.
// -> the kept rows of the block
__device__ __forceinline__ unsigned long long nms_resolve_block(unsigned long long d, unsigned long long rem, int rb, int n) {
  unsigned long long km = 0;
  for (int s2 = 0; s2 < 64; ++s2) {
    const unsigned lo = __shfl((unsigned)(d & 0xffffffffull), s2), hi = __shfl((unsigned)(d >> 32), s2);
    if (rb * 64 + s2 < n && !((rem >> s2) & 1ull)) {
      km |= 1ull << s2;
      rem |= ((unsigned long long)hi << 32) | lo;
    }
  }
  return km;
}

// ... and its output, by the same wave: lane l appends candidate order[64 rb + l] if its row was kept; lane 0 hands the kept set
// to the other waves and moves the count on.
__device__ __forceinline__ void nms_emit_block(unsigned long long km, int rb, int lane, const int* order, int* out_idx,
                                               int& nkept, unsigned long long& kept_word) {
  const int base = nkept;
  if ((km >> lane) & 1ull) out_idx[base + __popcll(km & ((1ull << lane) - 1ull))] = order[rb * 64 + lane];
  if (lane == 0) { kept_word = km; nkept = base + __popcll(km); }
}

}  // namespace

#endif  // HGL_NMS_WALK_H
