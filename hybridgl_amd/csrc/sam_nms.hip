// Proposal selection of the SAM mask generator (third_party/segment-anything/segment_anything/*).
//   nms / nms_segments / nms_large   torchvision.ops.batched_nms as automatic_mask_generator.py:251-257,209-220,259-266 call it
//   box_near_crop_edge               utils/amg.py:78-88
//   gather_masks                     the kept rows of a mask stack, by a device index list
// Every decision of the greedy NMS is written once, as a __device__ function, and inlined into each kernel that takes it:
// the ranking order (nms_before), the rank by counting (nms_rank), the IoU test (nms_overlap), the suppression word of a row
// (nms_row_word) and the walk over the row blocks (nms_resolve_block, nms_emit_block, nms_or_kept_rows).  The order and the walk's
// serial step live in nms_walk.h: the mask NMS on encoded sets (rle.hip) takes the same ones.
#include "hgl_common.h"
#include "nms_walk.h"       // nms_before, nms_resolve_block, nms_emit_block
#include <math.h>

namespace {

// rank by counting: how many of the K candidates are valid (keep[j] != 0) and come before candidate i of score si
__device__ __forceinline__ int nms_rank(const float* scores, const unsigned char* keep, int K, float si, int i) {
  int rank = 0;
#pragma unroll 8
  for (int j = 0; j < K; ++j) rank += (keep[j] && nms_before(scores[j], j, si, i)) ? 1 : 0;
  return rank;
}

// The only IoU expression.  The build contracts the union into fma(wa, ha, wb * hb) - inter, which decides beyond coordinate
// 2896: every kernel inlines this one form.
__device__ __forceinline__ bool nms_overlap(const int4 a, const int4 b, float thr) {
  const float ax0 = (float)a.x, ay0 = (float)a.y, ax1 = (float)a.z, ay1 = (float)a.w;
  const float bx0 = (float)b.x, by0 = (float)b.y, bx1 = (float)b.z, by1 = (float)b.w;
  const float iw = fmaxf(fminf(ax1, bx1) - fmaxf(ax0, bx0), 0.f);
  const float ih = fmaxf(fminf(ay1, by1) - fmaxf(ay0, by0), 0.f);
  const float inter = iw * ih;
  const float iou = inter / ((ax1 - ax0) * (ay1 - ay0) + (bx1 - bx0) * (by1 - by0) - inter);
  return iou > thr;
}

// The suppression word of the row of rank q (box `me`) against the jn <= 64 boxes cols[0 .. jn) of ranks c0 + j: bit j is set
// where the column ranks behind the row and overlaps it.
__device__ __forceinline__ unsigned long long nms_row_word(int4 me, int q, const int4* cols, int c0, int jn, float thr) {
  unsigned long long word = 0;
#pragma unroll 4
  for (int j = 0; j < jn; ++j)
    if (c0 + j > q && nms_overlap(me, cols[j], thr)) word |= 1ull << j;
  return word;
}

// The walk's parallel step for one later word of removed[]: acc | that word of every kept row of block rb.  word_of_row(r) is
// the caller's addressing of the suppression words.
template <class WordOfRow>
__device__ __forceinline__ unsigned long long nms_or_kept_rows(unsigned long long acc, unsigned long long km, int rb,
                                                               WordOfRow word_of_row) {
  while (km) {
    const int s2 = __ffsll((long long)km) - 1;
    km &= km - 1;
    acc |= word_of_row(rb * 64 + s2);
  }
  return acc;
}

// Greedy NMS in one workgroup (K <= 1024): candidates with keep[k]!=0, descending score with the
// original index as tie-break (stable sort), suppress IoU > thr.  out_idx[0..n) in kept order.  One barrier pair per rank;
// the boxes are read from global memory with scalar int loads, so the box pointer needs no alignment.
__device__ __forceinline__ void nms_serial_body(const int* __restrict__ boxes, const float* __restrict__ scores,
                                                const uint8_t* __restrict__ keep, int K, float thr,
                                                int* __restrict__ out_idx, int* __restrict__ out_n) {
  __shared__ int order[1024];
  __shared__ unsigned char alive[1024];
  __shared__ int cur, nkept;
  const int t = threadIdx.x;
  const bool valid = t < K && keep[t];
  order[t] = -1;
  __syncthreads();
  if (valid) order[nms_rank(scores, keep, K, scores[t], t)] = t;
  alive[t] = 1;
  if (t == 0) nkept = 0;
  __syncthreads();
  int nvalid = 0;
  for (int j = 0; j < K; ++j) nvalid += keep[j] ? 1 : 0;  // uniform
  for (int r = 0; r < nvalid; ++r) {
    if (t == 0) cur = alive[r] ? order[r] : -1;
    __syncthreads();
    const int ci = cur;
    if (ci >= 0) {
      if (t == 0) { out_idx[nkept] = ci; ++nkept; }
      // suppress lower-ranked boxes overlapping ci
      const int me = (t > r && t < nvalid) ? order[t] : -1;
      if (me >= 0 && alive[t]) {
        const int4 a = make_int4(boxes[ci * 4], boxes[ci * 4 + 1], boxes[ci * 4 + 2], boxes[ci * 4 + 3]);
        const int4 b = make_int4(boxes[me * 4], boxes[me * 4 + 1], boxes[me * 4 + 2], boxes[me * 4 + 3]);
        if (nms_overlap(a, b, thr)) alive[t] = 0;
      }
    }
    __syncthreads();
  }
  if (t == 0) *out_n = nkept;
}

// The serial body's semantics for K <= 512 without its loop of K iterations x (two barriers + global loads of the current box:
// 82 us for the 192 candidates of an image): ranks by counting, the boxes in rank order in LDS, the suppression words of
// every row dealt to the 512 threads, then the walk over the row blocks -- the scheme of the any-K path below in one
// workgroup, on LDS-resident words.  Loads the boxes as int4: the box pointer must be 16-byte aligned.
__device__ __forceinline__ void nms_bits_body(const int* __restrict__ boxes, const float* __restrict__ scores,
                                              const uint8_t* __restrict__ keep, int K, float thr,
                                              int* __restrict__ out_idx, int* __restrict__ out_n) {
  __shared__ int4 sbox[512];
  __shared__ int order[512];
  __shared__ float ssc[512];
  __shared__ unsigned char skeep[512];
  __shared__ unsigned long long mask[512][8];
  __shared__ unsigned long long removed[8];
  __shared__ unsigned long long kept_word;
  __shared__ int nv, nkept_s;
  const int t = threadIdx.x, lane = t & 63;
  const bool valid = t < K && keep[t];
  const float sc = valid ? scores[t] : 0.f;
  ssc[t] = sc;
  skeep[t] = valid ? 1 : 0;
  order[t] = -1;
  if (t < 8) removed[t] = 0;
  if (t == 0) { nv = 0; nkept_s = 0; }
  __syncthreads();
  if (valid) {
    order[nms_rank(ssc, skeep, K, sc, t)] = t;
    atomicAdd(&nv, 1);
  }
  __syncthreads();
  const int n = nv;
  if (t < n) sbox[t] = ((const int4*)boxes)[order[t]];
  __syncthreads();
  const int nw = (n + 63) >> 6;
  // word w is needed of rows 0 .. min(n, 64 (w + 1)) - 1 (words left of a row's diagonal block are never read): the (word, row)
  // pairs are dealt to all 512 threads -- 384 pairs of 64 IoUs for 192 boxes, not three words for each of 192 threads
  for (int w = 0, q0 = 0; w < nw; ++w) {
    const int rows = min(n, 64 * (w + 1));
    for (int q = t - (q0 & 511); q < rows; q += 512) {
      if (q < 0) continue;
      mask[q][w] = nms_row_word(sbox[q], q, sbox + 64 * w, 64 * w, min(64, n - 64 * w), thr);
    }
    q0 += rows;
  }
  __syncthreads();
  for (int rb = 0; rb < nw; ++rb) {
    if (t < 64) {
      const int a = rb * 64 + lane;
      const unsigned long long km = nms_resolve_block(a < n ? mask[a][rb] : 0ull, removed[rb], rb, n);
      nms_emit_block(km, rb, lane, order, out_idx, nkept_s, kept_word);
    }
    __syncthreads();
    if (t > rb && t < nw) removed[t] = nms_or_kept_rows(removed[t], kept_word, rb, [&](int r) { return mask[r][t]; });
    __syncthreads();
  }
  if (t == 0) *out_n = nkept_s;
}

// One workgroup a candidate list, exactly one of the two bodies a launch.  BITS: the LDS bit-matrix body (lists of up to 512
// candidates, 512 threads), else the serial body (up to 1024, 1024 threads).
//   offsets == nullptr: the single list [0, K) -- hgl_nms, a grid of one; the host has chosen the body.
//   else: workgroup s runs segment s = candidates offsets[s] .. offsets[s+1] exactly as hgl_nms runs that list alone:
//   out_idx[offsets[s] + 0 .. out_n[s]) holds the kept candidates as indices INTO the segment.  The BITS launch serves the
//   segments of 1 .. 512 candidates, the other launch those of 513 .. 1024; a workgroup whose segment belongs to the other
//   launch returns at once.
template <bool BITS>
__global__ __launch_bounds__(BITS ? 512 : 1024) void nms_segments_kernel(const int* __restrict__ boxes,
                                                                         const float* __restrict__ scores,
                                                                         const uint8_t* __restrict__ keep,
                                                                         const int* __restrict__ offsets, int K, float thr,
                                                                         int* __restrict__ out_idx, int* __restrict__ out_n) {
  const int s = blockIdx.x;
  int o = 0;
  if (offsets) {
    o = offsets[s];
    K = offsets[s + 1] - o;
    // (a list that is empty, or longer than the caller's max_len admits, keeps nothing: out_n[s] = 0 from the BITS launch,
    // which runs first; the other launch then overwrites the count of the lists it serves)
    if (K <= 0 || K > 512) {
      if (BITS && threadIdx.x == 0) out_n[s] = 0;
      if (BITS || K <= 0 || K > 1024) return;
    } else if (!BITS) {
      return;
    }
  }
  if (BITS)
    nms_bits_body(boxes + 4ll * o, scores + o, keep + o, K, thr, out_idx + o, out_n + s);
  else
    nms_serial_body(boxes + 4ll * o, scores + o, keep + o, K, thr, out_idx + o, out_n + s);
}

// ---- NMS for any K (crop layers / dense point grids, automatic_mask_generator.py:209-220,259-266) ----------
// The same semantics in three passes: rank by counting -> 64x64-bit suppression words of the sorted boxes -> one workgroup
// walks the row blocks, resolving each 64-row block with wave shuffles and OR-ing the kept rows into the running "removed"
// bit set.
__global__ __launch_bounds__(256) void nms_rank_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ keep,
                                                       int K, int* __restrict__ order, int* __restrict__ nvalid) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K || !keep[i]) return;
  order[nms_rank(scores, keep, K, scores[i], i)] = i;
  atomicAdd(nvalid, 1);
}

// grid (W, W), 64 threads: word (row a = 64*by + t, column block bx) of the upper triangle
__global__ __launch_bounds__(64) void nms_mask_kernel(const int* __restrict__ boxes, const int* __restrict__ order,
                                                      const int* __restrict__ nvalid, int W, float thr,
                                                      unsigned long long* __restrict__ mask) {
  const int cb = blockIdx.x, rb = blockIdx.y, t = threadIdx.x;
  const int n = *nvalid;
  if (cb < rb || rb * 64 >= n) return;
  __shared__ int4 colbox[64];
  const int b = cb * 64 + t;
  colbox[t] = b < n ? ((const int4*)boxes)[order[b]] : make_int4(0, 0, 0, 0);
  __syncthreads();
  const int a = rb * 64 + t;
  if (a >= n) return;       // the mask has K rows, not 64 W: rows from n on are neither written nor read (nms_scan_kernel)
  mask[(long long)a * W + cb] = nms_row_word(((const int4*)boxes)[order[a]], a, colbox, cb * 64, min(64, n - cb * 64), thr);
}

__global__ __launch_bounds__(256) void nms_scan_kernel(const unsigned long long* __restrict__ mask,
                                                       const int* __restrict__ order, const int* __restrict__ nvalid,
                                                       int W, int* __restrict__ out_idx, int* __restrict__ out_n) {
  __shared__ unsigned long long removed[1024];
  __shared__ unsigned long long kept_word;
  __shared__ int nkept_s;
  const int t = threadIdx.x, lane = t & 63;
  const int n = *nvalid;
  for (int w = t; w < W; w += 256) removed[w] = 0;
  if (t == 0) nkept_s = 0;
  __syncthreads();
  const int nblk = (n + 63) / 64;
  for (int rb = 0; rb < nblk; ++rb) {
    if (t < 64) {
      const int a = rb * 64 + lane;
      const unsigned long long km = nms_resolve_block(a < n ? mask[(long long)a * W + rb] : 0ull, removed[rb], rb, n);
      nms_emit_block(km, rb, lane, order, out_idx, nkept_s, kept_word);
    }
    __syncthreads();
    for (int w = rb + 1 + t; w < W; w += 256)
      removed[w] = nms_or_kept_rows(removed[w], kept_word, rb, [&](int r) { return mask[(long long)r * W + w]; });
    __syncthreads();
  }
  if (t == 0) *out_n = nkept_s;
}

// is_box_near_crop_edge (utils/amg.py:78-88) applied to keep flags: boxes are in crop coordinates
__global__ __launch_bounds__(256) void crop_edge_kernel(const int* __restrict__ boxes, int K, int cx0, int cy0, int cx1,
                                                        int cy1, int ox0, int oy0, int ox1, int oy1, float atol,
                                                        uint8_t* __restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K) return;
  const float b[4] = {(float)(boxes[i * 4] + cx0), (float)(boxes[i * 4 + 1] + cy0), (float)(boxes[i * 4 + 2] + cx0),
                      (float)(boxes[i * 4 + 3] + cy0)};
  const float c[4] = {(float)cx0, (float)cy0, (float)cx1, (float)cy1};
  const float o[4] = {(float)ox0, (float)oy0, (float)ox1, (float)oy1};
  bool near = false;
#pragma unroll
  for (int e = 0; e < 4; ++e) near |= (fabsf(b[e] - c[e]) <= atol) && !(fabsf(b[e] - o[e]) <= atol);
  if (near) keep[i] = 0;
}

// dst[i] = src[idx[i]] for i < *n (rows of row_bytes bytes, 16-byte multiples)
__global__ __launch_bounds__(256) void gather_masks_kernel(const uint8_t* __restrict__ src,
                                                           const int* __restrict__ idx,
                                                           const int* __restrict__ n, long long row16,
                                                           uint8_t* __restrict__ dst) {
  const int i = blockIdx.y;
  if (i >= *n) return;
  const uint4* s = (const uint4*)(src + (long long)idx[i] * row16 * 16);
  uint4* d = (uint4*)(dst + (long long)i * row16 * 16);
  for (long long j = blockIdx.x * 256ll + threadIdx.x; j < row16; j += (long long)gridDim.x * 256) d[j] = s[j];
}

}  // namespace

extern "C" {

// a single list is one segment: the segment kernel with a grid of one and no offsets
int hgl_nms(const int32_t* boxes_xyxy, const float* scores, const uint8_t* keep, int K, float iou_threshold,
            int32_t* out_idx, int32_t* out_n, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(boxes_xyxy && scores && keep && out_idx && out_n, "nms: null argument");
  HGL_REQUIRE(K > 0 && K <= 1024, "nms: K must be in [1,1024] (got %d)", K);
  hipStream_t st = (hipStream_t)stream;
  if (K <= 512 && ((uintptr_t)boxes_xyxy & 15) == 0)
    hipLaunchKernelGGL(nms_segments_kernel<true>, dim3(1), dim3(512), 0, st, (const int*)boxes_xyxy, scores, keep,
                       (const int*)nullptr, K, iou_threshold, (int*)out_idx, (int*)out_n);
  else
    hipLaunchKernelGGL(nms_segments_kernel<false>, dim3(1), dim3(1024), 0, st, (const int*)boxes_xyxy, scores, keep,
                       (const int*)nullptr, K, iou_threshold, (int*)out_idx, (int*)out_n);
  return hgl_check_launch("nms");
}

int hgl_nms_segments(const int32_t* boxes_xyxy, const float* scores, const uint8_t* keep, const int32_t* offsets, int n_seg,
                     int max_len, float iou_threshold, int32_t* out_idx, int32_t* out_n, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(boxes_xyxy && scores && keep && offsets && out_idx && out_n, "nms_segments: null argument");
  HGL_REQUIRE(n_seg > 0 && n_seg <= 65535, "nms_segments: n_seg must be in [1,65535] (got %d)", n_seg);
  HGL_REQUIRE(max_len >= 0 && max_len <= 1024, "nms_segments: segments hold up to 1024 candidates (max_len %d)", max_len);
  HGL_REQUIRE(((uintptr_t)boxes_xyxy & 15) == 0, "nms_segments: boxes must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(nms_segments_kernel<true>, dim3(n_seg), dim3(512), 0, st, (const int*)boxes_xyxy, scores, keep,
                     (const int*)offsets, 0, iou_threshold, (int*)out_idx, (int*)out_n);
  if (max_len > 512)
    hipLaunchKernelGGL(nms_segments_kernel<false>, dim3(n_seg), dim3(1024), 0, st, (const int*)boxes_xyxy, scores, keep,
                       (const int*)offsets, 0, iou_threshold, (int*)out_idx, (int*)out_n);
  return hgl_check_launch("nms_segments");
}

size_t hgl_nms_large_workspace_bytes(int K) {
  const size_t W = ((size_t)K + 63) / 64;
  return hgl_align_up((size_t)K * sizeof(int), 256) + hgl_align_up(sizeof(int), 256) + hgl_align_up((size_t)K * W * 8, 256);
}

int hgl_nms_large(const int32_t* boxes_xyxy, const float* scores, const uint8_t* keep, int K, float iou_threshold,
                  int32_t* out_idx, int32_t* out_n, void* workspace, size_t workspace_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(boxes_xyxy && scores && keep && out_idx && out_n, "nms_large: null argument");
  HGL_REQUIRE(K > 0 && K <= 32768, "nms_large: K must be in [1,32768] (got %d)", K);
  HGL_REQUIRE(((uintptr_t)boxes_xyxy & 15) == 0, "nms_large: boxes must be 16-byte aligned");
  if (!workspace || workspace_bytes < hgl_nms_large_workspace_bytes(K)) {
    hgl_set_error("nms_large: workspace too small");
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int W = (K + 63) / 64;
  HglArena ar(workspace, workspace_bytes);
  int* order = ar.take<int>((size_t)K);
  int* nvalid = ar.take<int>(1);
  unsigned long long* mask = ar.take<unsigned long long>((size_t)K * W);
  if (hipMemsetAsync(nvalid, 0, sizeof(int), st) != hipSuccess) {
    hgl_set_error("nms_large: memset failed");
    return HGL_ELAUNCH;
  }
  hipLaunchKernelGGL(nms_rank_kernel, dim3((K + 255) / 256), dim3(256), 0, st, scores, keep, K, order, nvalid);
  hipLaunchKernelGGL(nms_mask_kernel, dim3(W, W), dim3(64), 0, st, (const int*)boxes_xyxy, order, nvalid, W, iou_threshold, mask);
  hipLaunchKernelGGL(nms_scan_kernel, dim3(1), dim3(256), 0, st, mask, order, nvalid, W, (int*)out_idx, (int*)out_n);
  return hgl_check_launch("nms_large");
}

int hgl_box_near_crop_edge(const int32_t* boxes_xyxy, int K, const int32_t* crop_box_xyxy, const int32_t* orig_box_xyxy,
                           float atol, uint8_t* keep, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(boxes_xyxy && crop_box_xyxy && orig_box_xyxy && keep && K > 0, "box_near_crop_edge: bad arguments");
  hipLaunchKernelGGL(crop_edge_kernel, dim3((K + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const int*)boxes_xyxy, K,
                     crop_box_xyxy[0], crop_box_xyxy[1], crop_box_xyxy[2], crop_box_xyxy[3], orig_box_xyxy[0],
                     orig_box_xyxy[1], orig_box_xyxy[2], orig_box_xyxy[3], atol, keep);
  return hgl_check_launch("box_near_crop_edge");
}

int hgl_gather_masks(const uint8_t* masks, const int32_t* idx, const int32_t* n, int max_n, long long HW,
                     uint8_t* out, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(masks && idx && n && out && max_n > 0 && HW > 0 && (HW & 15) == 0, "gather_masks: bad arguments (HW must be a multiple of 16)");
  hipLaunchKernelGGL(gather_masks_kernel, dim3(64, max_n), dim3(256), 0, (hipStream_t)stream, masks, (const int*)idx, (const int*)n, HW / 16, out);
  return hgl_check_launch("gather_masks");
}

}  // extern "C"
