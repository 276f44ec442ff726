// The geometry of the fused mask post-processing (sam_glue.hip: sam_postprocess_kernel, sam_postprocess_sep_kernel and the
// host's choice between them), once: plain functions that compile under g++ (tests/native/post_geom_routes.cpp, which
// tests/test_post_cases_host.py holds against the Python restatement of tests/post_cases.py) and as __host__ __device__ code
// under hipcc.  Nothing here needs HIP when __HIPCC__ is absent.  An output index goes through two bilinear resamplings, both
// align_corners=False with ATen's source index (one fma): output -> stage 1 (the crop [hi, wi] of the S x S plane) at scale
// in / out, stage 1 -> low-res at scale low / S.  The kernels and the host must agree on every index to the bit: the same
// IEEE operations, one copy of them.
#ifndef HGL_POST_GEOM_H
#define HGL_POST_GEOM_H
#include <math.h>

#ifdef __HIPCC__
#define POST_FN static __host__ __device__ __forceinline__
#else
#define POST_FN static inline
#endif

// One workgroup = a 64x64 tile of output pixels of one candidate; a thread computes 16 consecutive pixels of one
// row and stores them as one 16-byte word.  The low-res logits the tile touches (a <= 48x48 patch for every
// realistic size ratio) are staged in LDS once, so the 16 taps per pixel are LDS reads instead of scattered global
// loads.  (The first version used 16x16 tiles with one pixel per thread: 300k workgroups whose fixed cost -- bounds,
// staging, two barriers, the reduction, atomics -- was 95 % of the 3.3 ms the kernel took.)
constexpr int PTW = 64, PTH = 64;   // output tile
constexpr int PPX = 16;             // pixels per thread (one row segment)
constexpr int PR = 48;              // max staged low-res patch side
constexpr int PX1 = 112;            // max stage-1 columns of a tile (64 output columns at a 1.6 : 1 size ratio: 104).  Wider
                                    // tables (192 columns = 47 KB of LDS, for the 2.7 : 1 crops of a crop layer) measured SLOWER
                                    // than the per-pixel kernel there (3.1 against 2.0 ms per crop): three workgroups per CU
                                    // do not hide the load -> build -> interpolate chain of a tile.  Round 6: 32-column tiles
                                    // (88 stage-1 columns: these tables, 128 threads) on the same crops: 3.1 ms again -- the
                                    // table of a tile costs what its 2048 pixels save

// scale of one axis of one resampling
POST_FN float post_scale(int in, int out) { return (float)in / (float)out; }

// destination index -> the two source indices and their weights (callers that need only the indices ignore the weights)
POST_FN void src_idx(float scale, int dst, int in_size, int& i0, int& i1, float& l0, float& l1) {
  float f = fmaf(scale, dst + 0.5f, -0.5f);
  f = f < 0.f ? 0.f : f;
  i0 = (int)f;
  i0 = i0 < in_size - 1 ? i0 : in_size - 1;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = f - i0;
  l0 = 1.f - l1;
}

// What one axis of one tile touches: output indices o0 .. ol (taps are monotone in the output index) at stage-1 scale s1 over
// a crop of `crop` and low-res scale s2 over a plane of `low`.
struct PostAxis {
  int s1_first, s1_count;     // first stage-1 index, number of stage-1 columns (rows)
  int low_first, patch;       // first low-res index, side of the low-res patch
};
POST_FN PostAxis post_axis(int o0, int ol, float s1, float s2, int crop, int low) {
  int a0, a1, b0, b1, u0, u1, e0, e1;
  float f0, f1;
  src_idx(s1, o0, crop, a0, a1, f0, f1);
  src_idx(s2, a0, low, u0, u1, f0, f1);
  src_idx(s1, ol, crop, b0, b1, f0, f1);
  src_idx(s2, b1, low, e0, e1, f0, f1);
  return PostAxis{a0, b1 - a0 + 1, u0, e1 - u0 + 1};
}

// last output index of the tile that starts at o0
POST_FN int post_tile_last(int o0, int out) { return o0 + PTW - 1 < out ? o0 + PTW - 1 : out - 1; }

// the per-pixel kernel stages a tile's low-res patch in LDS when it fits
POST_FN bool post_staged(const PostAxis& y, const PostAxis& x) { return y.patch <= PR && x.patch <= PR; }

// does every strip of one axis fit the shared tables of sam_postprocess_sep_kernel
POST_FN bool post_sep_fits(int out, int crop, int low, int S) {
  const float s1 = post_scale(crop, out), s2 = post_scale(low, S);
  for (int o0 = 0; o0 < out; o0 += PTW) {
    const PostAxis t = post_axis(o0, post_tile_last(o0, out), s1, s2, crop, low);
    if (t.s1_count > PX1 || t.patch > PR) return false;
  }
  return true;
}

// the host's choice: the shared-table kernel when both axes fit (HGL_SAM_POST_SEP=0 overrules it)
POST_FN bool post_geometry_fits_sep(int H, int W, int hi, int wi, int hl, int wl, int S) {
  return post_sep_fits(W, wi, wl, S) && post_sep_fits(H, hi, hl, S);
}

#endif  // HGL_POST_GEOM_H
