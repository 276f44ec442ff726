// The direction weight of a heat-map column (gen_dir_mask, utils.py:135-161), shared by the scoring tail (csrc/scoring.hip: the
// coherence pooling multiplies a map with it) and the heat-map painter (csrc/rle_paint.hip: hgl_heat_paint_device shows the same
// product).  One definition, so that the picture shows the very bits the scorer used.
#ifndef HGL_DIR_RAMP_H
#define HGL_DIR_RAMP_H
#include "hgl_common.h"

namespace {

// torch.linspace(start,end,steps)[i] in fp32 (ATen RangeFactories: symmetric evaluation)
__device__ __forceinline__ float linspace_at(float start, float end, int steps, int i) {
  if (steps == 1) return start;
  const float step = (end - start) / (float)(steps - 1);
  const int half = steps / 2;
  return i < half ? fmaf(step, (float)i, start) : fmaf(-step, (float)(steps - i - 1), end);  // fmas, as ATen
}

// gen_dir_mask column weight (utils.py:135-161): 0 none, 1 left, 2 right, 3 middle
__device__ __forceinline__ float dir_weight(int dirflag, int x, int W) {
  switch (dirflag) {
    case 1: return linspace_at(1.f, 0.f, W, x);
    case 2: return linspace_at(0.f, 1.f, W, x);
    case 3: {
      const int w1 = W / 2;
      return x < w1 ? linspace_at(0.f, 1.f, w1, x) : linspace_at(1.f, 0.f, W - w1, x - w1);
    }
    default: return 1.f;
  }
}

}  // namespace
#endif  // HGL_DIR_RAMP_H
