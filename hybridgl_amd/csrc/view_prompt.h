// The geometry and colour rules of a visual prompt (include/hybridgl.h HglViewPrompt; view_prompt.hip: synth_views_prompt_kernel
// and its entry), once: plain functions that compile under g++ (the sanitizer harness tests/native/view_prompt_sanitize.cpp,
// which tests/test_sanitize_view_prompt.py holds against the numpy contract of tests/view_prompt_cases.py) and as
// __host__ __device__ code under hipcc.  Nothing here needs HIP when __HIPCC__ is absent.  Every decision -- which pixels a
// view looks at, which tap is read, which pixel carries the marker, what gray is -- is integer arithmetic, so the device and
// the contract agree on it exactly; the only floats are the tap coordinate (one fma, as ATen) and its two weights.
//
//   box      inclusive XYXY.  x1 < x0 or y1 < y0 as GIVEN is the empty box: its window is the frame, it gets no marker.
//            Otherwise each coordinate is clamped into the image; w = x1 - x0 + 1, h = y1 - y0 + 1.
//   window   m = max(w, h) * pad_permille / 1000.  Not square: origin (x0 - m, y0 - m), extent (w + 2m, h + 2m).  Square:
//            s = max(w, h) + 2m, origin (floor((x0 + x1 + 1 - s) / 2), floor((y0 + y1 + 1 - s) / 2)), extent (s, s).
//            The window may leave the image; a tap outside the image is never read and takes the fill colour.
//   marker   doubled coordinates about the box's centre, DX = 2x + 1 - (x0 + x1 + 1); inside(A, B) is
//            A > 0 && B > 0 && DX^2 B^2 + DY^2 A^2 <= A^2 B^2 in int64.  With H, W <= 8192, grow <= 4096, thickness <= 64 and
//            (x, y) a pixel of the image: |DX| < 2^14, A < 2^14.02, each product < 2^56.1, their sum < 2^57.1.
#ifndef HGL_VIEW_PROMPT_H
#define HGL_VIEW_PROMPT_H
#include <math.h>
#include <stdint.h>

#include "../../include/hybridgl.h"

#ifdef __HIPCC__
#define VP_FN static __host__ __device__ __forceinline__
#else
#define VP_FN static inline
#endif

constexpr int VP_MAX_SIDE = 8192, VP_MAX_PAD = 4000, VP_MAX_THICK = 64, VP_MAX_GROW = 4096;
enum { VP_WINDOW_FRAME = 0, VP_WINDOW_BOX = 1 };
enum { VP_LOCAL_FILL = 0, VP_LOCAL_KEEP = 1 };
enum { VP_GLOBAL_BLUR = 0, VP_GLOBAL_KEEP = 1, VP_GLOBAL_GRAY = 2, VP_GLOBAL_FILL = 3 };
enum { VP_MARKER_NONE = 0, VP_MARKER_ELLIPSE = 1, VP_MARKER_BOX = 2 };

VP_FN bool vp_needs_boxes(const HglViewPrompt& p) { return p.window == VP_WINDOW_BOX || p.marker != VP_MARKER_NONE; }
VP_FN bool vp_needs_blurred(const HglViewPrompt& p) { return p.global_bg == VP_GLOBAL_BLUR; }

// The entry's refusals, one message per rule; nullptr when the call is acceptable.
VP_FN const char* vp_refusal(const HglViewPrompt& p, int H, int W, bool have_blurred, bool have_boxes) {
  if (H < 1 || W < 1 || H > VP_MAX_SIDE || W > VP_MAX_SIDE) return "image side outside 1..8192";
  if (p.window != VP_WINDOW_FRAME && p.window != VP_WINDOW_BOX) return "window is not 0 (frame) or 1 (box)";
  if (p.pad_permille < 0 || p.pad_permille > VP_MAX_PAD) return "pad_permille outside 0..4000";
  if (p.square != 0 && p.square != 1) return "square is not 0 or 1";
  if (p.local_bg != VP_LOCAL_FILL && p.local_bg != VP_LOCAL_KEEP) return "local_bg is not 0 (fill) or 1 (keep)";
  for (int c = 0; c < 3; ++c)
    if (!(p.local_fill[c] - p.local_fill[c] == 0.f)) return "local_fill is not finite";
  if (p.global_bg < VP_GLOBAL_BLUR || p.global_bg > VP_GLOBAL_FILL) return "global_bg is not 0 (blur), 1 (keep), 2 (gray) or 3 (fill)";
  if (p.marker < VP_MARKER_NONE || p.marker > VP_MARKER_BOX) return "marker is not 0 (none), 1 (ellipse) or 2 (box)";
  if (p.thickness < 1 || p.thickness > VP_MAX_THICK) return "thickness outside 1..64";
  if (p.grow < 0 || p.grow > VP_MAX_GROW) return "grow outside 0..4096";
  if (vp_needs_blurred(p) && !have_blurred) return "a blur background needs the blurred image";
  if (vp_needs_boxes(p) && !have_boxes) return "a box window or a marker needs the boxes";
  return nullptr;
}

struct VpBox {
  int x0, y0, x1, y1;
  bool empty;
};
VP_FN int vp_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
VP_FN VpBox vp_box(int bx0, int by0, int bx1, int by1, int H, int W) {
  VpBox b;
  b.empty = bx1 < bx0 || by1 < by0;
  b.x0 = vp_clampi(bx0, 0, W - 1);
  b.x1 = vp_clampi(bx1, 0, W - 1);
  b.y0 = vp_clampi(by0, 0, H - 1);
  b.y1 = vp_clampi(by1, 0, H - 1);
  return b;
}
VP_FN VpBox vp_no_box() { return VpBox{0, 0, 0, 0, true}; }

VP_FN int vp_floor_half(int a) { return a >= 0 ? a / 2 : -((1 - a) / 2); }

struct VpWindow {
  int ox, oy, ew, eh;      // origin (may be negative), extent (>= 1)
};
VP_FN VpWindow vp_window(const HglViewPrompt& p, const VpBox& b, int H, int W) {
  if (p.window != VP_WINDOW_BOX || b.empty) return VpWindow{0, 0, W, H};
  const int w = b.x1 - b.x0 + 1, h = b.y1 - b.y0 + 1, l = w > h ? w : h;
  const int m = (int)((long long)l * p.pad_permille / 1000);
  if (!p.square) return VpWindow{b.x0 - m, b.y0 - m, w + 2 * m, h + 2 * m};
  const int s = l + 2 * m;
  return VpWindow{vp_floor_half(b.x0 + b.x1 + 1 - s), vp_floor_half(b.y0 + b.y1 + 1 - s), s, s};
}

// scale of one axis of the resampling
VP_FN float vp_scale(int extent, int res) { return (float)extent / (float)res; }

// output index -> the two source pixels of one axis and their weights: ATen's source index (one fma, clamped at 0) inside the
// window, the taps stop at extent - 1, the window's origin is added last
VP_FN void vp_tap(float scale, int dst, int extent, int origin, int& i0, int& i1, float& l0, float& l1) {
  float f = fmaf(scale, dst + 0.5f, -0.5f);
  f = f < 0.f ? 0.f : f;
  int a = (int)f;
  a = a < extent - 1 ? a : extent - 1;
  l1 = f - a;
  l0 = 1.f - l1;
  i0 = a + origin;
  i1 = a + (a < extent - 1 ? 1 : 0) + origin;
}

VP_FN bool vp_in_image(int x, int y, int H, int W) { return x >= 0 && x < W && y >= 0 && y < H; }

VP_FN bool vp_inside(long long DX, long long DY, long long A, long long B) {
  return A > 0 && B > 0 && DX * DX * (B * B) + DY * DY * (A * A) <= (A * A) * (B * B);
}

// does pixel (x, y) OF THE IMAGE carry the marker of box b
VP_FN bool vp_marker(const HglViewPrompt& p, const VpBox& b, int x, int y) {
  if (p.marker == VP_MARKER_NONE || b.empty) return false;
  const int g = p.grow, t = p.thickness;
  if (p.marker == VP_MARKER_BOX) {
    const bool outer = x >= b.x0 - g - t && x <= b.x1 + g + t && y >= b.y0 - g - t && y <= b.y1 + g + t;
    const bool inner = x >= b.x0 - g && x <= b.x1 + g && y >= b.y0 - g && y <= b.y1 + g;
    return outer && !inner;
  }
  const long long w = b.x1 - b.x0 + 1, h = b.y1 - b.y0 + 1;
  const long long DX = 2ll * x + 1 - (b.x0 + b.x1 + 1), DY = 2ll * y + 1 - (b.y0 + b.y1 + 1);
  return vp_inside(DX, DY, w + 2 * g + 2 * t, h + 2 * g + 2 * t) && !vp_inside(DX, DY, w + 2 * g, h + 2 * g);
}

VP_FN uint8_t vp_gray(int r, int g, int b) { return (uint8_t)((77 * r + 150 * g + 29 * b + 128) >> 8); }

#endif  // HGL_VIEW_PROMPT_H
