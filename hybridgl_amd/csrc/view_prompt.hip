// hgl_synthesize_views_prompt: the two CLIP views of every proposal under a visual prompt (include/hybridgl.h HglViewPrompt).
// The rules are view_prompt.h; the launch shape, the tap arithmetic and the blend / normalise expressions are those of
// synth_views_kernel (scoring.hip), which the pipeline keeps calling for the default prompt: at that prompt this kernel writes
// the same bits (tests/test_gpu_view_prompt.py).
#include "hgl_common.h"
#include "view_prompt.h"

namespace {

// One thread per output pixel of one mask: both views, three channels, stores coalesced along ox.  The prompt arrives by value
// (kernel arguments: scalar registers), so every branch on one of its fields is wave-uniform; the window depends on the mask
// alone.  A box window makes the taps of a mask fall inside its box (plus margin): only that part of the mask and the image is
// read.  Nothing outside the image is read.
__global__ __launch_bounds__(256) void synth_views_prompt_kernel(
    const uint8_t* __restrict__ sam_img, const uint8_t* __restrict__ blurred, const float* __restrict__ image_norm,
    const uint8_t* __restrict__ masks, const int32_t* __restrict__ boxes, int N, int H, int W, int res, const HglViewPrompt p,
    float* __restrict__ local_imgs, float* __restrict__ global_imgs) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long total = (long long)N * res * res;
  if (i >= total) return;
  const int ox = (int)(i % res), oy = (int)((i / res) % res), n = (int)(i / ((long long)res * res));
  VpBox b = vp_no_box();
  if (vp_needs_boxes(p)) b = vp_box(boxes[4 * n], boxes[4 * n + 1], boxes[4 * n + 2], boxes[4 * n + 3], H, W);
  const VpWindow win = vp_window(p, b, H, W);
  int ty[2], tx[2];
  float ly0, ly1, lx0, lx1;
  vp_tap(vp_scale(win.eh, res), oy, win.eh, win.oy, ty[0], ty[1], ly0, ly1);
  vp_tap(vp_scale(win.ew, res), ox, win.ew, win.ox, tx[0], tx[1], lx0, lx1);
  const long long HW = (long long)H * W;
  const uint8_t* m = masks + (long long)n * HW;
  // per tap (row-major: 00, 01, 10, 11): its pixel, whether it lies in the image, in the mask, on the marker.  Pixel 0 stands in
  // for a tap outside the image, so that every load below has a valid address and none waits behind a lane's branch: what it
  // brings is not used.  The branches that remain are on the prompt alone.
  long long t[4];
  bool in[4], fg[4], mk[4];
  uint8_t gy[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = ty[k >> 1], x = tx[k & 1];
    in[k] = vp_in_image(x, y, H, W);
    t[k] = in[k] ? (long long)y * W + x : 0;
    const uint8_t mv = m[t[k]];
    fg[k] = in[k] && mv != 0;
    mk[k] = in[k] && vp_marker(p, b, x, y);
    if (p.global_bg == VP_GLOBAL_GRAY) gy[k] = vp_gray(sam_img[t[k] * 3], sam_img[t[k] * 3 + 1], sam_img[t[k] * 3 + 2]);
  }
  const float in_mean[3] = {0.485f, 0.456f, 0.406f};                   // Hybridgl_main.py:117
  const float in_std[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* im = image_norm + (long long)c * HW;
    float l[4], g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float iv = im[t[k]];
      l[k] = (fg[k] || (in[k] && p.local_bg == VP_LOCAL_KEEP)) ? iv : p.local_fill[c];
      // one byte per tap and channel: the image inside the mask, the blurred image outside it when the background is the blur
      const uint8_t* src = (p.global_bg == VP_GLOBAL_BLUR && !fg[k]) ? blurred : sam_img;
      const uint8_t sv = src[t[k] * 3 + c];
      const uint8_t bg = p.global_bg == VP_GLOBAL_GRAY ? gy[k] : (p.global_bg == VP_GLOBAL_FILL ? p.global_fill[c] : sv);
      const uint8_t v = mk[k] ? p.marker_rgb[c] : (fg[k] ? sv : (in[k] ? bg : p.global_fill[c]));
      g[k] = (float)v / 255.f;
    }
    const float l00 = l[0], l01 = l[1], l10 = l[2], l11 = l[3];
    const float g00 = g[0], g01 = g[1], g10 = g[2], g11 = g[3];
    const float lv = ly0 * (lx0 * l00 + lx1 * l01) + ly1 * (lx0 * l10 + lx1 * l11);
    const float gv = ly0 * (lx0 * g00 + lx1 * g01) + ly1 * (lx0 * g10 + lx1 * g11);
    const long long o = (((long long)n * 3 + c) * res + oy) * res + ox;
    local_imgs[o] = lv;
    global_imgs[o] = (gv - in_mean[c]) / in_std[c];
  }
}

}  // namespace

extern "C" {

int hgl_synthesize_views_prompt(const uint8_t* sam_img, const uint8_t* blurred, const float* image_norm, const uint8_t* masks,
                                const int32_t* boxes_xyxy, int N, int H, int W, int res, const HglViewPrompt* prompt,
                                float* local_imgs, float* global_imgs, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(sam_img && image_norm && masks && prompt && local_imgs && global_imgs, "synthesize_views_prompt: null argument");
  HGL_REQUIRE(N > 0 && res > 0, "synthesize_views_prompt: bad shape");
  const char* why = vp_refusal(*prompt, H, W, blurred != nullptr, boxes_xyxy != nullptr);
  HGL_REQUIRE(why == nullptr, "synthesize_views_prompt: %s", why);
  const long long total = (long long)N * res * res;
  HGL_REQUIRE((total + 255) / 256 <= 0x7fffffffll, "synthesize_views_prompt: %lld output pixels are too many", total);
  hipLaunchKernelGGL(synth_views_prompt_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sam_img,
                     blurred, image_norm, masks, boxes_xyxy, N, H, W, res, *prompt, local_imgs, global_imgs);
  return hgl_check_launch("synthesize_views_prompt");
}

}  // extern "C"
