// The rules of a visual prompt (hybridgl_amd/csrc/view_prompt.h: refusals, box clamping, window, taps, marker bands, gray) as a
// stand-alone program for g++ -fsanitize=address,undefined (tests/test_sanitize_view_prompt.py).  One case per input line:
//   H W res window pad square local_bg global_bg marker thickness grow fill_nan have_blurred have_boxes x0 y0 x1 y1 K (x y r g b)*K
// One line out: `-1 message` for a refused call, else
//   0 empty x0 y0 x1 y1 | ox oy ew eh | taps of output 0, res / 2, res - 1 on x then on y: i0 i1 bits(l0) bits(l1) | marker gray per pixel
// which the test compares with tests/view_prompt_cases.py harness_want, line for line.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../hybridgl_amd/csrc/view_prompt.h"

static unsigned bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    int H, W, res, fill_nan, have_blurred, have_boxes, bx[4], K;
    HglViewPrompt p;
    std::memset(&p, 0, sizeof p);
    ss >> H >> W >> res >> p.window >> p.pad_permille >> p.square >> p.local_bg >> p.global_bg >> p.marker >> p.thickness >> p.grow >>
        fill_nan >> have_blurred >> have_boxes >> bx[0] >> bx[1] >> bx[2] >> bx[3] >> K;
    if (!ss || K < 0) return 3;
    p.local_fill[0] = 0.48145466f;
    p.local_fill[1] = fill_nan ? NAN : 0.4578275f;
    p.local_fill[2] = 0.40821073f;
    std::vector<int> px(5 * (size_t)K);
    for (int& v : px) ss >> v;
    if (!ss) return 3;
    const char* why = vp_refusal(p, H, W, have_blurred != 0, have_boxes != 0);
    if (why) {
      std::printf("-1 %s\n", why);
      continue;
    }
    const VpBox shown = vp_box(bx[0], bx[1], bx[2], bx[3], H, W);
    const VpBox b = vp_needs_boxes(p) ? shown : vp_no_box();
    const VpWindow win = vp_window(p, b, H, W);
    std::printf("0 %d %d %d %d %d | %d %d %d %d |", (int)shown.empty, shown.x0, shown.y0, shown.x1, shown.y1, win.ox, win.oy, win.ew, win.eh);
    const int extent[2] = {win.ew, win.eh}, origin[2] = {win.ox, win.oy}, at[3] = {0, res / 2, res - 1};
    for (int a = 0; a < 2; ++a)
      for (int o : at) {
        int i0, i1;
        float l0, l1;
        vp_tap(vp_scale(extent[a], res), o, extent[a], origin[a], i0, i1, l0, l1);
        std::printf(" %d %d %u %u", i0, i1, bits(l0), bits(l1));
      }
    std::printf(" |");
    for (int k = 0; k < K; ++k) {
      const int* q = &px[5 * (size_t)k];
      const bool on = vp_in_image(q[0], q[1], H, W) && vp_marker(p, b, q[0], q[1]);
      std::printf(" %d %d", (int)on, (int)vp_gray(q[2], q[3], q[4]));
    }
    std::printf("\n");
  }
  return 0;
}
