// Sanitizer harness for heat_paint_plan (csrc/rle_group.h: the host side of hgl_heat_paint_device), built by
// tests/test_sanitize_heat_paint.py with g++ -fsanitize=address,undefined (and, without a sanitizer, by
// tests/test_heat_paint_abi.py).  Reads a case file written by the test, one case per line:
//   <M> <heat_elems> <canvas_pixels> <base> <out> <6*M numbers: H W dirflag heat-element base-pixel canvas-pixel per map>
// (the two addresses as numbers: the plan compares them and reads nothing through them) and prints one line per case: the
// return code, then for an accepted case the workgroups of a launch, per map "H W dirflag heat0 base0 pix0 blk0", then the
// workgroups again as the plan's last blk0 states them.  The rows live in a heap buffer of exactly 6*M words, so a read beyond
// them is a report.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "../../hybridgl_amd/csrc/rle_group.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    long long M, heat, canvas;
    unsigned long long addr[2];
    if (!(ss >> M >> heat >> canvas >> addr[0] >> addr[1])) continue;
    const long long rows = M < 0 ? 0 : (M > 70 ? 70 : M);      // what the caller owns
    int64_t* maps = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rows ? 6 * rows : 1));
    for (long long i = 0; i < 6 * rows; ++i) {
      long long v = 0;
      ss >> v;
      maps[i] = v;
    }
    HeatPaintPlan* plan = (HeatPaintPlan*)malloc(sizeof(HeatPaintPlan));
    char why[200] = "";
    // M beyond the limit is refused before a row is read: only RLE_GROUP_MAX + 1 .. 70 rows back such a case
    const int rc = heat_paint_plan(maps, (int)M, heat, canvas, (uintptr_t)addr[0], (uintptr_t)addr[1], plan, why, sizeof(why));
    if (rc != 0) {
      printf("%d %s\n", rc, why);
    } else {
      printf("0 %lld", plan->blocks);
      for (int m = 0; m < plan->p.M; ++m)
        printf(" | %d %d %d %lld %lld %lld %u", plan->p.H[m], plan->p.W[m], (int)plan->p.dirflag[m], plan->p.heat0[m], plan->p.base0[m],
               plan->p.pix0[m], plan->p.blk0[m]);
      printf(" | %u\n", plan->p.blk0[plan->p.M]);
    }
    free(plan);
    free(maps);
  }
  return 0;
}
