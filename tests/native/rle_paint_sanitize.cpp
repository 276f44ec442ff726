// Sanitizer harness for rle_paint_plan (csrc/rle_group.h: the host side of hgl_rle_paint_device), built by
// tests/test_sanitize_rle_paint.py with g++ -fsanitize=address,undefined (and, without a sanitizer, by
// tests/test_rle_paint_abi.py).  Reads a case file written by the test, one case per line:
//   <G> <S> <K> <slot_words> <canvas_pixels> <base> <out> <5*G numbers: H W first-entry first-position pixel-offset per image>
// (the two addresses as numbers: the plan compares them and reads nothing through them) and prints one line per case: the
// return code, then for an accepted case "tiles words blocks", per image "H W first word0 tile0 pix0 entry0 entries", then K as
// the plan states it.  The image rows live in a heap buffer of exactly 5*G words, so a read beyond them is a report.
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
    long long G, S, K, sw, canvas;
    unsigned long long addr[2];
    if (!(ss >> G >> S >> K >> sw >> canvas >> addr[0] >> addr[1])) continue;
    const long long rows = G < 0 ? 0 : (G > 70 ? 70 : G);      // what the caller owns
    int64_t* images = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rows ? 5 * rows : 1));
    for (long long i = 0; i < 5 * rows; ++i) {
      long long v = 0;
      ss >> v;
      images[i] = v;
    }
    RlePaintPlan* plan = (RlePaintPlan*)malloc(sizeof(RlePaintPlan));
    char why[200] = "";
    // G beyond the limit is refused before a row is read: only RLE_GROUP_MAX + 1 .. 70 rows back such a case
    const int rc = rle_paint_plan(images, (int)G, (int)S, (int)K, sw, canvas, (uintptr_t)addr[0], (uintptr_t)addr[1], plan, why, sizeof(why));
    if (rc != 0) {
      printf("%d %s\n", rc, why);
    } else {
      printf("0 %lld %lld %lld", plan->tiles, plan->pick.pos.words, plan->pick.pos.blocks);
      for (int g = 0; g < plan->p.G; ++g)
        printf(" | %d %d %d %u %u %lld %d %d", plan->p.H[g], plan->p.W[g], plan->p.first[g], plan->p.word0[g], plan->p.tile0[g],
               plan->p.pix0[g], plan->pick.entry0[g], plan->pick.entries[g]);
      printf(" | %d\n", plan->p.first[plan->p.G]);
    }
    free(plan);
    free(images);
  }
  return 0;
}
