// Sanitizer harness for rle_select_plan (csrc/rle_group.h: the host side of hgl_rle_select_device), built by
// tests/test_sanitize_rle_select.py with g++ -fsanitize=address,undefined (and, without a sanitizer, by
// tests/test_rle_select_abi.py).  Reads a case file written by the test, one case per line:
//   <G> <S> <slot_words> <C> <has_keep> <has_nms> <slots> <out_slots> <table> <out_table> <4*G numbers: H W first max_keep per image>
// (the four addresses as numbers: the plan compares them and reads nothing through them) and prints one line per case: the
// return code, then for an accepted case "chunks blocks wide", per image "H W first max_keep", then S as the plan states it.
// The image rows live in a heap buffer of exactly 4*G words, so a read beyond them is a report.
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
    long long G, S, sw, C, has_keep, has_nms;
    unsigned long long addr[4];
    if (!(ss >> G >> S >> sw >> C >> has_keep >> has_nms >> addr[0] >> addr[1] >> addr[2] >> addr[3])) continue;
    const long long rows = G < 0 ? 0 : (G > 70 ? 70 : G);      // what the caller owns
    int64_t* images = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rows ? 4 * rows : 1));
    for (long long i = 0; i < 4 * rows; ++i) {
      long long v = 0;
      ss >> v;
      images[i] = v;
    }
    RleSelectPlan* plan = (RleSelectPlan*)malloc(sizeof(RleSelectPlan));
    char why[200] = "";
    // G beyond the limit is refused before a row is read: only RLE_GROUP_MAX + 1 .. 70 rows back such a case
    const int rc = rle_select_plan(images, (int)G, (int)S, sw, (int)C, has_keep != 0, has_nms != 0, (uintptr_t)addr[0], (uintptr_t)addr[1],
                                   (uintptr_t)addr[2], (uintptr_t)addr[3], plan, why, sizeof(why));
    if (rc != 0) {
      printf("%d %s\n", rc, why);
    } else {
      printf("0 %lld %lld %d", plan->chunks, plan->blocks, plan->wide ? 1 : 0);
      for (int g = 0; g < plan->s.G; ++g) printf(" | %d %d %d %d", plan->s.H[g], plan->s.W[g], plan->s.first[g], plan->s.max_keep[g]);
      printf(" | %d\n", plan->s.first[plan->s.G]);
    }
    free(plan);
    free(images);
  }
  return 0;
}
