// Sanitizer harness for rle_nms_plan (csrc/rle_group.h: the host side of hgl_rle_nms_device), built by
// tests/test_sanitize_rle_nms.py with g++ -fsanitize=address,undefined.  Reads a case file written by the test, one case per
// line:   <G> <S> <3*G numbers: H W first per image>
// and prints one line per case: the return code, then for an accepted case "tiles blocks words pairs splits sup_words" and per
// image "H W first word0 tile0 blk0 pair0 sup0", then S as the plan states it.  The image rows live in a heap buffer of exactly
// 3*G words, so a read beyond them is a report.
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
    long long G, S;
    if (!(ss >> G >> S)) continue;
    const long long rows = G < 0 ? 0 : (G > 70 ? 70 : G);      // what the caller owns
    int64_t* images = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rows ? 3 * rows : 1));
    for (long long i = 0; i < 3 * rows; ++i) {
      long long v = 0;
      ss >> v;
      images[i] = v;
    }
    RleNmsPlan* plan = (RleNmsPlan*)malloc(sizeof(RleNmsPlan));
    char why[200] = "";
    // G beyond the limit is refused before a row is read: only RLE_GROUP_MAX + 1 .. 70 rows back such a case
    const int rc = rle_nms_plan(images, (int)G, (int)S, plan, why, sizeof(why));
    if (rc != 0) {
      printf("%d %s\n", rc, why);
    } else {
      const RlePairs& p = plan->p;
      const RleSet& set = plan->set;
      printf("0 %lld %lld %lld %lld %d %lld", p.tiles, set.blocks, set.words, p.pairs, p.splits, plan->sup_words);
      for (int g = 0; g < plan->n.G; ++g)
        printf(" | %d %d %d %u %u %u %lld %lld", p.m.H[g], p.m.W[g], plan->n.first[g], p.m.word0_a[g], p.m.tile0[g], set.blk0[g],
               plan->n.pair0[g], plan->n.sup0[g]);
      // both sides of the pair count are the one set
      int same = p.m.G == set.G && p.m.first_a[p.m.G] == set.first[set.G] && p.m.first_a[p.m.G] == p.m.first_b[p.m.G];
      for (int g = 0; g < plan->n.G; ++g)
        same = same && p.m.first_a[g] == set.first[g] && p.m.first_a[g] == p.m.first_b[g] && p.m.word0_a[g] == set.word0[g] &&
               p.m.word0_a[g] == p.m.word0_b[g];
      printf(" | %d %d\n", plan->n.first[plan->n.G], same);
    }
    free(plan);
    free(images);
  }
  return 0;
}
