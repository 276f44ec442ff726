// Sanitizer harness for rle_match_plan (csrc/rle_group.h: the host side of hgl_rle_match_device), built by
// tests/test_sanitize_rle_match.py with g++ -fsanitize=address,undefined.  Reads a case file written by the test, one case per
// line:   <G> <Sa> <Sb> <inter_elems> <5*G numbers: H W first_a first_b offset per image>
// and prints one line per case: the return code, then for an accepted case "tiles blocks_a blocks_b words_a words_b pairs splits"
// and per image "H W first_a first_b off word0_a word0_b tile0 blk0_a blk0_b pair0".  The image rows live in a heap buffer of exactly 5*G
// words, so a read beyond them is a report.
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
    long long G, Sa, Sb, elems;
    if (!(ss >> G >> Sa >> Sb >> elems)) continue;
    const long long rows = G < 0 ? 0 : (G > 70 ? 70 : G);      // what the caller owns
    int64_t* images = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rows ? 5 * rows : 1));
    for (long long i = 0; i < 5 * rows; ++i) {
      long long v = 0;
      ss >> v;
      images[i] = v;
    }
    RleMatchPlan* plan = (RleMatchPlan*)malloc(sizeof(RleMatchPlan));
    char why[200] = "";
    // G beyond the limit is refused before a row is read: only RLE_GROUP_MAX + 1 .. 70 rows back such a case
    const int rc = rle_match_plan(images, (int)G, (int)Sa, (int)Sb, elems, plan, why, sizeof(why));
    if (rc != 0) {
      printf("%d %s\n", rc, why);
    } else {
      const RleMatch& m = plan->p.m;
      printf("0 %lld %lld %lld %lld %lld %lld %d", plan->p.tiles, plan->a.blocks, plan->b.blocks, plan->a.words, plan->b.words, plan->p.pairs,
             plan->p.splits);
      for (int g = 0; g < m.G; ++g)
        printf(" | %d %d %d %d %lld %u %u %u %u %u %lld", m.H[g], m.W[g], m.first_a[g], m.first_b[g], m.off[g], m.word0_a[g], m.word0_b[g],
               m.tile0[g], plan->a.blk0[g], plan->b.blk0[g], m.pair0[g]);
      printf(" | %d %d\n", m.first_a[m.G], m.first_b[m.G]);
    }
    free(plan);
    free(images);
  }
  return 0;
}
