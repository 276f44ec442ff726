// Sanitizer harness for rle_merge_plan (csrc/rle_group.h: the host side of hgl_rle_merge_device), built by
// tests/test_sanitize_rle_merge.py with g++ -fsanitize=address,undefined.  Reads a case file written by the test, one case per
// line:   <G> <Ssrc> <S> <M> <4*G numbers: H W first_src first_out per image>
// and prints one line per case: the return code, then for an accepted case "blocks_src words_src words_out" and per image
// "H W first_src first_out word0_src word0_out blk0" (the merge kernel's struct and the RleSet it was filled from must agree, or the line says
// "split").  The image rows live in a heap buffer of exactly 4*G words, so a read beyond them is a report.
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
    long long G, Ssrc, S, M;
    if (!(ss >> G >> Ssrc >> S >> M)) continue;
    const long long rows = G < 0 ? 0 : (G > 70 ? 70 : G);      // what the caller owns
    int64_t* images = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rows ? 4 * rows : 1));
    for (long long i = 0; i < 4 * rows; ++i) {
      long long v = 0;
      ss >> v;
      images[i] = v;
    }
    RleMergePlan* plan = (RleMergePlan*)malloc(sizeof(RleMergePlan));
    char why[200] = "";
    // G beyond the limit is refused before a row is read: only RLE_GROUP_MAX + 1 .. 70 rows back such a case
    const int rc = rle_merge_plan(images, (int)G, (int)Ssrc, (int)S, (int)M, plan, why, sizeof(why));
    if (rc != 0) {
      printf("%d %s\n", rc, why);
    } else {
      const RleMerge& m = plan->m;
      const RleSet& p = plan->src;
      printf("0 %lld %lld %lld", p.blocks, p.words, plan->words_out);
      bool split = p.G != m.G;
      for (int g = 0; g < m.G; ++g) {
        split = split || p.H[g] != m.H[g] || p.W[g] != m.W[g] || p.first[g] != m.first_src[g] || p.word0[g] != m.word0_src[g];
        printf(" | %d %d %d %d %u %llu %u", m.H[g], m.W[g], m.first_src[g], m.first_out[g], m.word0_src[g], m.word0_out[g], p.blk0[g]);
      }
      printf(" | %d %d%s\n", m.first_src[m.G], m.first_out[m.G], split ? " split" : "");
    }
    free(plan);
    free(images);
  }
  return 0;
}
