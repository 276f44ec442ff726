// Sanitizer harness for rle_group_plan and rle_tiles (csrc/rle_group.h: the host side of the RLE entries), built by
// tests/test_sanitize_rle_group.py with g++ -fsanitize=address,undefined.  Reads a case file written by the test, one case per
// line:   <G> <S> <base address> <masks_bytes> <4*G numbers: H W first offset per image>
// and prints one line per case: the return code, then for an accepted case the number of tiles, the wide bits and per image
// "H W first tile0 off".  The image rows live in a heap buffer of exactly 4*G words, so a read beyond them is a report.
// A line   T <H> <W> <base address>   is a case of rle_tiles and prints "T wide HW64 col_tiles row_tiles".
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../hybridgl_amd/csrc/rle_group.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    if (line.rfind("T ", 0) == 0) {
      char tag;
      long long H, W, base;
      ss >> tag >> H >> W >> base;
      const RleTiles t = rle_tiles(H, W, (uintptr_t)base);
      printf("T %d %d %d %d\n", (int)t.wide, t.HW64, t.col_tiles, t.row_tiles);
      continue;
    }
    long long G, S, base, bytes;
    if (!(ss >> G >> S >> base >> bytes)) continue;
    const long long rows = G < 0 ? 0 : (G > 70 ? 70 : G);      // what the caller owns
    int64_t* images = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rows ? 4 * rows : 1));
    for (long long i = 0; i < 4 * rows; ++i) {
      long long v = 0;
      ss >> v;
      images[i] = v;
    }
    RleGroup grp;
    long long tiles = -1;
    char why[200] = "";
    // G beyond the limit is refused before a row is read: only RLE_GROUP_MAX + 1 .. 70 rows back such a case
    const int rc = rle_group_plan(images, (int)G, (int)S, (uintptr_t)base, bytes, &grp, &tiles, why, sizeof(why));
    if (rc != 0) {
      printf("%d %s\n", rc, why);
    } else {
      printf("0 %lld %llu", tiles, grp.wide);
      for (int g = 0; g < grp.G; ++g) printf(" | %d %d %d %u %lld", grp.H[g], grp.W[g], grp.first[g], grp.tile0[g], grp.off[g]);
      printf("\n");
    }
    free(images);
  }
  return 0;
}
