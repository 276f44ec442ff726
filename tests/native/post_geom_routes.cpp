// What csrc/post_geom.h -- the header the two post-processing kernels and the host's choice between them are built from --
// answers for the geometries of tests/post_cases.py, as a stand-alone program: no GPU, no HIP, nothing loaded into Python.
// tests/test_post_cases_host.py builds it with g++ (-fsanitize=address,undefined) and holds its output against the Python
// restatement (post_cases.classify, sep_fits, src_idx), which the GPU tests rely on to know the route they pin.
//
//   post_geom_routes <requests.txt> <indices.bin>
// One request per line, one line of text on stdout per request, int16 index pairs (i0, i1) appended to indices.bin:
//   G H W ih iw S low   -> "G sep ntiles" and per tile (row-major) " by bx ph pw cols staged": the kernel the host would choose
//                          and what each tile of the launch touches
//   A out crop low S    -> "A fits nstrips" and per 64-wide strip " cols patch"; indices.bin: src_idx(crop / out, dst, crop) for
//                          every dst of the axis
//   L crop low S        -> "L crop"; indices.bin: src_idx(low / S, j, low) for every stage-1 index j below crop
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../hybridgl_amd/csrc/post_geom.h"

static void put_indices(std::vector<int16_t>& out, float scale, int n, int in_size) {
  for (int d = 0; d < n; ++d) {
    int i0, i1;
    float l0, l1;
    src_idx(scale, d, in_size, i0, i1, l0, l1);
    out.push_back((int16_t)i0);
    out.push_back((int16_t)i1);
  }
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s requests.txt indices.bin\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "r");
  FILE* bin = fopen(argv[2], "wb");
  if (!in || !bin) { fprintf(stderr, "cannot open the files\n"); return 2; }
  printf("C %d %d %d %d %d\n", PTW, PTH, PPX, PR, PX1);
  char line[256];
  std::vector<int16_t> idx;
  while (fgets(line, sizeof line, in)) {
    int v[6];
    idx.clear();
    if (sscanf(line, "G %d %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) == 6) {
      const int H = v[0], W = v[1], ih = v[2], iw = v[3], S = v[4], low = v[5];
      const float sy1 = post_scale(ih, H), sx1 = post_scale(iw, W), s2 = post_scale(low, S);
      const int ty = (H + PTH - 1) / PTH, tx = (W + PTW - 1) / PTW;
      printf("G %d %d", post_geometry_fits_sep(H, W, ih, iw, low, low, S) ? 1 : 0, ty * tx);
      for (int by = 0; by < ty; ++by)
        for (int bx = 0; bx < tx; ++bx) {
          const PostAxis y = post_axis(by * PTH, post_tile_last(by * PTH, H), sy1, s2, ih, low);
          const PostAxis x = post_axis(bx * PTW, post_tile_last(bx * PTW, W), sx1, s2, iw, low);
          printf(" %d %d %d %d %d %d", by, bx, y.patch, x.patch, x.s1_count, post_staged(y, x) ? 1 : 0);
        }
      printf("\n");
    } else if (sscanf(line, "A %d %d %d %d", &v[0], &v[1], &v[2], &v[3]) == 4) {
      const int out = v[0], crop = v[1], low = v[2], S = v[3];
      const float s1 = post_scale(crop, out), s2 = post_scale(low, S);
      printf("A %d %d", post_sep_fits(out, crop, low, S) ? 1 : 0, (out + PTW - 1) / PTW);
      for (int o0 = 0; o0 < out; o0 += PTW) {
        const PostAxis t = post_axis(o0, post_tile_last(o0, out), s1, s2, crop, low);
        printf(" %d %d", t.s1_count, t.patch);
      }
      printf("\n");
      put_indices(idx, s1, out, crop);
    } else if (sscanf(line, "L %d %d %d", &v[0], &v[1], &v[2]) == 3) {
      printf("L %d\n", v[0]);
      put_indices(idx, post_scale(v[1], v[2]), v[0], v[1]);
    } else {
      fprintf(stderr, "bad request: %s", line);
      return 2;
    }
    if (!idx.empty() && fwrite(idx.data(), sizeof(int16_t), idx.size(), bin) != idx.size()) return 3;
  }
  fclose(in);
  return fclose(bin) == 0 ? 0 : 3;
}
