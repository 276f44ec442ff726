// Sanitizer harness for the polygon walk (csrc/poly_walk.h: what the kernel of rle_poly.hip runs per step), built by
// tests/test_sanitize_poly_walk.py with g++ -fsanitize=address,undefined.  It rasterises the way the device does and in the
// order least like the host codec's: every (edge, step) is evaluated on its own, edges and steps in REVERSE, every crossing
// XORs one bit of a plane of H*W + 1 bits (the position H*W dropped), the polygon's mask is the prefix parity of the plane, and
// the polygons join in two planes once / more.
// Input (argv[1]), one case after the other:   <H> <W> <polygons>  then per polygon  <k> <2k coordinates, hex floats>
// Output (argv[2]), binary, per case: the bits of "covered exactly once" in column-major order, ceil(H*W/8) bytes LSB first,
// the same of "covered at least once", and the sum of the polygons' own areas as int64.
// The planes are heap buffers of exactly the words the kernel owns, so a toggle outside them is a report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hybridgl_amd/csrc/poly_walk.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int H, W, np;
  long long cases = 0;
  while (fscanf(in, "%d %d %d", &H, &W, &np) == 3) {
    const unsigned HW = (unsigned)H * (unsigned)W, nw = HW / 32u + 1u;
    std::vector<uint32_t> once(nw, 0u), more(nw, 0u);
    long long area_sum = 0;
    for (int i = 0; i < np; ++i) {
      int k = 0;
      if (fscanf(in, "%d", &k) != 1 || k < 1) return 3;
      double* xy = (double*)malloc(sizeof(double) * 2 * (size_t)k);
      for (int c = 0; c < 2 * k; ++c) {
        if (fscanf(in, "%lf", &xy[c]) != 1) return 3;
        if (!poly_coord_ok(xy[c])) return 4;
      }
      uint32_t* T = (uint32_t*)calloc(nw, sizeof(uint32_t));
      for (int j = k - 1; j >= 0; --j) {
        const PolyEdge e = poly_edge_of(xy, k, j);
        for (int d = e.n; d >= 0; --d) {
          unsigned pos;
          if (!poly_step(xy, k, j, e, d, H, W, &pos)) continue;
          if (pos > HW) return 5;
          if (pos < HW) T[pos >> 5] ^= 1u << (pos & 31u);
        }
      }
      unsigned run = 0;
      for (unsigned p = 0; p < HW; ++p) {
        run ^= (T[p >> 5] >> (p & 31u)) & 1u;
        if (!run) continue;
        ++area_sum;
        const uint32_t bit = 1u << (p & 31u);
        more[p >> 5] |= once[p >> 5] & bit;
        once[p >> 5] ^= bit;
      }
      free(T);
      free(xy);
    }
    const size_t nbytes = ((size_t)HW + 7) / 8;
    for (int rule = 0; rule < 2; ++rule) {
      std::vector<uint8_t> bytes(nbytes, 0);
      for (unsigned p = 0; p < HW; ++p) {
        const uint32_t o = (once[p >> 5] >> (p & 31u)) & 1u, m = (more[p >> 5] >> (p & 31u)) & 1u;
        if (rule ? (o | m) : (o & ~m)) bytes[p >> 3] |= (uint8_t)(1u << (p & 7u));
      }
      if (nbytes && fwrite(bytes.data(), 1, nbytes, out) != nbytes) return 6;
    }
    const int64_t a = area_sum;
    if (fwrite(&a, sizeof(a), 1, out) != 1) return 6;
    ++cases;
  }
  fclose(in);
  fclose(out);
  printf("%lld\n", cases);
  return 0;
}
