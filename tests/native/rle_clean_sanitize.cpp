// Sanitizer harness for the host-callable side of hgl_rle_clean_device: rle_clean_plan (csrc/rle_group.h) and the segment logic
// of csrc/ccl_runs.h, the functions the kernel of csrc/rle_clean.hip is made of, walked here by one thread with a serial
// union-find (link by minimum, as the kernel's).  Built by tests/test_sanitize_rle_clean.py with g++ -fsanitize=address,undefined
// (and, without a sanitizer, by tests/test_rle_clean_abi.py).  Reads a case file written by the test, one case per line:
//   plan <G> <S> <slot_words> <out_slot_words> <area_thresh> <modes> <seg_cap> <3*G numbers: H W first per image>
//     -> the return code and the reason, or "0 <cap> <plane words> | H W first ... | S"
//   mask <H> <W> <area_thresh> <modes> <seg_cap> <W * ceil(H/64) column words, hex>
//     -> "<code> <changed> <area> <x0> <y0> <x1> <y1> <the cleaned column words, hex>" (code 3: more than seg_cap segments)
// The image rows, the plane, the per-word ranks and the segment arrays live in heap buffers of exactly their size, so a step
// beyond them is a report.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../hybridgl_amd/csrc/rle_group.h"
#include "../../hybridgl_amd/csrc/ccl_runs.h"

static int uf_find(int* L, int x) {
  while (L[x] != x) {
    L[x] = L[L[x]];
    x = L[x];
  }
  return x;
}

// one pass of the kernel over the plane P: -1 over the cap, 0 nothing small, 1 a small component found
static int clean_pass(unsigned long long* P, int H, int W, bool holes, int thresh, long long cap) {
  const int HW64 = (H + 63) / 64;
  const long long Q = (long long)W * HW64;
  unsigned* wb = (unsigned*)malloc(sizeof(unsigned) * (size_t)Q);
  unsigned nseg = 0;
  for (long long q = 0; q < Q; ++q) {
    wb[q] = nseg;
    nseg += (unsigned)__builtin_popcountll(ccl_word_starts(P + (q / HW64) * HW64, H, (int)(q % HW64), holes));
  }
  if ((long long)nseg > cap) { free(wb); return -1; }
  if (nseg == 0) { free(wb); return 0; }
  int* y0 = (int*)malloc(sizeof(int) * nseg);
  int* y1 = (int*)malloc(sizeof(int) * nseg);
  int* parent = (int*)malloc(sizeof(int) * nseg);
  unsigned* area = (unsigned*)malloc(sizeof(unsigned) * nseg);
  unsigned* key = (unsigned*)malloc(sizeof(unsigned) * nseg);
  for (long long q = 0; q < Q; ++q) {
    const int x = (int)(q / HW64), j = (int)(q % HW64);
    const unsigned long long* col = P + (long long)x * HW64;
    unsigned long long st = ccl_word_starts(col, H, j, holes);
    int id = (int)wb[q];
    while (st) {
      const int b = __builtin_ctzll(st);
      st &= st - 1ull;
      y0[id] = 64 * j + b;
      y1[id] = ccl_seg_end(col, H, HW64, holes, j, b);
      parent[id] = id;
      area[id] = (unsigned)(y1[id] - y0[id] + 1);
      key[id] = ccl_key(y0[id], x, W);
      ++id;
    }
  }
  for (int x = 0; x + 1 < W; ++x) {
    int a = (int)wb[(long long)x * HW64];
    const int a_end = (int)wb[(long long)(x + 1) * HW64];
    int b = a_end;
    const int b_end = x + 2 < W ? (int)wb[(long long)(x + 2) * HW64] : (int)nseg;
    while (a < a_end && b < b_end) {
      if (ccl_touch(y0[a], y1[a], y0[b], y1[b])) {
        int ra = uf_find(parent, a), rb = uf_find(parent, b);
        if (ra != rb) parent[ra > rb ? ra : rb] = ra > rb ? rb : ra;
      }
      if (ccl_first_moves(y1[a], y1[b])) ++a; else ++b;
    }
  }
  for (unsigned i = 0; i < nseg; ++i) {
    const int r = uf_find(parent, (int)i);
    if (r != (int)i) {
      parent[i] = r;
      area[r] += area[i];
      key[r] = key[r] < key[i] ? key[r] : key[i];
    }
  }
  unsigned n_small = 0, n_large = 0;
  unsigned long long best = 0;
  for (unsigned i = 0; i < nseg; ++i) {
    if (parent[i] != (int)i) continue;
    if (ccl_small(area[i], thresh)) ++n_small; else ++n_large;
    const unsigned long long r = ccl_rank(area[i], key[i]);
    best = best > r ? best : r;
  }
  if (n_small) {
    for (long long q = 0; q < Q; ++q) {
      const int x = (int)(q / HW64), j = (int)(q % HW64);
      int lo = (int)wb[q];
      const int hi = q + 1 < Q ? (int)wb[q + 1] : (int)nseg;
      if (lo > (int)wb[(long long)x * HW64] && y1[lo - 1] >= 64 * j) --lo;
      unsigned long long m = 0;
      for (int id = lo; id < hi; ++id) {
        const int r = parent[id];
        if (ccl_flips(holes, area[r], key[r], thresh, n_large != 0, best)) m |= ccl_seg_bits(y0[id], y1[id], j);
      }
      if (m) P[q] = holes ? (P[q] | m) : (P[q] & ~m);
    }
  }
  free(wb); free(y0); free(y1); free(parent); free(area); free(key);
  return n_small ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string kind;
    if (!(ss >> kind)) continue;
    if (kind == "plan") {
      long long G, S, sw, osw, thresh, modes, cap;
      if (!(ss >> G >> S >> sw >> osw >> thresh >> modes >> cap)) continue;
      const long long rows = G < 0 ? 0 : (G > 70 ? 70 : G);      // what the caller owns
      int64_t* images = (int64_t*)malloc(sizeof(int64_t) * (size_t)(rows ? 3 * rows : 1));
      for (long long i = 0; i < 3 * rows; ++i) {
        long long v = 0;
        ss >> v;
        images[i] = v;
      }
      RleCleanPlan* plan = (RleCleanPlan*)malloc(sizeof(RleCleanPlan));
      char why[200] = "";
      const int rc = rle_clean_plan(images, (int)G, (int)S, sw, osw, (int)thresh, (int)modes, cap, plan, why, sizeof(why));
      if (rc != 0) {
        printf("%d %s\n", rc, why);
      } else {
        printf("0 %lld %lld", plan->cap, plan->set.words);
        for (int g = 0; g < plan->set.G; ++g) printf(" | %d %d %d", plan->set.H[g], plan->set.W[g], plan->set.first[g]);
        printf(" | %d\n", plan->set.first[plan->set.G]);
      }
      free(plan);
      free(images);
    } else if (kind == "mask") {
      int H, W, thresh, modes;
      long long cap;
      if (!(ss >> H >> W >> thresh >> modes >> cap)) continue;
      const int HW64 = (H + 63) / 64;
      const long long Q = (long long)W * HW64;
      unsigned long long* P = (unsigned long long*)malloc(sizeof(unsigned long long) * (size_t)Q);
      for (long long q = 0; q < Q; ++q) {
        std::string w;
        ss >> w;
        P[q] = strtoull(w.c_str(), nullptr, 16);
      }
      int code = 0, changed = 0;
      for (int pass = 0; pass < 2 && code == 0; ++pass) {
        if (!((modes >> pass) & 1)) continue;
        const int r = clean_pass(P, H, W, pass == 0, thresh, cap);
        if (r < 0) code = 3; else changed |= r << pass;
      }
      if (code) {
        printf("3 0 0 0 0 0 0\n");
      } else {
        long long area = 0;
        int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = 0, y1 = 0;
        for (long long q = 0; q < Q; ++q) {
          if (!P[q]) continue;
          const int x = (int)(q / HW64), y = 64 * (int)(q % HW64);
          const int ya = y + __builtin_ctzll(P[q]), yb = y + 63 - __builtin_clzll(P[q]);
          area += __builtin_popcountll(P[q]);
          x0 = x0 < x ? x0 : x; x1 = x1 > x ? x1 : x;
          y0 = y0 < ya ? y0 : ya; y1 = y1 > yb ? y1 : yb;
        }
        if (!area) x0 = y0 = x1 = y1 = 0;
        printf("0 %d %lld %d %d %d %d", changed, area, x0, y0, x1, y1);
        for (long long q = 0; q < Q; ++q) printf(" %llx", P[q]);
        printf("\n");
      }
      free(P);
    }
  }
  return 0;
}
