// Sanitizer harness for csrc/rle_string.h, the arithmetic of the device's COCO string codec, built by
// tests/test_sanitize_rle_string_walk.py with g++ -fsanitize=address,undefined -fno-sanitize-recover=all as a stand-alone
// program: the header alone, no HIP, nothing loaded into Python.  Every function is called the way a thread of the kernels
// calls it -- one count, one byte, one group at a time, on heap copies of exactly the right size -- and the counts' un-delta
// runs in stretches that begin at either parity.
//
//   usage: rle_string_walk_sanitize CASES      one case per line, one answer line per case on stdout
//     X x                 -> k and the k characters of the group of x, in hex
//     G hex               -> the value of the group `hex` (1 .. 7 bytes)
//     W n c0 .. c(n-1)    -> the string of the n counts, in hex ("-" when empty)
//     R stretch hex       -> code n c0 .. : what the reader makes of the string ("-": empty), un-delta in stretches of `stretch`
//     U i0 n carry0 carry1 v0 .. v(n-1) -> the stretch after rstr_undelta_stretch, then the two carries
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../hybridgl_amd/csrc/rle_string.h"

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> b;
  if (h == "-") return b;
  for (size_t i = 0; i + 1 < h.size(); i += 2) b.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return b;
}

static void put_hex(const uint8_t* b, size_t n) {
  if (n == 0) printf("-");
  for (size_t i = 0; i < n; ++i) printf("%02x", b[i]);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string kind;
    ls >> kind;
    if (kind == "X") {
      long long x;
      ls >> x;
      const int k = rstr_length(x);
      uint8_t* g = new uint8_t[k];
      for (int j = k - 1; j >= 0; --j) g[j] = rstr_char(x, j, k);      // any order: a character depends on x, j and k alone
      printf("%d ", k);
      put_hex(g, k);
      printf("\n");
      delete[] g;
    } else if (kind == "G") {
      std::string h;
      ls >> h;
      const std::vector<uint8_t> b = unhex(h);
      uint8_t* g = new uint8_t[b.size()];
      if (!b.empty()) memcpy(g, b.data(), b.size());
      printf("%u\n", rstr_group_value(g, (int)b.size()));
      delete[] g;
    } else if (kind == "W") {
      long long n;
      ls >> n;
      uint32_t* c = new uint32_t[n];
      for (long long i = 0; i < n; ++i) { unsigned long long v; ls >> v; c[i] = (uint32_t)v; }
      // the writer's two sweeps: the lengths, then every group at its own place, last count first
      std::vector<long long> at(n + 1, 0);
      for (long long i = 0; i < n; ++i) at[i + 1] = at[i] + rstr_length(rstr_delta(c, i));
      uint8_t* out = new uint8_t[at[n]];
      for (long long i = n - 1; i >= 0; --i) {
        const long long x = rstr_delta(c, i);
        const int k = rstr_length(x);
        for (int j = 0; j < k; ++j) out[at[i] + j] = rstr_char(x, j, k);
      }
      put_hex(out, (size_t)at[n]);
      printf("\n");
      delete[] out;
      delete[] c;
    } else if (kind == "R") {
      long long stretch;
      std::string h;
      ls >> stretch >> h;
      const std::vector<uint8_t> b = unhex(h);
      const long long L = (long long)b.size();
      uint8_t* s = new uint8_t[L];
      if (L > 0) memcpy(s, b.data(), L);
      // sweep 1, last byte first
      long long ends = 0;
      bool is_long = false;
      for (long long p = L - 1; p >= 0; --p) {
        ends += rstr_more(s[p]) ? 0 : 1;
        is_long = is_long || rstr_long_at(s, p);
      }
      if (is_long) printf("3 0\n");
      else if (L > 0 && rstr_more(s[L - 1])) printf("2 0\n");
      else {
        uint32_t* slot = new uint32_t[ends];
        // sweep 2: the rank of an ending byte is the number of ending bytes before it
        std::vector<long long> rank(L + 1, 0);
        for (long long p = 0; p < L; ++p) rank[p + 1] = rank[p] + (rstr_more(s[p]) ? 0 : 1);
        for (long long p = L - 1; p >= 0; --p)
          if (!rstr_more(s[p])) {
            const int k = rstr_group_length(s, p);
            slot[rank[p]] = rstr_group_value(s + (p - k + 1), k);
          }
        // sweep 3 in stretches
        uint32_t carry[2] = {0u, 0u};
        for (long long i0 = 0; i0 < ends; i0 += stretch)
          rstr_undelta_stretch(slot + i0, i0, ends - i0 < stretch ? ends - i0 : stretch, carry);
        printf("0 %lld", ends);
        for (long long i = 0; i < ends; ++i) printf(" %u", slot[i]);
        printf("\n");
        delete[] slot;
      }
      delete[] s;
    } else if (kind == "U") {
      long long i0, n;
      unsigned long long c0, c1;
      ls >> i0 >> n >> c0 >> c1;
      uint32_t* v = new uint32_t[n];
      for (long long i = 0; i < n; ++i) { unsigned long long x; ls >> x; v[i] = (uint32_t)x; }
      uint32_t carry[2] = {(uint32_t)c0, (uint32_t)c1};
      rstr_undelta_stretch(v, i0, n, carry);
      for (long long i = 0; i < n; ++i) printf("%u ", v[i]);
      printf("%u %u\n", carry[0], carry[1]);
      delete[] v;
    } else if (!kind.empty()) {
      return 3;
    }
  }
  return 0;
}
