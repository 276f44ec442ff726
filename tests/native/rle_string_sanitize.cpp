// Sanitizer harness for hgl_rle_from_string (csrc/gtmask.cpp), built by tests/test_sanitize_rle_string.py with
// g++ -fsanitize=address,undefined.  Reads a case file written by the test, one case per line:
//   <cap> <string>        cap = capacity of the counts buffer in words, -1 = the size query with a null pointer;
//                         <empty> stands for the empty string
// and prints one line per case: the return code, the number of counts and an FNV-1a hash of the counts written.
#include <cstdint>
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <string>

extern "C" int hgl_rle_from_string(const char* s, uint32_t* counts, long long cap, long long* m);
void hgl_set_error(const char*, ...) {}

static unsigned long long fnv(const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  unsigned long long h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  long long cap;
  char buf[4096];
  while (fscanf(f, "%lld %4095s", &cap, buf) == 2) {
    std::string s(buf);
    if (s == "<empty>") s.clear();
    // exact-size heap copies: a read past the terminator or a write past cap is a heap-buffer-overflow for ASan
    char* heap = new char[s.size() + 1];
    memcpy(heap, s.c_str(), s.size() + 1);
    uint32_t* counts = cap >= 0 ? new uint32_t[cap > 0 ? cap : 1] : nullptr;
    long long m = -1;
    const int rc = hgl_rle_from_string(heap, counts, cap < 0 ? 0 : cap, &m);
    const long long written = rc ? 0 : (cap < 0 ? 0 : (m < cap ? m : cap));
    printf("%d %lld %llu\n", rc, rc ? -1ll : m, fnv(counts, (size_t)written * sizeof(uint32_t)));
    delete[] counts;
    delete[] heap;
  }
  fclose(f);
  return 0;
}
