// The parser of the device JPEG decoder (collaborative-distillation_amd/csrc/jdec_parse.h) as a stand-alone program for the host
// sanitizers: tests/test_jdec_cpu.py compiles it with -fsanitize=address,undefined and runs it as a child process.
//   jdec_parse_main FILE...   for every file: the parser on every prefix and on every single-byte corruption (three values per byte),
//                             each from a heap copy of exactly that length, so that a read past the end is a heap overflow
// Prints "FILE accepted refused" per file; exit 0 unless the intact file is refused.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../collaborative-distillation_amd/csrc/jdec_parse.h"

static int run(const std::vector<uint8_t>& v, size_t n, wct_jdec_info* info) {
  uint8_t* p = (uint8_t*)malloc(n ? n : 1);
  for (size_t i = 0; i < n; ++i) p[i] = v[i];
  const int rc = wct_jdec::parse(p, n, info);
  free(p);
  return rc;
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) return 2;
    std::vector<uint8_t> v;
    for (int c; (c = fgetc(f)) != EOF;) v.push_back((uint8_t)c);
    fclose(f);
    wct_jdec_info info;
    long ok = 0, no = 0;
    if (run(v, v.size(), &info) != WCT_OK) return 3;
    for (size_t n = 0; n < v.size(); ++n) (run(v, n, &info) == WCT_OK ? ok : no)++;
    for (size_t i = 0; i < v.size(); ++i)
      for (int x : {0xFF, 0x01, 0x80}) {
        std::vector<uint8_t> w = v;
        w[i] ^= (uint8_t)x;
        const int rc = run(w, w.size(), &info);
        if (rc == WCT_OK && !wct_jdec::info_ok(info)) return 4;
        (rc == WCT_OK ? ok : no)++;
      }
    printf("%s %ld %ld\n", argv[a], ok, no);
  }
  return 0;
}
