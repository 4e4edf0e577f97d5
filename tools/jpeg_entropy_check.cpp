// Stand-alone robustness check of egohmr_amd/csrc/jpeg_entropy.h, meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I egohmr_amd/csrc tools/jpeg_entropy_check.cpp -o check
//   ./check tests/golden/jpeg/*.jpg
// It decodes every file given, every proper prefix of every file, and 20 000 single-byte mutations drawn from a fixed LCG seed.  Inputs and
// the coefficient buffer live in heap blocks of exactly their size, so a read or write one byte past either is a sanitizer report.  A file
// whose name contains "progressive" must be refused, every other must decode, every proper prefix must be refused; a mutation may give either.
// Exit status 0: all of that held (and the sanitizers, which abort on their own, saw nothing).
#include "jpeg_entropy.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

static int decode(const std::vector<uint8_t>& src, size_t n, int64_t capacity, ehm_jpeg::Frame* f, char* msg, size_t msgcap) {
  uint8_t* data = (uint8_t*)malloc(n ? n : 1);                       // exactly n bytes: an over-read is a heap-buffer-overflow
  int16_t* coef = (int16_t*)malloc(capacity ? (size_t)capacity * sizeof(int16_t) : 1);
  if (!data || !coef) abort();
  memcpy(data, src.data(), n);
  const int rc = ehm_jpeg::entropy_decode(data, (int64_t)n, f, coef, capacity, msg, msgcap);
  free(coef);
  free(data);
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]);
    return 2;
  }
  std::vector<std::vector<uint8_t>> files;
  std::vector<int64_t> counts;
  char msg[256];
  long decoded = 0, refused = 0;
  for (int a = 1; a < argc; ++a) {
    FILE* fp = fopen(argv[a], "rb");
    if (!fp) {
      fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> d;
    uint8_t chunk[4096];
    size_t got;
    while ((got = fread(chunk, 1, sizeof chunk, fp)) > 0) d.insert(d.end(), chunk, chunk + got);
    fclose(fp);
    const bool must_refuse = std::string(argv[a]).find("progressive") != std::string::npos;
    ehm_jpeg::Frame f;
    memset(&f, 0, sizeof f);
    int rc = ehm_jpeg::read_header(d.data(), (int64_t)d.size(), &f, msg, sizeof msg);
    if ((rc != 0) != must_refuse || (rc != 0 && !msg[0])) {
      fprintf(stderr, "%s: read_header gave %d (%s)\n", argv[a], rc, msg);
      return 1;
    }
    const int64_t count = must_refuse ? 64 : f.coef_count;
    rc = decode(d, d.size(), count, &f, msg, sizeof msg);
    if ((rc != 0) != must_refuse || (rc != 0 && !msg[0])) {
      fprintf(stderr, "%s: entropy_decode gave %d (%s)\n", argv[a], rc, msg);
      return 1;
    }
    if (!must_refuse && decode(d, d.size(), count - 1, &f, msg, sizeof msg) == 0) {
      fprintf(stderr, "%s: a capacity one short was accepted\n", argv[a]);
      return 1;
    }
    for (size_t n = 0; n < d.size(); ++n) {                           // every proper prefix
      rc = decode(d, n, count, &f, msg, sizeof msg);
      if (rc == 0 || !msg[0]) {
        fprintf(stderr, "%s: the prefix of %zu bytes gave %d (%s)\n", argv[a], n, rc, msg);
        return 1;
      }
    }
    files.push_back(d);
    counts.push_back(count);
  }
  uint64_t lcg = 0x9E3779B97F4A7C15ull;
  auto next = [&lcg]() {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(lcg >> 33);
  };
  for (int i = 0; i < 20000; ++i) {
    const size_t k = next() % files.size();
    std::vector<uint8_t> d = files[k];
    d[next() % d.size()] = (uint8_t)next();
    ehm_jpeg::Frame f;
    const int rc = decode(d, d.size(), counts[k], &f, msg, sizeof msg);
    if (rc != 0 && (rc != -22 || !msg[0])) {
      fprintf(stderr, "mutation %d: status %d with message '%s'\n", i, rc, msg);
      return 1;
    }
    ++(rc ? refused : decoded);
  }
  printf("%zu files, every prefix refused, 20000 mutations: %ld decoded, %ld refused\n", files.size(), decoded, refused);
  return 0;
}
