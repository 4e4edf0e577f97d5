// Stand-alone check of the encoder's host entries (egohmr_amd/csrc/jpeg_enc.h), meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I egohmr_amd/csrc tools/jpeg_header_check.cpp -o check
//   ./check
// For every capacity from 0 to the header's size (and a little beyond) the output lives in a heap block of exactly that size, so a write one
// byte past the capacity is a sanitizer report.  Over all sizes 1..40 x 1..40 and the three samplings: a capacity below the header's size
// must be refused with *n = 0 and the block untouched; from the header's size on the header must be written, and the decoder's own parser
// (jpeg_entropy.h read_header) must read the same geometry and tables back.  Every quality -10..110 goes through quality_tables, unsupported
// samplings, a zero table entry and null pointers must be refused.  Exit status 0: all of that held.
#include "jpeg_enc.h"
#include "jpeg_entropy.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int fail(const char* what, int a, int b, int c, int d) {
  fprintf(stderr, "%s (%d %d %d %d)\n", what, a, b, c, d);
  return 1;
}

int main() {
  using namespace ehm_jpeg_enc;
  char msg[128];
  uint16_t quant[2][64];
  for (int q = -10; q <= 110; ++q) {
    memset(quant, 0, sizeof quant);
    const int rc = quality_tables(q, quant, msg, sizeof msg);
    if ((rc == 0) != (q >= 1 && q <= 100)) return fail("quality_tables status", q, rc, 0, 0);
    if (rc == 0)
      for (int i = 0; i < 128; ++i)
        if (quant[i / 64][i % 64] < 1 || quant[i / 64][i % 64] > 255) return fail("quality_tables entry", q, i, quant[i / 64][i % 64], 0);
    if (rc != 0 && (rc != kError || !msg[0])) return fail("quality_tables refusal", q, rc, 0, 0);
  }
  if (quality_tables(50, nullptr, msg, sizeof msg) != kError) return fail("quality_tables null", 0, 0, 0, 0);
  const int samplings[3][2] = {{1, 1}, {2, 1}, {2, 2}};
  long geometries = 0, calls = 0;
  for (int64_t capacity = 0; capacity <= kHeaderBytes + 8; ++capacity) {
    uint8_t* out = (uint8_t*)malloc(capacity ? (size_t)capacity : 1);           // exactly `capacity` bytes
    if (!out) abort();
    memset(out, 0xA5, (size_t)capacity);
    for (int s = 0; s < 3; ++s)
      for (int H = 1; H <= 40; ++H)
        for (int W = 1; W <= 40; ++W) {
          if (quality_tables(1 + (H * 41 + W) % 100, quant, msg, sizeof msg)) return fail("quality_tables", H, W, 0, 0);
          if (capacity >= kHeaderBytes) memset(out, 0xA5, (size_t)capacity);
          int64_t n = -1;
          const int rc = write_header(H, W, samplings[s][0], samplings[s][1], quant, out, capacity, &n, msg, sizeof msg);
          ++calls;
          if (capacity < kHeaderBytes) {                              // (the block is inspected once, after every geometry had its try)
            if (rc != kError || n != 0 || !msg[0]) return fail("a short capacity was accepted", H, W, s, (int)capacity);
            continue;
          }
          if (rc != kOk || n != kHeaderBytes) return fail("write_header failed", H, W, s, rc);
          for (int64_t i = n; i < capacity; ++i)
            if (out[i] != 0xA5) return fail("written past the header", H, W, s, (int)capacity);
          if (capacity != kHeaderBytes) continue;
          ++geometries;
          ehm_jpeg::Frame f;
          memset(&f, 0, sizeof f);
          char pmsg[256];
          if (ehm_jpeg::read_header(out, n, &f, pmsg, sizeof pmsg)) return fail(pmsg, H, W, s, 0);
          if (f.H != H || f.W != W || f.components != 3 || f.hmax != samplings[s][0] || f.vmax != samplings[s][1] || f.restart_interval != 0 ||
              f.quant_id[0] != 0 || f.quant_id[1] != 1 || f.quant_id[2] != 1 || memcmp(f.quant, quant, sizeof quant) != 0)
            return fail("the parser read other fields back", H, W, s, 0);
        }
    if (capacity < kHeaderBytes)
      for (int64_t i = 0; i < capacity; ++i)
        if (out[i] != 0xA5) return fail("a refused call wrote", (int)i, 0, 0, (int)capacity);
    free(out);
  }
  uint8_t buf[kHeaderBytes];
  int64_t n = 0;
  quality_tables(75, quant, msg, sizeof msg);
  const int bad[5][2] = {{1, 2}, {2, 4}, {4, 1}, {0, 0}, {3, 3}};
  for (const auto& b : bad)
    if (write_header(8, 8, b[0], b[1], quant, buf, sizeof buf, &n, msg, sizeof msg) != kError || n != 0) return fail("sampling accepted", b[0], b[1], 0, 0);
  if (write_header(0, 8, 2, 2, quant, buf, sizeof buf, &n, msg, sizeof msg) != kError) return fail("H = 0 accepted", 0, 0, 0, 0);
  if (write_header(8, 65536, 2, 2, quant, buf, sizeof buf, &n, msg, sizeof msg) != kError) return fail("W = 65536 accepted", 0, 0, 0, 0);
  if (write_header(8, 8, 2, 2, nullptr, buf, sizeof buf, &n, msg, sizeof msg) != kError) return fail("null tables accepted", 0, 0, 0, 0);
  if (write_header(8, 8, 2, 2, quant, nullptr, sizeof buf, &n, msg, sizeof msg) != kError) return fail("null output accepted", 0, 0, 0, 0);
  if (write_header(8, 8, 2, 2, quant, buf, sizeof buf, nullptr, msg, sizeof msg) != kError) return fail("null count accepted", 0, 0, 0, 0);
  if (write_header(8, 8, 2, 2, quant, buf, sizeof buf, &n, nullptr, 0) != kOk) return fail("a null message buffer broke a good call", 0, 0, 0, 0);
  quant[1][63] = 0;
  if (write_header(8, 8, 2, 2, quant, buf, sizeof buf, &n, msg, sizeof msg) != kError) return fail("a zero table entry accepted", 0, 0, 0, 0);
  printf("%ld geometries, %ld calls over capacities 0..%d: nothing written past a capacity\n", geometries, calls, kHeaderBytes + 8);
  return 0;
}
