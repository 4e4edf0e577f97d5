// The host side of the baseline-JPEG encoder: libjpeg's quality scaling of the Annex K.1 / K.2 quantisation tables, the fixed Annex K.3 - K.6
// Huffman tables, and the marker segments around the entropy-coded stream (SOI ... SOS, in the order PIL writes them).  Header-only, plain
// C++17, no HIP include, no allocation: the caller brings the output buffer and the message buffer.  Nothing is written at or past
// out + capacity; a refusal returns a negative status with a message.  csrc/jpeg_enc.hip derives the device's code tables from the same arrays.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace ehm_jpeg_enc {

constexpr int kOk = 0;
constexpr int kError = -22;
constexpr int kHeaderBytes = 623;   // SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 33 + 183 + 33 + 183, SOS 14

constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.1 (luminance) and K.2 (chrominance), natural order
constexpr uint8_t kBaseQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3 - K.6: the number of codes of each length 1..16, then the symbols in code order
struct HuffSpec {
  uint8_t id;   // the DHT byte: (class << 4) | table
  uint8_t counts[16];
  int nsym;
  uint8_t symbols[162];
};
constexpr HuffSpec kHuffman[4] = {
    {0x00, {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {0x10, {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, 162,
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
      0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
      0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
      0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
      0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
      0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
      0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa}},
    {0x01, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {0x11, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}, 162,
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
      0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
      0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
      0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
      0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
      0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa}}};

// The canonical code of one table by symbol: (length << 16) | code, 0 for a symbol the table does not hold.
struct CodeTable {
  uint32_t e[256];
};
constexpr CodeTable make_codes(const HuffSpec& s) {
  CodeTable t = {};
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < s.counts[len - 1]; ++i) t.e[s.symbols[k++]] = ((uint32_t)len << 16) | code++;
    code <<= 1;
  }
  return t;
}

inline int fail(char* msg, size_t msgcap, const char* text) {
  if (msg && msgcap) snprintf(msg, msgcap, "jpeg encoder: %s", text);
  return kError;
}

inline bool sampling_ok(int hmax, int vmax) { return (hmax == 1 && vmax == 1) || (hmax == 2 && vmax == 1) || (hmax == 2 && vmax == 2); }

// libjpeg's jpeg_set_quality with force_baseline: quant[2][64], natural order
inline int quality_tables(int quality, uint16_t (*quant)[64], char* msg, size_t msgcap) {
  if (!quant) return fail(msg, msgcap, "null argument");
  if (quality < 1 || quality > 100) return fail(msg, msgcap, "quality outside 1..100");
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      const int v = (kBaseQuant[t][i] * s + 50) / 100;
      quant[t][i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
  return kOk;
}

// SOI, APP0 JFIF 1.01, DQT 0, DQT 1, SOF0, DHT DC0 AC0 DC1 AC1, SOS: kHeaderBytes bytes into out[0 .. capacity); *n = the bytes written
// (0 on a refusal: a capacity below kHeaderBytes writes nothing).
inline int write_header(int H, int W, int hmax, int vmax, const uint16_t (*quant)[64], uint8_t* out, int64_t capacity, int64_t* n, char* msg,
                        size_t msgcap) {
  if (n) *n = 0;
  if (!quant || !out || !n) return fail(msg, msgcap, "null argument");
  if (H < 1 || H > 65535 || W < 1 || W > 65535) return fail(msg, msgcap, "height or width outside 1..65535");
  if (!sampling_ok(hmax, vmax)) return fail(msg, msgcap, "unsupported sampling (luma 1x1, 2x1 or 2x2 with chroma 1x1 only)");
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i)
      if (quant[t][i] < 1 || quant[t][i] > 255) return fail(msg, msgcap, "a quantisation table entry outside 1..255 (baseline tables are 8-bit)");
  if (capacity < kHeaderBytes) return fail(msg, msgcap, "capacity too small for the header");
  uint8_t* p = out;
  auto put = [&p](int v) { *p++ = (uint8_t)v; };
  auto open = [&put](int marker, int body) { put(0xFF), put(marker), put((body + 2) >> 8), put((body + 2) & 255); };
  put(0xFF), put(0xD8);
  open(0xE0, 14);
  const int app0[14] = {0x4A, 0x46, 0x49, 0x46, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};   // "JFIF", version 1.01, units 0, density 1 x 1, no thumbnail
  for (const int v : app0) put(v);
  for (int t = 0; t < 2; ++t) {
    open(0xDB, 65);
    put(t);
    for (int i = 0; i < 64; ++i) put(quant[t][kZigzag[i]]);
  }
  open(0xC0, 15);
  const int sof[15] = {8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, (hmax << 4) | vmax, 0, 2, 0x11, 1, 3, 0x11, 1};
  for (const int v : sof) put(v);
  for (const HuffSpec& s : kHuffman) {
    open(0xC4, 17 + s.nsym);
    put(s.id);
    for (int i = 0; i < 16; ++i) put(s.counts[i]);
    for (int i = 0; i < s.nsym; ++i) put(s.symbols[i]);
  }
  open(0xDA, 10);
  const int sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  for (const int v : sos) put(v);
  *n = p - out;
  return kOk;
}

}  // namespace ehm_jpeg_enc
