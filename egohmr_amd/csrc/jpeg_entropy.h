// The host stage of the baseline-JPEG decoder: marker parser + Huffman (entropy) decoder over a byte span.  Header-only, plain C++17, no HIP
// include, no allocation: the caller brings the coefficient buffer and the message buffer.  Every read is bounds-checked and every table index
// validated; anything unsupported or malformed returns a negative status with a message - it never crashes and never writes past `capacity`.
//
// Accepted: SOI, DQT (8-bit tables), DHT, SOF0 / SOF1 with 8-bit precision, DRI, SOS, RSTn, EOI; APPn and COM are skipped (EXIF orientation
// included: it is ignored, as cv2's IMREAD_IGNORE_ORIENTATION asks).  One interleaved scan of 1 or 3 components; luma sampling (1,1), (2,1)
// or (2,2) with chroma (1,1); a one-component frame is decoded as (1,1) whatever factors it declares, as libjpeg does.
// Refused: progressive, arithmetic, lossless and hierarchical processes, 12-bit samples, 16-bit quantisation tables, 4 components, any other
// sampling, several scans, data that ends early, a marker inside the entropy data, restart markers out of order, a missing EOI.
//
// Output: QUANTISED int16 coefficients (a dequantised value does not fit in int16; the tables travel in Frame::quant), component planes one
// after the other, each plane blocks in row-major order over the MCU-padded grid [blocks_y][blocks_x], each block 64 values in natural order.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace ehm_jpeg {

constexpr int kOk = 0;
constexpr int kError = -22;
constexpr int kMaxComponents = 3;

struct Frame {
  int H, W, components, hmax, vmax, mcus_x, mcus_y, restart_interval;
  int h[kMaxComponents], v[kMaxComponents], blocks_x[kMaxComponents], blocks_y[kMaxComponents], quant_id[kMaxComponents];
  uint16_t quant[4][64];   // natural order; a table no DQT defined is zero
  int64_t coef_count;      // int16 values of one frame's coefficients
};

namespace detail {

constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr int kLookBits = 9;

struct Huffman {
  bool defined;
  int nsym;
  uint8_t sym[256];
  int32_t mincode[17], maxcode[17], valptr[17];   // per code length 1..16; maxcode -1: no code of that length
  uint16_t look[1 << kLookBits];                  // (length << 8) | symbol for codes of up to kLookBits bits, 0: longer or none
};

struct Parser {
  const uint8_t* d;
  int64_t n, pos;
  char* msg;
  size_t msgcap;
  Frame f;
  bool have_frame, qdef[4];
  int comp_id[kMaxComponents], dc_tab[kMaxComponents], ac_tab[kMaxComponents];
  Huffman huff[2][4];   // [class: 0 DC, 1 AC][id]
};

inline int fail(Parser& p, const char* text) {
  if (p.msg && p.msgcap) snprintf(p.msg, p.msgcap, "jpeg: %s (at byte %lld of %lld)", text, (long long)p.pos, (long long)p.n);
  return kError;
}

inline int build_huffman(Parser& p, Huffman& t, const uint8_t* counts, const uint8_t* symbols, int nsym) {
  t.defined = false;
  t.nsym = nsym;
  memcpy(t.sym, symbols, (size_t)nsym);
  memset(t.look, 0, sizeof(t.look));
  int32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int c = counts[l - 1];
    t.valptr[l] = k;
    t.mincode[l] = code;
    if (code + c > (1 << l)) return fail(p, "DHT: more codes of a length than the length allows");
    if (c && l <= kLookBits)
      for (int i = 0; i < c; ++i) {
        const int first = (code + i) << (kLookBits - l);
        for (int j = 0; j < (1 << (kLookBits - l)); ++j) t.look[first + j] = (uint16_t)((l << 8) | symbols[k + i]);
      }
    code += c;
    k += c;
    t.maxcode[l] = c ? code - 1 : -1;
    code <<= 1;
  }
  t.defined = true;
  return kOk;
}

inline int read_dqt(Parser& p, int64_t at, int64_t end) {
  while (at < end) {
    const int pq = p.d[at] >> 4, tq = p.d[at] & 15;
    if (pq != 0) return fail(p, "16-bit quantisation tables are not supported");
    if (tq > 3) return fail(p, "DQT: table id above 3");
    if (at + 65 > end) return fail(p, "DQT: segment too short");
    for (int i = 0; i < 64; ++i) p.f.quant[tq][kZigzag[i]] = p.d[at + 1 + i];
    p.qdef[tq] = true;
    at += 65;
  }
  return kOk;
}

inline int read_dht(Parser& p, int64_t at, int64_t end) {
  while (at < end) {
    const int tc = p.d[at] >> 4, th = p.d[at] & 15;
    if (tc > 1 || th > 3) return fail(p, "DHT: table class or id out of range");
    if (at + 17 > end) return fail(p, "DHT: segment too short");
    int total = 0;
    for (int i = 0; i < 16; ++i) total += p.d[at + 1 + i];
    if (total > 256 || at + 17 + total > end) return fail(p, "DHT: symbol count does not fit the segment");
    const int rc = build_huffman(p, p.huff[tc][th], p.d + at + 1, p.d + at + 17, total);
    if (rc) return rc;
    at += 17 + total;
  }
  return kOk;
}

inline int read_sof(Parser& p, int64_t at, int64_t end) {
  if (p.have_frame) return fail(p, "a second frame header");
  if (end - at < 6) return fail(p, "SOF: segment too short");
  if (p.d[at] != 8) return fail(p, "only 8-bit samples are supported (12-bit JPEG refused)");
  Frame& f = p.f;
  f.H = (p.d[at + 1] << 8) | p.d[at + 2];
  f.W = (p.d[at + 3] << 8) | p.d[at + 4];
  const int nc = p.d[at + 5];
  if (nc != 1 && nc != 3) return fail(p, "only 1 or 3 components are supported (4-component JPEG refused)");
  if (f.H == 0 || f.W == 0) return fail(p, "SOF: zero height or width");
  if (end - at != 6 + 3 * nc) return fail(p, "SOF: segment length does not match the component count");
  f.components = nc;
  for (int c = 0; c < nc; ++c) {
    const uint8_t* q = p.d + at + 6 + 3 * c;
    p.comp_id[c] = q[0];
    f.h[c] = q[1] >> 4;
    f.v[c] = q[1] & 15;
    f.quant_id[c] = q[2];
    if (f.h[c] < 1 || f.h[c] > 4 || f.v[c] < 1 || f.v[c] > 4) return fail(p, "SOF: sampling factor out of range");
    if (f.quant_id[c] > 3) return fail(p, "SOF: quantisation table id above 3");
  }
  if (nc == 1) {
    f.h[0] = f.v[0] = 1;
  } else {
    const bool luma = (f.h[0] == 1 && f.v[0] == 1) || (f.h[0] == 2 && f.v[0] == 1) || (f.h[0] == 2 && f.v[0] == 2);
    if (!luma || f.h[1] != 1 || f.v[1] != 1 || f.h[2] != 1 || f.v[2] != 1)
      return fail(p, "unsupported sampling (luma 1x1, 2x1 or 2x2 with chroma 1x1 only)");
  }
  f.hmax = f.h[0];
  f.vmax = f.v[0];
  f.mcus_x = (f.W + 8 * f.hmax - 1) / (8 * f.hmax);
  f.mcus_y = (f.H + 8 * f.vmax - 1) / (8 * f.vmax);
  f.coef_count = 0;
  for (int c = 0; c < nc; ++c) {
    f.blocks_x[c] = f.mcus_x * f.h[c];
    f.blocks_y[c] = f.mcus_y * f.v[c];
    f.coef_count += (int64_t)64 * f.blocks_x[c] * f.blocks_y[c];
  }
  p.have_frame = true;
  return kOk;
}

inline int read_sos(Parser& p, int64_t at, int64_t end) {
  if (!p.have_frame) return fail(p, "SOS before the frame header");
  const int nc = p.f.components;
  if (end - at < 1 || p.d[at] != nc || end - at != 4 + 2 * nc) return fail(p, "only one interleaved scan of every component is supported");
  for (int c = 0; c < nc; ++c) {
    if (p.d[at + 1 + 2 * c] != p.comp_id[c]) return fail(p, "SOS: component ids do not follow the frame's");
    const int td = p.d[at + 2 + 2 * c] >> 4, ta = p.d[at + 2 + 2 * c] & 15;
    if (td > 3 || ta > 3) return fail(p, "SOS: Huffman table id above 3");
    if (!p.huff[0][td].defined || !p.huff[1][ta].defined) return fail(p, "SOS: a Huffman table it names was never defined");
    p.dc_tab[c] = td;
    p.ac_tab[c] = ta;
    if (!p.qdef[p.f.quant_id[c]]) return fail(p, "a quantisation table the frame names was never defined");
  }
  const uint8_t* q = p.d + at + 1 + 2 * nc;
  if (q[0] != 0 || q[1] != 63 || q[2] != 0) return fail(p, "SOS: spectral selection / approximation of a progressive scan");
  return kOk;
}

// SOI ... SOS: on success p.pos is the first byte of the entropy-coded data
inline int parse_headers(Parser& p) {
  if (p.n < 2 || p.d[0] != 0xFF || p.d[1] != 0xD8) return fail(p, "no SOI marker: not a JPEG file");
  p.pos = 2;
  for (;;) {
    if (p.pos >= p.n || p.d[p.pos] != 0xFF) return fail(p, p.pos >= p.n ? "truncated: the data ends before SOS" : "marker expected");
    while (p.pos < p.n && p.d[p.pos] == 0xFF) ++p.pos;
    if (p.pos >= p.n) return fail(p, "truncated: the data ends inside a marker");
    const int m = p.d[p.pos++];
    if (m == 0xD9 || m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD8)) return fail(p, "unexpected marker before SOS");
    if (p.pos + 2 > p.n) return fail(p, "truncated: the data ends inside a segment length");
    const int len = (p.d[p.pos] << 8) | p.d[p.pos + 1];
    if (len < 2 || p.pos + len > p.n) return fail(p, "truncated: a segment is longer than the data");
    const int64_t at = p.pos + 2, end = p.pos + len;
    int rc = kOk;
    if (m == 0xDB) {
      rc = read_dqt(p, at, end);
    } else if (m == 0xC4) {
      rc = read_dht(p, at, end);
    } else if (m == 0xC0 || m == 0xC1) {
      rc = read_sof(p, at, end);
    } else if (m == 0xC2) {
      rc = fail(p, "progressive JPEG is not supported");
    } else if (m == 0xC9 || m == 0xCA || m == 0xCB || m == 0xCC || m == 0xCD || m == 0xCE || m == 0xCF) {
      rc = fail(p, "arithmetic-coded JPEG is not supported");
    } else if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7 || m == 0xC8) {
      rc = fail(p, "lossless / hierarchical JPEG is not supported");
    } else if (m == 0xDD) {
      if (len != 4) rc = fail(p, "DRI: bad segment length");
      else p.f.restart_interval = (p.d[at] << 8) | p.d[at + 1];
    } else if (m == 0xDA) {
      rc = read_sos(p, at, end);
      if (rc) return rc;
      p.pos = end;
      return kOk;
    } else if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
      // APPn, COM: skipped
    } else {
      rc = fail(p, "unsupported marker");
    }
    if (rc) return rc;
    p.pos = end;
  }
}

// The entropy-coded bytes as a bit stream.  buf holds cnt valid bits left-aligned, zeros below them.  FF 00 is the data byte FF; at any other
// FF xx (a marker) or at the end of the data the reader stops taking bytes - pos stays on that FF - and asking for more bits than it has fails.
struct Bits {
  const uint8_t* d;
  int64_t n, pos;
  uint64_t buf;
  int cnt;
};

inline void fill(Bits& b) {
  while (b.cnt <= 56) {
    if (b.pos >= b.n) return;
    const uint8_t x = b.d[b.pos];
    if (x == 0xFF) {
      if (b.pos + 1 >= b.n || b.d[b.pos + 1] != 0) return;
      b.pos += 2;
    } else {
      b.pos += 1;
    }
    b.buf |= (uint64_t)x << (56 - b.cnt);
    b.cnt += 8;
  }
}

// nbits in 1..16; -1: the data ran out
inline int take(Bits& b, int nbits) {
  if (b.cnt < nbits) {
    fill(b);
    if (b.cnt < nbits) return -1;
  }
  const int v = (int)(b.buf >> (64 - nbits));
  b.buf <<= nbits;
  b.cnt -= nbits;
  return v;
}

// -> symbol, -1: the data ran out, -2: a code with no entry
inline int decode_symbol(Bits& b, const Huffman& t) {
  if (b.cnt < 16) fill(b);
  const uint32_t top = (uint32_t)(b.buf >> 48);   // the next 16 bits, zeros past the valid ones
  const uint16_t e = t.look[top >> (16 - kLookBits)];
  int len, sym;
  if (e) {
    len = e >> 8;
    sym = e & 255;
  } else {
    len = kLookBits + 1;
    for (; len <= 16; ++len) {
      const int32_t code = (int32_t)(top >> (16 - len));
      if (t.maxcode[len] >= 0 && code <= t.maxcode[len] && code >= t.mincode[len]) break;
    }
    if (len > 16) return b.cnt < 16 ? -1 : -2;
    const int idx = t.valptr[len] + (int32_t)(top >> (16 - len)) - t.mincode[len];
    if (idx < 0 || idx >= t.nsym) return -2;
    sym = t.sym[idx];
  }
  if (len > b.cnt) return -1;
  b.buf <<= len;
  b.cnt -= len;
  return sym;
}

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// one 8x8 block: DC difference on *pred, AC run/size pairs, un-zigzag into blk[64] (cleared here)
inline int decode_block(Parser& p, Bits& b, const Huffman& dc, const Huffman& ac, int* pred, int16_t* blk) {
  memset(blk, 0, 64 * sizeof(int16_t));
  int s = decode_symbol(b, dc);
  if (s < 0) return fail(p, s == -1 ? "truncated: the entropy data ends inside a block" : "corrupt: Huffman code with no entry");
  if (s > 11) return fail(p, "corrupt: DC size above 11");
  if (s) {
    const int v = take(b, s);
    if (v < 0) return fail(p, "truncated: the entropy data ends inside a block");
    *pred += extend(v, s);
  }
  if (*pred < -32768 || *pred > 32767) return fail(p, "corrupt: DC value outside int16");
  blk[0] = (int16_t)*pred;
  for (int k = 1; k < 64;) {
    const int rs = decode_symbol(b, ac);
    if (rs < 0) return fail(p, rs == -1 ? "truncated: the entropy data ends inside a block" : "corrupt: Huffman code with no entry");
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;   // EOB
      k += 16;              // ZRL
      continue;
    }
    k += r;
    if (k > 63) return fail(p, "corrupt: coefficient index above 63");
    const int v = take(b, s);
    if (v < 0) return fail(p, "truncated: the entropy data ends inside a block");
    blk[kZigzag[k]] = (int16_t)extend(v, s);
    ++k;
  }
  return kOk;
}

// the marker the reader stopped at must be `want` (fill bytes FF may precede it); the bits left in the buffer are padding and are dropped
inline int expect_marker(Parser& p, Bits& b, int want, const char* what) {
  b.buf = 0;
  b.cnt = 0;
  p.pos = b.pos;
  if (b.pos >= b.n || b.d[b.pos] != 0xFF) return fail(p, what);
  while (b.pos < b.n && b.d[b.pos] == 0xFF) ++b.pos;
  p.pos = b.pos;
  if (b.pos >= b.n || b.d[b.pos] != want) return fail(p, what);
  ++b.pos;
  return kOk;
}

inline void init(Parser& p, const uint8_t* data, int64_t n, char* msg, size_t msgcap) {
  memset(&p, 0, sizeof(p));
  p.d = data;
  p.n = n;
  p.msg = msg;
  p.msgcap = msgcap;
  if (msg && msgcap) msg[0] = 0;
}

}  // namespace detail

// Parses SOI ... SOS: the frame's geometry and quantisation tables.  msg (may be null) receives the reason of a refusal.
inline int read_header(const uint8_t* data, int64_t n, Frame* out, char* msg, size_t msgcap) {
  static thread_local detail::Parser p;   // (about 10 KB of tables: kept off the stack)
  detail::init(p, data, n, msg, msgcap);
  if (!data || n < 0 || !out) return detail::fail(p, "null argument");
  const int rc = detail::parse_headers(p);
  if (rc) return rc;
  *out = p.f;
  return kOk;
}

// Parses the headers and decodes the scan into coef[0 .. coef_count); capacity: the int16 values coef can take.  *out (may be null) as
// read_header.  Nothing is written at or past coef + capacity; on a refusal coef holds the blocks decoded so far.
inline int entropy_decode(const uint8_t* data, int64_t n, Frame* out, int16_t* coef, int64_t capacity, char* msg, size_t msgcap) {
  using namespace detail;
  static thread_local Parser p;
  init(p, data, n, msg, msgcap);
  if (!data || n < 0 || !coef) return fail(p, "null argument");
  int rc = parse_headers(p);
  if (rc) return rc;
  const Frame& f = p.f;
  if (out) *out = f;
  if (capacity < f.coef_count) return fail(p, "capacity too small for the frame's coefficients");
  int16_t* plane[kMaxComponents];
  int64_t off = 0;
  for (int c = 0; c < f.components; ++c) {
    plane[c] = coef + off;
    off += (int64_t)64 * f.blocks_x[c] * f.blocks_y[c];
  }
  Bits b = {p.d, p.n, p.pos, 0, 0};
  int pred[kMaxComponents] = {0, 0, 0};
  const int64_t mcus = (int64_t)f.mcus_x * f.mcus_y;
  int to_restart = f.restart_interval, next_rst = 0;
  int mx = 0, my = 0;
  for (int64_t mcu = 0; mcu < mcus; ++mcu) {
    if (f.restart_interval && to_restart == 0) {
      rc = expect_marker(p, b, 0xD0 + next_rst, "corrupt: restart marker missing or out of order");
      if (rc) return rc;
      next_rst = (next_rst + 1) & 7;
      to_restart = f.restart_interval;
      pred[0] = pred[1] = pred[2] = 0;
    }
    for (int c = 0; c < f.components; ++c) {
      const Huffman& dc = p.huff[0][p.dc_tab[c]];
      const Huffman& ac = p.huff[1][p.ac_tab[c]];
      for (int vy = 0; vy < f.v[c]; ++vy)
        for (int hx = 0; hx < f.h[c]; ++hx) {
          const int64_t blk = (int64_t)(my * f.v[c] + vy) * f.blocks_x[c] + (mx * f.h[c] + hx);
          p.pos = b.pos;
          rc = decode_block(p, b, dc, ac, &pred[c], plane[c] + blk * 64);
          if (rc) return rc;
        }
    }
    --to_restart;
    if (++mx == f.mcus_x) {
      mx = 0;
      ++my;
    }
  }
  return expect_marker(p, b, 0xD9, "truncated or corrupt: no EOI marker after the scan");
}

}  // namespace ehm_jpeg
