// Baseline JPEG encoding on gfx950 (include/egohmr_hip.h, "JPEG encoding", states the rule: libjpeg's default encoder, all int32):
//   ehm_jpeg_forward         jpeg_forward_kernel   colour conversion + chroma downsampling + 8x8 forward DCT + quantisation + dummy blocks:
//                                                  uint8 [F,H,W,3] frames -> the quantised int16 coefficients ehm_jpeg_decode reads
//   ehm_jpeg_entropy_encode  jpeg_count_kernel     the bits of every block (its code length depends on the block and its predecessor's DC only)
//                            jpeg_scan_kernel      exclusive scan per frame: every block's bit offset
//                            jpeg_zero_kernel      the words the stream will occupy
//                            jpeg_pack_kernel      every block writes its bits at its offset (atomicOr on the words it shares with a neighbour)
//                            jpeg_ff_count_kernel  FF bytes per chunk of the packed stream; jpeg_scan_kernel again; jpeg_finish_kernel: lengths
//                            jpeg_stuff_kernel     the scatter that follows every FF with 00
// The scans are one workgroup per frame walking its elements in chunks: no workgroup ever waits on another one.  The host entries
// (ehm_jpeg_quality_tables, ehm_jpeg_write_header) live in jpeg_enc.h and make no device call.
#include "common.h"
#include "egohmr_hip.h"
#include "jpeg_enc.h"

namespace {

using ehm_jpeg_enc::CodeTable;
using ehm_jpeg_enc::kHuffman;
using ehm_jpeg_enc::make_codes;

constexpr int kThreads = 256;
constexpr int kBlocksPerGroup = kThreads / 8;   // eight lanes per 8x8 block, as in the decoder
constexpr int kSlotStride = 72;                 // dwords per block in LDS
constexpr int kScanChunk = EHM_JPEG_ENC_SCAN_CHUNK;
constexpr int kStuffChunk = EHM_JPEG_ENC_STUFF_CHUNK;
constexpr int kBlockWords = EHM_JPEG_ENC_MAX_BLOCK_BYTES / 4;   // a block is at most 22 + 63 * 26 = 1660 bits
static_assert(kScanChunk == kThreads && kStuffChunk == kThreads * 16, "the kernels below assume these");
static_assert(EHM_JPEG_ENC_HEADER_BYTES == ehm_jpeg_enc::kHeaderBytes, "header and writer disagree");

// (length << 16) | code by symbol: DC luma, AC luma, DC chroma, AC chroma
__constant__ CodeTable kCodes[4] = {make_codes(kHuffman[0]), make_codes(kHuffman[1]), make_codes(kHuffman[2]), make_codes(kHuffman[3])};

struct EncGeo {
  int H, W, hmax, vmax;
  int bx[3], by[3];      // the MCU-padded block grid per component
  int rw[3], rh[3];      // the real block grid
  int start[3];          // first block of each component's plane within a frame
  int blocks;            // blocks per frame
  int mcus_x, mcus_y, bpm;   // bpm: blocks per MCU
};

int make_geo(int H, int W, int hmax, int vmax, EncGeo* g) {
  EHM_CHECK_ARG(H > 0 && H <= 65535 && W > 0 && W <= 65535);
  EHM_CHECK_ARG(ehm_jpeg_enc::sampling_ok(hmax, vmax));
  g->H = H, g->W = W, g->hmax = hmax, g->vmax = vmax;
  g->mcus_x = (int)ceil_div(W, 8 * hmax), g->mcus_y = (int)ceil_div(H, 8 * vmax);
  g->bpm = hmax * vmax + 2;
  int64_t total = 0;
  for (int c = 0; c < 3; ++c) {
    const int h = c == 0 ? hmax : 1, v = c == 0 ? vmax : 1;
    g->bx[c] = g->mcus_x * h, g->by[c] = g->mcus_y * v;
    g->rw[c] = (int)ceil_div((int64_t)W * h, 8 * hmax), g->rh[c] = (int)ceil_div((int64_t)H * v, 8 * vmax);
    g->start[c] = (int)total;
    total += (int64_t)g->bx[c] * g->by[c];
  }
  EHM_CHECK_ARG(total * 64 < (1ll << 31));     // a frame's coefficient offsets are ints in the kernels, as in the decoder
  g->blocks = (int)total;
  return 0;
}

constexpr int fix16(double v) { return (int)(v * 65536.0 + 0.5); }

// One component of one pixel (jccolor.c)
__device__ __forceinline__ int ycc(const uint8_t* __restrict__ p, const int c, const int rgb) {
  const int r = p[rgb ? 0 : 2], g = p[1], b = p[rgb ? 2 : 0];
  if (c == 0) return (fix16(.29900) * r + fix16(.58700) * g + fix16(.11400) * b + 32768) >> 16;
  if (c == 1) return (-fix16(.16874) * r - fix16(.33126) * g + fix16(.50000) * b + (128 << 16) + 32767) >> 16;
  return (fix16(.50000) * r - fix16(.41869) * g - fix16(.08131) * b + (128 << 16) + 32767) >> 16;
}

// Sample (sy, sx) of component c's plane on its real block grid: the padding and downsampling rule of the header.  Every pixel index is
// clamped into the frame, so nothing outside it is read.
__device__ __forceinline__ int sample(const EncGeo& g, const uint8_t* __restrict__ frame, const int c, const int sy, const int sx, const int rgb) {
  const int64_t W = g.W;
  if (c == 0 || g.hmax == 1) return ycc(frame + ((int64_t)min(sy, g.H - 1) * W + min(sx, g.W - 1)) * 3, c, rgb);
  const int x0 = min(2 * sx, g.W - 1), x1 = min(2 * sx + 1, g.W - 1);
  if (g.vmax == 1) {
    const uint8_t* row = frame + (int64_t)min(sy, g.H - 1) * W * 3;
    return (ycc(row + x0 * 3, c, rgb) + ycc(row + x1 * 3, c, rgb) + (sx & 1)) >> 1;
  }
  const int cy = min(sy, ((g.H + 1) >> 1) - 1);                       // rows past the downsampled plane repeat ITS last row
  const uint8_t* r0 = frame + (int64_t)min(2 * cy, g.H - 1) * W * 3;
  const uint8_t* r1 = frame + (int64_t)min(2 * cy + 1, g.H - 1) * W * 3;
  return (ycc(r0 + x0 * 3, c, rgb) + ycc(r0 + x1 * 3, c, rgb) + ycc(r1 + x0 * 3, c, rgb) + ycc(r1 + x1 * 3, c, rgb) + 1 + (sx & 1)) >> 2;
}

__device__ __forceinline__ int descale(const int x, const int n) { return (x + (1 << (n - 1))) >> n; }

// One 1-D pass of jfdctint over x[0..7], in place.
template <bool kFirst>
__device__ __forceinline__ void fdct_pass(int (&x)[8]) {
  constexpr int n = kFirst ? 11 : 15;
  const int t0 = x[0] + x[7], t1 = x[1] + x[6], t2 = x[2] + x[5], t3 = x[3] + x[4];
  int t7 = x[0] - x[7], t6 = x[1] - x[6], t5 = x[2] - x[5], t4 = x[3] - x[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  x[0] = kFirst ? (t10 + t11) << 2 : descale(t10 + t11, 2);
  x[4] = kFirst ? (t10 - t11) << 2 : descale(t10 - t11, 2);
  int z1 = (t12 + t13) * 4433;
  x[2] = descale(z1 + t13 * 6270, n);
  x[6] = descale(z1 - t12 * 15137, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;
  z1 *= -7373, z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  x[7] = descale(t4 + z1 + z3, n);
  x[5] = descale(t5 + z2 + z4, n);
  x[3] = descale(t6 + z2 + z3, n);
  x[1] = descale(t7 + z1 + z4, n);
}

// Eight lanes per block.  Lane j gathers row j of the block's samples, runs the row pass, hands the rows over through LDS, runs column j,
// quantises it, hands the block back and stores row j of the coefficients (16 bytes; a wave writes 1 KiB of contiguous coefficients).  A dummy
// block of the MCU padding transforms the real block it takes its DC from - the same arithmetic, so the same value - and stores zeros elsewhere.
__global__ __launch_bounds__(kThreads) void jpeg_forward_kernel(const EncGeo g, const uint8_t* __restrict__ frames, const uint16_t* __restrict__ quant,
                                                                int16_t* __restrict__ coef, const int64_t total, const int rgb) {
  __shared__ int ws[kBlocksPerGroup * kSlotStride];
  const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
  const int64_t blk = (int64_t)blockIdx.x * kBlocksPerGroup + slot;
  const bool ok = blk < total;
  int* w = ws + slot * kSlotStride;
  int64_t f = 0;
  int r = 0, c = 0;
  bool dummy = false;
  int x[8];
  if (ok) {
    f = blk / g.blocks;
    r = (int)(blk - f * g.blocks);
    c = r >= g.start[2] ? 2 : (r >= g.start[1] ? 1 : 0);
    const int rc = r - g.start[c];
    const int by = rc / g.bx[c], bx = rc - by * g.bx[c];
    const int h = c == 0 ? g.hmax : 1;
    int sby = by, sbx = bx;
    if (by >= g.rh[c]) sby = by - 1, sbx = (bx / h) * h + h - 1;      // a dummy row: the MCU's last block of the row above ...
    sbx = min(sbx, g.rw[c] - 1);                                      // ... which, like a dummy column of a real row, takes the block to its left
    dummy = sby != by || sbx != bx;
    const uint8_t* frame = frames + f * ((int64_t)g.H * g.W * 3);
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = sample(g, frame, c, sby * 8 + j, sbx * 8 + k, rgb) - 128;
    fdct_pass<true>(x);
#pragma unroll
    for (int k = 0; k < 8; ++k) w[j * 8 + k] = x[k];
  }
  __syncthreads();
  if (ok) {
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = w[k * 8 + j];
    fdct_pass<false>(x);
  }
  __syncthreads();
  if (ok) {
    const uint16_t* q = quant + (f * 3 + c) * 64;
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                    // x[k]: the coefficient of row k, column j
      const int d = 8 * (int)q[k * 8 + j];
      const int a = abs(x[k]) + (d >> 1);
      const int v = a >= d ? a / d : 0;
      w[k * 8 + j] = (dummy && (k | j)) ? 0 : (x[k] < 0 ? -v : v);
    }
  }
  __syncthreads();
  if (ok) {
    unsigned int o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = ((unsigned int)w[j * 8 + 2 * i] & 0xffffu) | ((unsigned int)w[j * 8 + 2 * i + 1] << 16);
    *(uint4*)(coef + (f * g.blocks + r) * 64 + j * 8) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// ---------------------------------------------------------------------------------------------------- entropy coding

constexpr int zig(const int k) {
  constexpr uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return z[k];
}

// Block i (luma in raster order, then Cb, Cr) of MCU m: its component and its index within a frame's coefficient blocks.
__device__ __forceinline__ int scan_block(const EncGeo& g, const int m, const int i, int* comp) {
  const int my = m / g.mcus_x, mx = m - my * g.mcus_x, nl = g.hmax * g.vmax;
  if (i < nl) {
    const int vy = i / g.hmax, hx = i - vy * g.hmax;
    *comp = 0;
    return (my * g.vmax + vy) * g.bx[0] + mx * g.hmax + hx;
  }
  *comp = 1 + i - nl;
  return g.start[*comp] + my * g.bx[*comp] + mx;
}

struct BitCount {
  unsigned int n = 0;
  __device__ __forceinline__ void put(unsigned int, int len) { n += len; }
};

// Bits go out most significant first; word k of a frame holds the stream's bytes 4k .. 4k + 3 with byte 4k in its top eight bits.
struct BitPack {
  unsigned int* words;
  int64_t w, wcap;
  unsigned long long acc;
  int fill;
  bool first;
  __device__ __forceinline__ void put(unsigned int bits, int len) {
    acc = (acc << len) | bits;
    fill += len;
    if (fill >= 32) {
      fill -= 32;
      const unsigned int word = (unsigned int)(acc >> fill);
      if (w < wcap) {
        if (first) atomicOr(words + w, word);      // shared with the block before
        else words[w] = word;                      // wholly this block's
      }
      first = false;
      ++w;
      acc &= (1ull << fill) - 1;
    }
  }
  __device__ __forceinline__ void flush() {
    if (fill && w < wcap) atomicOr(words + w, (unsigned int)(acc << (32 - fill)));   // shared with the block after
  }
};

// The Huffman code of one block (table set t: 0 luma, 1 chroma) into sink.  A DC difference beyond 11 bits or an AC value beyond 10 has no
// code: it is clamped, so a block never exceeds kBlockWords, and *bad is set.
template <class Sink>
__device__ __forceinline__ void encode_block(const int16_t* __restrict__ blk, const int pred, const int t, Sink& sink, bool* bad) {
  int c[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 v = ((const uint4*)blk)[i];
    const unsigned int u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) c[i * 8 + 2 * k] = (int)(short)(u[k] & 0xffffu), c[i * 8 + 2 * k + 1] = (int)u[k] >> 16;
  }
  const CodeTable& dc = kCodes[2 * t];
  const CodeTable& ac = kCodes[2 * t + 1];
  int d = c[0] - pred;
  if (d < -2047 || d > 2047) *bad = true, d = max(-2047, min(2047, d));
  int s = 32 - __clz(abs(d));
  unsigned int e = dc.e[s];
  sink.put(e & 0xffffu, (int)(e >> 16));
  if (s) sink.put((unsigned int)(d - (d < 0)) & ((1u << s) - 1), s);
  int run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    int v = c[zig(k)];
    if (v == 0) {
      ++run;
      continue;
    }
    while (run > 15) {
      e = ac.e[0xF0];
      sink.put(e & 0xffffu, (int)(e >> 16));
      run -= 16;
    }
    if (v < -1023 || v > 1023) *bad = true, v = max(-1023, min(1023, v));
    s = 32 - __clz(abs(v));
    e = ac.e[(run << 4) | s];
    sink.put(e & 0xffffu, (int)(e >> 16));
    sink.put((unsigned int)(v - (v < 0)) & ((1u << s) - 1), s);
    run = 0;
  }
  if (run) {
    e = ac.e[0x00];
    sink.put(e & 0xffffu, (int)(e >> 16));
  }
}

// One thread per block in SCAN order (blockIdx.y: the frame).  pack: false counts the block's bits, true writes them at offs[].
template <bool kPack>
__global__ __launch_bounds__(kThreads) void jpeg_code_kernel(const EncGeo g, const int16_t* __restrict__ coef, unsigned int* __restrict__ bits,
                                                             const unsigned long long* __restrict__ offs, unsigned int* __restrict__ words,
                                                             const int64_t wcap, unsigned int* __restrict__ status) {
  const int s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= g.blocks) return;
  const int64_t f = blockIdx.y;
  const int m = s / g.bpm, i = s - m * g.bpm;
  int c, pc;
  const int b = scan_block(g, m, i, &c);
  const int16_t* base = coef + f * ((int64_t)g.blocks * 64);
  int pred = 0;                                                        // the previous block of the same component in scan order
  if (c == 0 && i > 0) pred = base[(int64_t)scan_block(g, m, i - 1, &pc) * 64];
  else if (m > 0) pred = base[(int64_t)scan_block(g, m - 1, c == 0 ? g.hmax * g.vmax - 1 : i, &pc) * 64];
  bool bad = false;
  if (!kPack) {
    BitCount sink;
    encode_block(base + (int64_t)b * 64, pred, c ? 1 : 0, sink, &bad);
    bits[f * g.blocks + s] = sink.n;
    if (bad) atomicOr(status + f, 1u);
  } else {
    const unsigned long long off = offs[f * g.blocks + s];
    BitPack sink = {words + f * wcap, (int64_t)(off >> 5), wcap, 0ull, (int)(off & 31), true};
    encode_block(base + (int64_t)b * 64, pred, c ? 1 : 0, sink, &bad);
    sink.flush();
  }
}

// Exclusive scan of in[f][0 .. n) into out[f][0 .. n) and the sum into total[f]: ONE workgroup per frame walks its row kScanChunk elements at
// a time and carries the running sum itself.
__global__ __launch_bounds__(kThreads) void jpeg_scan_kernel(const unsigned int* __restrict__ in, unsigned long long* __restrict__ out, const int64_t n,
                                                             unsigned long long* __restrict__ total) {
  __shared__ unsigned long long wsum[kThreads / 64];
  const int64_t f = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  in += f * n, out += f * n;
  unsigned long long carry = 0;
  for (int64_t base = 0; base < n; base += kScanChunk) {
    const int64_t i = base + threadIdx.x;
    const unsigned long long v = i < n ? in[i] : 0;
    unsigned long long x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) {
      if (k < wave) before += wsum[k];
      all += wsum[k];
    }
    if (i < n) out[i] = carry + before + x - v;
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) total[f] = carry;
}

// Zeroes the words frame blockIdx.y's stream will occupy (rounded up to 16 bytes; wcap is a multiple of 4 words).
__global__ __launch_bounds__(kThreads) void jpeg_zero_kernel(unsigned int* __restrict__ words, const int64_t wcap,
                                                             const unsigned long long* __restrict__ total_bits) {
  const int64_t f = blockIdx.y, q = (int64_t)blockIdx.x * kThreads + threadIdx.x;     // q: a group of four words
  const int64_t used = min((int64_t)(total_bits[f] >> 5) + 1, wcap);
  if (q * 4 < used) ((uint4*)(words + f * wcap))[q] = make_uint4(0, 0, 0, 0);
}

// Word k of a frame's packed stream, the 1 bits that pad its last byte included.
__device__ __forceinline__ unsigned int stream_word(const unsigned int* __restrict__ words, const int64_t k, const unsigned long long total_bits) {
  unsigned int w = words[k];
  const int nb = (int)(total_bits & 31), pad = (8 - (nb & 7)) & 7;
  if (pad && k == (int64_t)(total_bits >> 5)) w |= ((1u << pad) - 1) << (32 - nb - pad);
  return w;
}

// The FF bytes among a thread's 16 bytes [b0, b0 + 16) of a stream of nbytes bytes; the four words are left in w[].
__device__ __forceinline__ int load16(const unsigned int* __restrict__ words, const int64_t b0, const int64_t nbytes, const unsigned long long total_bits,
                                      unsigned int (&w)[4]) {
  int cnt = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    w[q] = b0 + 4 * q < nbytes ? stream_word(words, (b0 >> 2) + q, total_bits) : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt += (b0 + 4 * q + k < nbytes) && ((w[q] >> (24 - 8 * k)) & 0xffu) == 0xffu;
  }
  return cnt;
}

// The sum of v over the workgroup's threads before this one (exclusive) and, in *all, over every thread.
__device__ __forceinline__ int block_exclusive(const int v, int* all) {
  __shared__ int wsum[kThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  int before = 0, sum = 0;
#pragma unroll
  for (int k = 0; k < kThreads / 64; ++k) {
    if (k < wave) before += wsum[k];
    sum += wsum[k];
  }
  *all = sum;
  return before + x - v;
}

// Workgroup (chunk, frame): the FF bytes among the chunk's kStuffChunk bytes (0 for a chunk past the stream's end).
__global__ __launch_bounds__(kThreads) void jpeg_ff_count_kernel(const unsigned int* __restrict__ words, const int64_t wcap,
                                                                 const unsigned long long* __restrict__ total_bits, unsigned int* __restrict__ ffcount) {
  const int64_t f = blockIdx.y;
  const unsigned long long tb = total_bits[f];
  const int64_t nbytes = (int64_t)((tb + 7) >> 3);
  unsigned int w[4];
  int all;
  block_exclusive(load16(words + f * wcap, (int64_t)blockIdx.x * kStuffChunk + threadIdx.x * 16, nbytes, tb, w), &all);
  if (threadIdx.x == 0) ffcount[f * gridDim.x + blockIdx.x] = (unsigned int)all;
}

// needed = packed bytes + FF bytes; lengths = needed, -1 when it exceeds the capacity, -2 when a coefficient had no code.
__global__ void jpeg_finish_kernel(const unsigned long long* __restrict__ total_bits, const unsigned long long* __restrict__ fftotal,
                                   const unsigned int* __restrict__ status, const int64_t capacity, const int F, int64_t* __restrict__ lengths,
                                   int64_t* __restrict__ needed) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const int64_t n = (int64_t)((total_bits[f] + 7) >> 3) + (int64_t)fftotal[f];
  needed[f] = status[f] ? 0 : n;
  lengths[f] = status[f] ? -2 : (n <= capacity ? n : -1);
}

// Workgroup (chunk, frame): byte i of the packed stream goes to i + (FF bytes before it), a 00 behind every FF.  A flagged frame is left alone,
// and nothing is written at or past capacity.
__global__ __launch_bounds__(kThreads) void jpeg_stuff_kernel(const unsigned int* __restrict__ words, const int64_t wcap,
                                                              const unsigned long long* __restrict__ total_bits,
                                                              const unsigned long long* __restrict__ ffoff, const int64_t* __restrict__ lengths,
                                                              uint8_t* __restrict__ streams, const int64_t capacity) {
  const int64_t f = blockIdx.y;
  const unsigned long long tb = total_bits[f];
  const int64_t nbytes = (int64_t)((tb + 7) >> 3), b0 = (int64_t)blockIdx.x * kStuffChunk + threadIdx.x * 16;
  unsigned int w[4];
  int all;
  const int before = block_exclusive(load16(words + f * wcap, b0, nbytes, tb, w), &all);
  if (lengths[f] < 0 || b0 >= nbytes) return;
  int64_t pos = b0 + (int64_t)ffoff[f * gridDim.x + blockIdx.x] + before;
  uint8_t* out = streams + f * capacity;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (b0 + k >= nbytes) break;
    const unsigned int b = (w[k >> 2] >> (24 - 8 * (k & 3))) & 0xffu;
    if (pos < capacity) out[pos] = (uint8_t)b;
    ++pos;
    if (b == 0xffu) {
      if (pos < capacity) out[pos] = 0;
      ++pos;
    }
  }
}

// The workspace of ehm_jpeg_entropy_encode: byte offsets of its parts, every one a multiple of 16.
struct EncPlan {
  int64_t wcap, chunks;                                                 // words and stuffing chunks per frame
  int64_t total_bits, fftotal, status, bits, offs, ffcount, ffoff, words, bytes;
};

void make_plan(const EncGeo& g, int F, EncPlan* p) {
  p->wcap = round_up((int64_t)g.blocks * kBlockWords + 1, 4);
  p->chunks = ceil_div(p->wcap * 4, kStuffChunk);
  int64_t at = 0;
  auto take = [&at](int64_t bytes) {
    const int64_t o = at;
    at += round_up(bytes, 16);
    return o;
  };
  p->total_bits = take((int64_t)F * 8);
  p->fftotal = take((int64_t)F * 8);
  p->status = take((int64_t)F * 4);
  p->bits = take((int64_t)F * g.blocks * 4);
  p->offs = take((int64_t)F * g.blocks * 8);
  p->ffcount = take((int64_t)F * p->chunks * 4);
  p->ffoff = take((int64_t)F * p->chunks * 8);
  p->words = take((int64_t)F * p->wcap * 4);
  p->bytes = at;
}

}  // namespace

extern "C" int ehm_jpeg_quality_tables(int quality, uint16_t* quant) {
  char msg[128];
  if (ehm_jpeg_enc::quality_tables(quality, (uint16_t(*)[64])quant, msg, sizeof msg)) {
    ehm_set_error("%s", msg);
    return EHM_EINVAL;
  }
  return 0;
}

extern "C" int ehm_jpeg_write_header(int H, int W, int hmax, int vmax, const uint16_t* quant, uint8_t* out, int64_t capacity, int64_t* n) {
  char msg[128];
  if (ehm_jpeg_enc::write_header(H, W, hmax, vmax, (const uint16_t(*)[64])quant, out, capacity, n, msg, sizeof msg)) {
    ehm_set_error("%s", msg);
    return EHM_EINVAL;
  }
  return 0;
}

extern "C" int ehm_jpeg_forward(const ehm_jpeg_forward_desc* d, void* stream) {
  EHM_CHECK_ARG(d && d->frames && d->quant && d->coef && d->F > 0 && d->F <= 65535);
  EncGeo g;
  if (int rc = make_geo(d->H, d->W, d->hmax, d->vmax, &g)) return rc;
  EHM_CHECK_ARG(((uintptr_t)d->coef & 15) == 0 && ((uintptr_t)d->quant & 1) == 0);
  const int64_t total = (int64_t)d->F * g.blocks;
  EHM_CHECK_ARG(ceil_div(total, kBlocksPerGroup) < (1ll << 31));
  hipLaunchKernelGGL(jpeg_forward_kernel, dim3((unsigned)ceil_div(total, kBlocksPerGroup)), dim3(kThreads), 0, (hipStream_t)stream, g, d->frames,
                     d->quant, d->coef, total, d->rgb ? 1 : 0);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_jpeg_entropy_encode_workspace_bytes(const ehm_jpeg_entropy_encode_desc* d, int64_t* bytes) {
  EHM_CHECK_ARG(d && bytes && d->F > 0 && d->F <= 65535);
  EncGeo g;
  if (int rc = make_geo(d->H, d->W, d->hmax, d->vmax, &g)) return rc;
  EncPlan p;
  make_plan(g, d->F, &p);
  *bytes = p.bytes;
  return 0;
}

extern "C" int ehm_jpeg_entropy_encode(const ehm_jpeg_entropy_encode_desc* d, void* stream) {
  EHM_CHECK_ARG(d && d->coef && d->streams && d->lengths && d->needed && d->workspace && d->F > 0 && d->F <= 65535 && d->capacity >= 0);
  EncGeo g;
  if (int rc = make_geo(d->H, d->W, d->hmax, d->vmax, &g)) return rc;
  EncPlan p;
  make_plan(g, d->F, &p);
  EHM_CHECK_ARG(d->workspace_bytes >= p.bytes);
  EHM_CHECK_ARG(((uintptr_t)d->coef & 15) == 0 && ((uintptr_t)d->workspace & 15) == 0 && ((uintptr_t)d->lengths & 7) == 0 &&
                ((uintptr_t)d->needed & 7) == 0);
  EHM_CHECK_ARG(p.chunks < (1ll << 31) && ceil_div(p.wcap / 4, kThreads) < (1ll << 31));
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)d->workspace;
  auto* total_bits = (unsigned long long*)(ws + p.total_bits);
  auto* fftotal = (unsigned long long*)(ws + p.fftotal);
  auto* status = (unsigned int*)(ws + p.status);
  auto* bits = (unsigned int*)(ws + p.bits);
  auto* offs = (unsigned long long*)(ws + p.offs);
  auto* ffcount = (unsigned int*)(ws + p.ffcount);
  auto* ffoff = (unsigned long long*)(ws + p.ffoff);
  auto* words = (unsigned int*)(ws + p.words);
  const dim3 F((unsigned)d->F), T(kThreads);
  const dim3 per_block((unsigned)ceil_div(g.blocks, kThreads), (unsigned)d->F), per_chunk((unsigned)p.chunks, (unsigned)d->F);
  EHM_HIP(hipMemsetAsync(status, 0, (size_t)d->F * 4, st));
  hipLaunchKernelGGL(jpeg_code_kernel<false>, per_block, T, 0, st, g, d->coef, bits, (const unsigned long long*)nullptr, (unsigned int*)nullptr,
                     p.wcap, status);
  EHM_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_scan_kernel, F, T, 0, st, (const unsigned int*)bits, offs, (int64_t)g.blocks, total_bits);
  EHM_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_zero_kernel, dim3((unsigned)ceil_div(p.wcap / 4, kThreads), (unsigned)d->F), T, 0, st, words, p.wcap,
                     (const unsigned long long*)total_bits);
  EHM_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_code_kernel<true>, per_block, T, 0, st, g, d->coef, bits, (const unsigned long long*)offs, words, p.wcap, status);
  EHM_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_ff_count_kernel, per_chunk, T, 0, st, (const unsigned int*)words, p.wcap, (const unsigned long long*)total_bits, ffcount);
  EHM_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_scan_kernel, F, T, 0, st, (const unsigned int*)ffcount, ffoff, p.chunks, fftotal);
  EHM_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_finish_kernel, dim3((unsigned)ceil_div(d->F, kThreads)), T, 0, st, (const unsigned long long*)total_bits,
                     (const unsigned long long*)fftotal, (const unsigned int*)status, d->capacity, d->F, d->lengths, d->needed);
  EHM_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_stuff_kernel, per_chunk, T, 0, st, (const unsigned int*)words, p.wcap, (const unsigned long long*)total_bits,
                     (const unsigned long long*)ffoff, (const int64_t*)d->lengths, d->streams, d->capacity);
  EHM_LAUNCH_CHECK();
  return 0;
}
