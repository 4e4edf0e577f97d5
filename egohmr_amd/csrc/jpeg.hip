// Baseline JPEG on gfx950: the C ABI of the host entropy stage (jpeg_entropy.h) and the two kernels behind ehm_jpeg_decode
// (include/egohmr_hip.h, "JPEG decoding", states the pixel rule: libjpeg's ISLOW IDCT, fancy upsampling and colour tables, all int32):
//   jpeg_idct_kernel    dequantisation + 8x8 inverse DCT: quantised int16 coefficients -> uint8 component planes on the MCU grid (workspace)
//   jpeg_colour_kernel  chroma upsampling + YCbCr -> BGR: the planes -> the interleaved uint8 [F,H,W,3] frames
// Both are bandwidth-bound streaming kernels (per 1920 x 1080 4:2:0 frame: 6.3 MB of coefficients in, 3.1 MB of planes out and in again,
// 6.2 MB of pixels out).  They stay two launches: fusing them would need each colour tile's chroma neighbours from the blocks around it - a
// halo of re-done IDCTs or a second pass - for 3.1 MB + 3.1 MB of plane traffic that the L2 / Infinity Cache mostly absorbs.
// No atomics, every byte written once by one thread: two calls give the same bits.
#include "common.h"
#include "egohmr_hip.h"
#include "jpeg_entropy.h"

#include <type_traits>

namespace {

constexpr int kThreads = 256;
constexpr int kBlocksPerGroup = kThreads / 8;   // eight lanes per 8x8 block: a wave handles eight blocks, a workgroup 32
constexpr int kSlotStride = 72;                 // dwords per block in LDS: 64 + 8, so the four blocks of a 32-lane half sit on different banks

// The block grids that follow from (H, W, components, hmax, vmax); chroma is always (1,1).
struct JpegGeo {
  int H, W, components, hmax, vmax;
  int bx[3], by[3];
  int start[3];        // first block of each component's plane within a frame (start[c] * 64: its first sample / coefficient)
  int blocks;          // blocks per frame
  int cw, ch;          // the chroma planes' real size
};

int make_geo(const ehm_jpeg_decode_desc* d, JpegGeo* g) {
  EHM_CHECK_ARG(d->H > 0 && d->H <= 65535 && d->W > 0 && d->W <= 65535);
  EHM_CHECK_ARG(d->components == 1 || d->components == 3);
  if (d->components == 1) EHM_CHECK_ARG(d->hmax == 1 && d->vmax == 1);
  else EHM_CHECK_ARG((d->hmax == 1 && d->vmax == 1) || (d->hmax == 2 && d->vmax == 1) || (d->hmax == 2 && d->vmax == 2));
  g->H = d->H, g->W = d->W, g->components = d->components, g->hmax = d->hmax, g->vmax = d->vmax;
  const int mx = (int)ceil_div(d->W, 8 * d->hmax), my = (int)ceil_div(d->H, 8 * d->vmax);
  int64_t total = 0;
  for (int c = 0; c < 3; ++c) {
    const bool present = c < d->components;
    g->bx[c] = present ? mx * (c == 0 ? d->hmax : 1) : 0;
    g->by[c] = present ? my * (c == 0 ? d->vmax : 1) : 0;
    g->start[c] = (int)total;
    total += (int64_t)g->bx[c] * g->by[c];
  }
  EHM_CHECK_ARG(total * 64 < (1ll << 31));     // a frame's sample offsets are ints in the kernels (65535 x 8192 would still pass)
  g->blocks = (int)total;
  g->cw = (int)ceil_div(d->W, d->hmax);
  g->ch = (int)ceil_div(d->H, d->vmax);
  return 0;
}

// One 1-D pass of jidctint over x[0..7], in place.
__device__ __forceinline__ void idct_pass(int (&x)[8], const int shift, const int round_) {
  int z1 = (x[2] + x[6]) * 4433;
  const int t2 = z1 - x[6] * 15137;
  const int t3 = z1 + x[2] * 6270;
  const int t0 = ((x[0] + x[4]) << 13) + round_;
  const int t1 = ((x[0] - x[4]) << 13) + round_;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a0 = x[7], a1 = x[5], a2 = x[3], a3 = x[1];
  z1 = a0 + a3;
  int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const int z5 = (z3 + z4) * 9633;
  a0 *= 2446, a1 *= 16819, a2 *= 25172, a3 *= 12299;
  z1 *= -7373, z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4;
  x[0] = (t10 + a3) >> shift, x[7] = (t10 - a3) >> shift;
  x[1] = (t11 + a2) >> shift, x[6] = (t11 - a2) >> shift;
  x[2] = (t12 + a1) >> shift, x[5] = (t12 - a1) >> shift;
  x[3] = (t13 + a0) >> shift, x[4] = (t13 - a0) >> shift;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Eight lanes per block.  Lane j loads row j of the coefficients and of the table (16 bytes each, so a wave reads 1 KiB of contiguous
// coefficients), dequantises it into LDS, runs column j, hands the intermediate back through LDS, runs row j and stores its 8 samples.
__global__ __launch_bounds__(kThreads) void jpeg_idct_kernel(const JpegGeo g, const int16_t* __restrict__ coef, const uint16_t* __restrict__ quant,
                                                             uint8_t* __restrict__ planes, const int64_t total) {
  __shared__ int ws[kBlocksPerGroup * kSlotStride];
  const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
  const int64_t blk = (int64_t)blockIdx.x * kBlocksPerGroup + slot;
  const bool ok = blk < total;
  int* w = ws + slot * kSlotStride;
  int64_t f = 0;
  int r = 0, c = 0;
  if (ok) {
    f = blk / g.blocks;
    r = (int)(blk - f * g.blocks);                                    // the block's index within its frame = its place in the coefficients
    c = (g.components == 3 && r >= g.start[2]) ? 2 : ((g.components == 3 && r >= g.start[1]) ? 1 : 0);
    const uint4 cv = *(const uint4*)(coef + (f * g.blocks + r) * 64 + j * 8);
    const uint4 qv = *(const uint4*)(quant + (f * 3 + c) * 64 + j * 8);
    const unsigned int cw4[4] = {cv.x, cv.y, cv.z, cv.w}, qw4[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[j * 8 + 2 * i] = (int)(short)(cw4[i] & 0xffffu) * (int)(qw4[i] & 0xffffu);
      w[j * 8 + 2 * i + 1] = ((int)cw4[i] >> 16) * (int)(qw4[i] >> 16);
    }
  }
  __syncthreads();
  int x[8];
  if (ok) {
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = w[k * 8 + j];
    idct_pass(x, 11, 1 << 10);
  }
  __syncthreads();
  if (ok) {
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k * 8 + j] = x[k];
  }
  __syncthreads();
  if (ok) {
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = w[j * 8 + k];
    idct_pass(x, 18, 1 << 17);
    unsigned int lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (unsigned int)clamp255(x[k] + 128) << (8 * k);
      hi |= (unsigned int)clamp255(x[k + 4] + 128) << (8 * k);
    }
    const int rc = r - g.start[c];
    const int by = rc / g.bx[c], bx = rc - by * g.bx[c];
    uint8_t* dst = planes + f * ((int64_t)g.blocks * 64) + (int64_t)g.start[c] * 64 + ((int64_t)(by * 8 + j) * g.bx[c] + bx) * 8;
    *(uint2*)dst = make_uint2(lo, hi);
  }
}

// Six chroma samples i0 - 1 ... i0 + 4 of one plane row for a lane's eight output pixels (i0 = x0 / 2, a multiple of 4), indices clamped to
// the plane's real width cw: away from the right edge one aligned dword and its two neighbours, else byte by byte.
__device__ __forceinline__ void chroma_row6(const uint8_t* __restrict__ row, int i0, int cw, int (&s)[6]) {
  if (i0 + 4 <= cw - 1) {
    const unsigned int m = *(const unsigned int*)(row + i0);
    s[0] = row[max(i0 - 1, 0)];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[1 + k] = (int)((m >> (8 * k)) & 0xffu);
    s[5] = row[i0 + 4];
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = row[min(max(i0 - 1 + k, 0), cw - 1)];
  }
}

// One chroma plane's eight upsampled samples for the pixels x0 ... x0 + 7 of row y (the rule of the header).
__device__ __forceinline__ void chroma8(const uint8_t* __restrict__ P, int sc, int cw, int ch, int hmax, int vmax, int x0, int y, int (&c)[8]) {
  if (hmax == 1) {                                                     // 4:4:4: the samples themselves (8 aligned bytes inside the padded row)
    const uint2 m = *(const uint2*)(P + y * sc + x0);
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = (int)((m.x >> (8 * k)) & 0xffu), c[4 + k] = (int)((m.y >> (8 * k)) & 0xffu);
    return;
  }
  const int cy = vmax == 2 ? (y >> 1) : y;
  int s[6];
  chroma_row6(P + cy * sc, x0 >> 1, cw, s);
  if (cw <= 2) {                                                       // libjpeg replicates a plane this narrow
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = s[1 + (j >> 1)];
    return;
  }
  if (vmax == 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c[2 * k] = (3 * s[1 + k] + s[k] + 1) >> 2;
      c[2 * k + 1] = (3 * s[1 + k] + s[2 + k] + 2) >> 2;
    }
    return;
  }
  int n[6];
  chroma_row6(P + ((y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0)) * sc, x0 >> 1, cw, n);
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = 3 * s[k] + n[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    c[2 * k] = (3 * s[1 + k] + s[k] + 8) >> 4;
    c[2 * k + 1] = (3 * s[1 + k] + s[2 + k] + 7) >> 4;
  }
}

constexpr int fix16(double v) { return (int)(v * 65536.0 + 0.5); }

// One thread: eight consecutive pixels of one row of one frame (blockIdx.y) = 24 contiguous bytes; a wave writes 1536 contiguous bytes.
// wide: W % 8 == 0 and 8-byte aligned frames, so every thread's run is whole and aligned (three 8-byte stores); else it is written byte by byte.
__global__ __launch_bounds__(kThreads) void jpeg_colour_kernel(const JpegGeo g, const uint8_t* __restrict__ planes, uint8_t* __restrict__ frames,
                                                               const int wide) {
  const int octs = (g.W + 7) >> 3;
  const int q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= octs * g.H) return;
  const int y = q / octs, x0 = (q - y * octs) << 3;
  const int64_t f = blockIdx.y;
  const uint8_t* P0 = planes + f * ((int64_t)g.blocks * 64);
  const uint2 y8 = *(const uint2*)(P0 + y * (g.bx[0] * 8) + x0);          // the row stride is a multiple of 8: aligned, and inside the padded row
  int Y[8], cb[8], cr[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) Y[k] = (int)((y8.x >> (8 * k)) & 0xffu), Y[4 + k] = (int)((y8.y >> (8 * k)) & 0xffu);
  if (g.components == 3) {
    const int sc = g.bx[1] * 8;
    chroma8(P0 + (int64_t)g.start[1] * 64, sc, g.cw, g.ch, g.hmax, g.vmax, x0, y, cb);
    chroma8(P0 + (int64_t)g.start[2] * 64, sc, g.cw, g.ch, g.hmax, g.vmax, x0, y, cr);
  }
  unsigned int out[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int B = Y[i], G = Y[i], R = Y[i];
    if (g.components == 3) {
      const int u = cb[i] - 128, v = cr[i] - 128;
      R = Y[i] + ((fix16(1.40200) * v + 32768) >> 16);
      B = Y[i] + ((fix16(1.77200) * u + 32768) >> 16);
      G = Y[i] + ((-fix16(0.34414) * u + (-fix16(0.71414) * v + 32768)) >> 16);
    }
    const int bgr[3] = {clamp255(B), clamp255(G), clamp255(R)};
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(3 * i + k) >> 2] |= (unsigned int)bgr[k] << (8 * ((3 * i + k) & 3));
  }
  uint8_t* dst = frames + ((f * g.H + y) * g.W + x0) * 3;
  if (wide) {
#pragma unroll
    for (int k = 0; k < 3; ++k) ((uint2*)dst)[k] = make_uint2(out[2 * k], out[2 * k + 1]);
  } else {
    const int n = min(8, g.W - x0) * 3;
    for (int k = 0; k < n; ++k) dst[k] = (uint8_t)(out[k >> 2] >> (8 * (k & 3)));
  }
}

void copy_header(const ehm_jpeg::Frame& f, ehm_jpeg_header* h) {
  static_assert(EHM_JPEG_MAX_COMPONENTS == ehm_jpeg::kMaxComponents, "header and parser disagree");
  static_assert(std::is_same<decltype(h->quant), decltype(ehm_jpeg::Frame::quant)>::value, "header and parser disagree");
  memset(h, 0, sizeof(*h));
  h->H = f.H, h->W = f.W, h->components = f.components, h->hmax = f.hmax, h->vmax = f.vmax;
  h->mcus_x = f.mcus_x, h->mcus_y = f.mcus_y, h->restart_interval = f.restart_interval;
  for (int c = 0; c < f.components; ++c)
    h->h[c] = f.h[c], h->v[c] = f.v[c], h->blocks_x[c] = f.blocks_x[c], h->blocks_y[c] = f.blocks_y[c], h->quant_id[c] = f.quant_id[c];
  memcpy(h->quant, f.quant, sizeof(h->quant));
  h->coef_count = f.coef_count;
}

}  // namespace

extern "C" int ehm_jpeg_read_header(const uint8_t* data, int64_t n, ehm_jpeg_header* hdr) {
  EHM_CHECK_ARG(data && n >= 0 && hdr);
  char msg[256];
  ehm_jpeg::Frame f;
  const int rc = ehm_jpeg::read_header(data, n, &f, msg, sizeof msg);
  if (rc) {
    ehm_set_error("%s", msg);
    return EHM_EINVAL;
  }
  copy_header(f, hdr);
  return 0;
}

extern "C" int ehm_jpeg_entropy_decode(const uint8_t* data, int64_t n, ehm_jpeg_header* hdr, int16_t* coef, int64_t capacity) {
  EHM_CHECK_ARG(data && n >= 0 && coef && capacity >= 0);
  char msg[256];
  ehm_jpeg::Frame f;
  memset(&f, 0, sizeof f);
  const int rc = ehm_jpeg::entropy_decode(data, n, &f, coef, capacity, msg, sizeof msg);
  if (rc) {
    ehm_set_error("%s", msg);
    return EHM_EINVAL;
  }
  if (hdr) copy_header(f, hdr);
  return 0;
}

extern "C" int ehm_jpeg_workspace_bytes(const ehm_jpeg_decode_desc* d, int64_t* bytes) {
  EHM_CHECK_ARG(d && bytes && d->F > 0 && d->F <= 65535);
  JpegGeo g;
  if (int rc = make_geo(d, &g)) return rc;
  *bytes = (int64_t)d->F * g.blocks * 64;
  return 0;
}

extern "C" int ehm_jpeg_decode(const ehm_jpeg_decode_desc* d, void* stream) {
  EHM_CHECK_ARG(d && d->coef && d->quant && d->frames && d->workspace && d->F > 0 && d->F <= 65535);
  JpegGeo g;
  if (int rc = make_geo(d, &g)) return rc;
  const int64_t total = (int64_t)d->F * g.blocks;
  EHM_CHECK_ARG(d->workspace_bytes >= total * 64);
  EHM_CHECK_ARG(((uintptr_t)d->coef & 15) == 0 && ((uintptr_t)d->quant & 15) == 0 && ((uintptr_t)d->workspace & 15) == 0);
  EHM_CHECK_ARG(ceil_div(total, kBlocksPerGroup) < (1ll << 31));
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)ceil_div(total, kBlocksPerGroup)), dim3(kThreads), 0, (hipStream_t)stream, g, d->coef,
                     d->quant, (uint8_t*)d->workspace, total);
  EHM_LAUNCH_CHECK();
  const int64_t octs = (int64_t)((d->W + 7) / 8) * d->H;
  EHM_CHECK_ARG(octs < (1ll << 31) - kThreads);
  const int wide = d->W % 8 == 0 && ((uintptr_t)d->frames & 7) == 0;
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)ceil_div(octs, kThreads), (unsigned)d->F), dim3(kThreads), 0, (hipStream_t)stream, g,
                     (const uint8_t*)d->workspace, d->frames, wide);
  EHM_LAUNCH_CHECK();
  return 0;
}
