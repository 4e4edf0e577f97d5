// Vector-Jacobian product of the ResNet-50 trunk in eval mode (egohmr_amd/encoders.py ResNet50Features, csrc/conv.hip, csrc/stem.hip) for gfx950
// (MI355X): everything of its backward that is not a data-gradient convolution.  Per conv with folded weight w', folded bias b', input x (the SAVED X2
// activation), output y = relu(conv(x, w') + b' (+ res)) and g = dL/dy:
//   G = s g (.) [y > 0]                                  conv_bwd_gate_kernel  (dense, or zero-dilated for the data gradient of a stride-2 conv;
//                                                                               per-pixel g, or the average pool's per-image g / (H W))
//   b'bar = sum over the pixels of G                     conv_bwd_colsum_kernel + colsum_finish_kernel
//   w'bar[co, kh, kw, ci] = sum_p G[p, co] x[tap(p), ci] conv_bwd_wgrad_kernel (exact-f32 MFMA, k = the pixel, the taps gathered) + conv_wgrad_finish_kernel
//   stem: w'bar [64][147], b'bar [64]                    stem_bwd_preact_kernel / stem_bwd_route_kernel / stem_bwd_wgrad_kernel + stem_bwd_finish_kernel
// The data gradients xbar = conv_transpose(G, w') run on ehm_conv_nhwc_split (egohmr_amd/trunk_grad.py).
// No atomics anywhere: every sum over pixels is split into runs that are a function of the shape alone and added in index order, so two calls on the
// same inputs give the same bits.
#include "common.h"
#include "egohmr_hip.h"
#include "gcn_dev.h"

namespace {

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// sum of n floats `stride` apart in index order (float64); the loads go out 16 at a time
__device__ __forceinline__ double strided_sum(const float* __restrict__ p, size_t stride, int n) {
  double s = 0.0;
  int k = 0;
  for (; k + 16 <= n; k += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = p[(size_t)(k + u) * stride];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += (double)v[u];
  }
  for (; k < n; ++k) s += (double)p[(size_t)k * stride];
  return s;
}

// ------------------------------------------------------------------------------------------------------------------------------ gate
struct GateArgs {
  const float* g; const half_t* y; const float* scale; float* out;
  int Ho, Wo, C, H, W, dil, per_image;
  float hw;
  long long total8;
};

// one thread = 8 consecutive channels of one OUTPUT pixel (h, w) of [N, H, W, C]: 16-byte loads of the hi and the lo halves of y and of g, two 16-byte stores
__global__ __launch_bounds__(256) void conv_bwd_gate_kernel(GateArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.total8) return;
  const int c8 = a.C / 8;
  const int c = 8 * (int)(t % c8);
  long long pix = t / c8;
  const int w = (int)(pix % a.W);
  pix /= a.W;
  const int h = (int)(pix % a.H);
  const long long n = pix / a.H;
  int ho = h, wo = w;
  bool live = true;
  if (a.dil == 2) {
    ho = h >> 1;
    wo = w >> 1;
    live = !(h & 1) && !(w & 1) && ho < a.Ho && wo < a.Wo;
  }
  f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const size_t row = ((size_t)n * a.Ho + ho) * a.Wo + wo;
    const half_t* p = a.y + split_off<32>(row, c, a.C);
    const half8 hi = *(const half8*)p, lo = *(const half8*)(p + 32);
    const float* gp = a.per_image ? a.g + (size_t)n * a.C + c : a.g + row * (size_t)a.C + c;
    const f32x4 g0 = *(const f32x4*)gp, g1 = *(const f32x4*)(gp + 4);
    const float s = a.scale ? *a.scale : 1.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float ga = a.per_image ? g0[q] / a.hw : g0[q], gb = a.per_image ? g1[q] / a.hw : g1[q];
      v0[q] = (float)hi[q] + (float)lo[q] > 0.f ? ga * s : 0.f;                 // (a NaN behind a closed gate does not pass)
      v1[q] = (float)hi[4 + q] + (float)lo[4 + q] > 0.f ? gb * s : 0.f;
    }
  }
  float* o = a.out + (size_t)(t / c8) * a.C + c;
  *(f32x4*)o = v0;
  *(f32x4*)(o + 4) = v1;
}

// ------------------------------------------------------------------------------------------------------------------------------ column sums
// G [P, C] -> part[chunk][C]: a block owns `rows` pixels x 128 columns (32 lanes x 16 bytes across, 8 row lanes down); a lane adds its rows in row order,
// the 8 row lanes are added in index order through LDS, the chunks in index order by colsum_finish_kernel
__global__ __launch_bounds__(256) void conv_bwd_colsum_kernel(const float* __restrict__ G, float* __restrict__ part, long long P, int C, int rows) {
  __shared__ __attribute__((aligned(16))) float red[8][128];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c = blockIdx.y * 128 + 4 * cl;
  const long long p0 = (long long)blockIdx.x * rows;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (c < C)
    for (int r = rl; r < rows && p0 + r < P; r += 8) acc += *(const f32x4*)(G + (size_t)(p0 + r) * C + c);
  *(f32x4*)&red[rl][4 * cl] = acc;
  __syncthreads();
  if (threadIdx.x < 128 && blockIdx.y * 128 + (int)threadIdx.x < C) {
    float s = red[0][threadIdx.x];
#pragma unroll
    for (int r = 1; r < 8; ++r) s += red[r][threadIdx.x];
    part[(size_t)blockIdx.x * C + blockIdx.y * 128 + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(256) void colsum_finish_kernel(const float* __restrict__ part, float* __restrict__ out, int C, int chunks) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= C) return;
  out[t] = (float)strided_sum(part + t, (size_t)C, chunks);
}

// ------------------------------------------------------------------------------------------------------------------------------ weight gradient
// out[co, tap, ci] = sum over the output pixels p of G[p, co] x[tap(p), ci]: the contraction over the pixels, straight from the row-major operands.
// v_mfma_f32_32x32x2_f32 takes A[i][k] from lane (i = l & 31, k = l >> 5) and B[k][j] from lane (j = l & 31, k = l >> 5): with k = the pixel, both fragments
// are 128-byte runs of a row of G and of x (csrc/pointnet_bwd.hip pointnet_wgrad_kernel has the form).  Here the x row is the tap's pixel of the saved X2
// activation (an implicit GEMM: no im2col); a tap outside the image is a zero, never a load.  A block owns a 128 x 128 tile of one tap's [Co, Ci] for one
// run of pixels (split-K); its 4 waves own 64 x 64 each = 2 x 2 accumulators, 16 pixels of loads in flight.  Co and Ci are multiples of 64: a wave whose
// 64 x 64 quarter lies past an edge does nothing.
struct CwArgs {
  const float* G; const half_t* X; float* part;
  int H, W, Ci, Ho, Wo, Co, KW, stride, pad, cit;
  long long P;
  int run;
};

__global__ __launch_bounds__(256) void conv_bwd_wgrad_kernel(CwArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
  const int tap = blockIdx.z / p.cit, ct = blockIdx.z - tap * p.cit;
  const int kh = tap / p.KW, kw = tap - kh * p.KW;
  const int gbase = blockIdx.y * 128 + 64 * (wave >> 1), abase = ct * 128 + 64 * (wave & 1);
  if (gbase >= p.Co || abase >= p.Ci) return;                                      // (wave-uniform; no barrier in this kernel)
  const int g0 = gbase + l31, a0 = abase + l31;
  f32x16 acc[2][2];
#pragma unroll
  for (int gb = 0; gb < 2; ++gb)
#pragma unroll
    for (int ab = 0; ab < 2; ++ab)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[gb][ab][r] = 0.f;
  const long long p_begin = (long long)blockIdx.x * p.run;
  const long long p_end = p_begin + p.run < p.P ? p_begin + p.run : p.P;
  const int hw = p.Ho * p.Wo;
  for (long long mm = p_begin; mm < p_end; mm += 16) {
    float pg[8][2], qa[8][2];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long long pix = mm + 2 * u + h;
      const bool ok = pix < p_end;
      const long long n = pix / hw;
      const int rem = (int)(pix - n * hw);
      const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
      const int hi = ho * p.stride - p.pad + kh, wi = wo * p.stride - p.pad + kw;
      const bool in = ok && hi >= 0 && hi < p.H && wi >= 0 && wi < p.W;
      const size_t row = ((size_t)n * p.H + hi) * p.W + wi;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        pg[u][e] = 0.f;
        qa[u][e] = 0.f;
        if (ok) pg[u][e] = p.G[(size_t)pix * p.Co + g0 + 32 * e];
        if (in) qa[u][e] = split_load<32>(p.X, row, a0 + 32 * e, p.Ci);
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int gb = 0; gb < 2; ++gb)
#pragma unroll
        for (int ab = 0; ab < 2; ++ab) acc[gb][ab] = __builtin_amdgcn_mfma_f32_32x32x2f32(pg[u][gb], qa[u][ab], acc[gb][ab], 0, 0, 0);
  }
  // accumulator layout: column = l & 31, row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)
  const size_t K = (size_t)gridDim.z / p.cit * p.Ci;
  float* o = p.part + (size_t)blockIdx.x * p.Co * K + (size_t)tap * p.Ci;
#pragma unroll
  for (int gb = 0; gb < 2; ++gb)
#pragma unroll
    for (int ab = 0; ab < 2; ++ab)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int g = gbase + 32 * gb + (r & 3) + 8 * (r >> 2) + 4 * h;
        o[(size_t)g * K + a0 + 32 * ab] = acc[gb][ab][r];
      }
}

// part [nsplit][total] -> out [total]: the runs in index order
__global__ __launch_bounds__(256) void conv_wgrad_finish_kernel(const float* __restrict__ part, float* __restrict__ out, long long total, int nsplit) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  out[t] = (float)strided_sum(part + t, (size_t)total, nsplit);
}

struct CwPlan { long long P; int Ho, Wo, taps, cit, cot, run, nsplit, crows, chunks; };

// split-K plan: runs of whole 16-pixel groups, at most 256 of them, enough for about a thousand blocks; a function of the shape alone
int cw_plan(int N, int H, int W, int Ci, int Co, int K, int stride, int pad, CwPlan* pl) {
  EHM_CHECK_ARG(N > 0 && H > 0 && W > 0 && Ci > 0 && Co > 0 && Ci % 64 == 0 && Co % 64 == 0 && (K == 1 || K == 3) && (stride == 1 || stride == 2));
  EHM_CHECK_ARG(pad >= 0 && pad < 16 && H + 2 * pad >= K && W + 2 * pad >= K);
  pl->Ho = (H + 2 * pad - K) / stride + 1;
  pl->Wo = (W + 2 * pad - K) / stride + 1;
  pl->P = (long long)N * pl->Ho * pl->Wo;
  EHM_CHECK_ARG(pl->P * Co < (1ll << 40) && (long long)N * H * W * Ci < (1ll << 40) && pl->P < (1ll << 31));
  pl->taps = K * K;
  pl->cit = (int)ceil_div(Ci, 128);
  pl->cot = (int)ceil_div(Co, 128);
  const long long tiles = (long long)pl->taps * pl->cit * pl->cot;
  long long want = ceil_div(1024, tiles), byrun = ceil_div(pl->P, 64);
  want = want < byrun ? want : byrun;
  want = want > 256 ? 256 : (want < 1 ? 1 : want);
  pl->run = (int)round_up(ceil_div(pl->P, want), 16);
  pl->nsplit = (int)ceil_div(pl->P, pl->run);
  pl->crows = (int)round_up(ceil_div(pl->P, 256), 64);
  pl->chunks = (int)ceil_div(pl->P, pl->crows);
  EHM_CHECK_ARG(pl->taps * pl->cit < 65536 && pl->cot < 65536);
  return 0;
}

int64_t cw_ws_floats(const CwPlan& pl, int Ci, int Co) { return (int64_t)pl.nsplit * Co * pl.taps * Ci + (int64_t)pl.chunks * Co; }

// ------------------------------------------------------------------------------------------------------------------------------ stem
constexpr int SB_K = 148;          // 147 weights (k = (ci * 7 + kh) * 7 + kw) + the bias
constexpr int SB_KG = 37;          // k's per wave of stem_bwd_wgrad_kernel (4 waves)
constexpr int SB_BLOCKS = 256;     // its grid: fixed, so the partial sums' order is a function of the shape alone

// z[n, r, c, ch] = conv 7x7 / 2 / pad 3 of the image + bias in float32 on the vector ALU: one wave = one conv pixel, lane = channel; the image values
// are wave-uniform
__global__ __launch_bounds__(256) void stem_bwd_preact_kernel(const float* __restrict__ img, const float* __restrict__ Wt, const float* __restrict__ bias,
                                                               float* __restrict__ z, int H, int W, long long pixels) {
  const int ch = threadIdx.x & 63;
  const long long pix = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (pix >= pixels) return;
  const int Hc = H / 2, Wc = W / 2;
  const int c = (int)(pix % Wc), r = (int)((pix / Wc) % Hc);
  const long long n = pix / ((long long)Wc * Hc);
  float acc = 0.f;
  for (int ci = 0; ci < 3; ++ci)
    for (int kh = 0; kh < 7; ++kh) {
      const int ir = 2 * r + kh - 3;
      if (ir < 0 || ir >= H) continue;
      const float* src = img + ((size_t)(n * 3 + ci) * H + ir) * W;
#pragma unroll
      for (int kw = 0; kw < 7; ++kw) {
        const int ic = 2 * c + kw - 3;
        if (ic >= 0 && ic < W) acc = fmaf(src[ic], Wt[((ci * 7 + kh) * 7 + kw) * 64 + ch], acc);
      }
    }
  z[(size_t)pix * 64 + ch] = acc + bias[ch];
}

// is (v, i) a better maximum than (bv, bi)?  NaN beats every number (torch's max-pool propagates it); among equals the lower index wins
__device__ __forceinline__ bool pool_better(float v, float bv) {
  if (v != v) return bv == bv;
  if (bv != bv) return false;
  return v > bv;
}

// gz[n, r, c, ch] = sum over the (at most four) 3x3 / stride-2 / pad-1 windows that cover (r, c) and whose arg-max (lowest row-major index among equals) it
// is, of that window's cotangent.  A gather: every pre-pool pixel is written once; the windows in (row, column) order
__global__ __launch_bounds__(256) void stem_bwd_route_kernel(const float* __restrict__ z, const float* __restrict__ gpool, float* __restrict__ gz, int Hc,
                                                              int Wc, long long pixels) {
  const int ch = threadIdx.x & 63;
  const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pix >= pixels) return;
  const int Hq = Hc / 2, Wq = Wc / 2;
  const int c = (int)(pix % Wc), r = (int)((pix / Wc) % Hc);
  const long long n = pix / ((long long)Wc * Hc);
  const float* zn = z + (size_t)n * Hc * Wc * 64 + ch;
  float acc = 0.f;
  for (int pr = r >> 1; pr <= ((r + 1) >> 1) && pr < Hq; ++pr)
    for (int pc = c >> 1; pc <= ((c + 1) >> 1) && pc < Wq; ++pc) {
      float bv = 0.f;
      int br = -1, bc = -1;
      for (int dr = -1; dr <= 1; ++dr) {
        const int rr = 2 * pr + dr;
        if (rr < 0 || rr >= Hc) continue;
        for (int dc = -1; dc <= 1; ++dc) {
          const int cc = 2 * pc + dc;
          if (cc < 0 || cc >= Wc) continue;
          const float v = zn[((size_t)rr * Wc + cc) * 64];
          if (br < 0 || pool_better(v, bv)) { bv = v; br = rr; bc = cc; }
        }
      }
      if (br == r && bc == c) acc += gpool[(((size_t)n * Hq + pr) * Wq + pc) * 64 + ch];
    }
  gz[(size_t)pix * 64 + ch] = acc;
}

// part[block][k][ch] (+)= sum over the block's conv rows (block, block + 256, ...) and their pixels in order of gz[n, r, c, ch] * tap k of the image
// (k = 147: 1, the bias).  thread = (channel, one of 4 groups of 37 k's); the image values are wave-uniform
__global__ __launch_bounds__(256) void stem_bwd_wgrad_kernel(const float* __restrict__ img, const float* __restrict__ gz, float* __restrict__ part, int H, int W,
                                                              int rows, int accumulate) {
  const int ch = threadIdx.x & 63;
  const int kg = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int Hc = H / 2, Wc = W / 2;
  float acc[SB_KG];
#pragma unroll
  for (int j = 0; j < SB_KG; ++j) acc[j] = 0.f;
  for (int rr = blockIdx.x; rr < rows; rr += SB_BLOCKS) {
    const int n = rr / Hc, r = rr - n * Hc;
    const float* gp = gz + (size_t)rr * Wc * 64 + ch;
    const float* im = img + (size_t)n * 3 * H * W;
    for (int c = 0; c < Wc; ++c) {
      const float g = gp[(size_t)c * 64];
#pragma unroll
      for (int j = 0; j < SB_KG; ++j) {
        const int k = kg * SB_KG + j;
        float v = 1.f;
        if (k < 147) {
          const int ci = k / 49, kh = (k - 49 * ci) / 7, kw = k - 49 * ci - 7 * kh;
          const int ir = 2 * r + kh - 3, ic = 2 * c + kw - 3;
          v = (ir >= 0 && ir < H && ic >= 0 && ic < W) ? im[((size_t)ci * H + ir) * W + ic] : 0.f;
        }
        acc[j] = fmaf(g, v, acc[j]);
      }
    }
  }
  float* o = part + (size_t)blockIdx.x * SB_K * 64;
#pragma unroll
  for (int j = 0; j < SB_KG; ++j) {
    const int k = kg * SB_KG + j;
    o[k * 64 + ch] = accumulate ? o[k * 64 + ch] + acc[j] : acc[j];
  }
}

__global__ __launch_bounds__(256) void stem_bwd_finish_kernel(const float* __restrict__ part, float* __restrict__ gW, float* __restrict__ gb) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= SB_K * 64) return;
  const int k = t / 64, ch = t - 64 * k;
  const float s = (float)strided_sum(part + t, (size_t)SB_K * 64, SB_BLOCKS);
  if (k < 147) { if (gW) gW[ch * 147 + k] = s; }
  else if (gb) gb[ch] = s;
}

struct StemPlan { int chunk; int64_t zfloats; };

int stem_plan(int N, int H, int W, StemPlan* pl) {
  EHM_CHECK_ARG(N > 0 && H > 0 && W > 0 && H % 32 == 0 && W % 32 == 0 && (long long)N * H * W < (1ll << 31));
  const int64_t per_image = (int64_t)(H / 2) * (W / 2) * 64;
  int64_t chunk = ((int64_t)8 << 20) / per_image;                  // 32 MiB of pre-pool activations (and as much of their cotangent) at a time
  chunk = chunk < 1 ? 1 : (chunk > N ? N : chunk);
  pl->chunk = (int)chunk;
  pl->zfloats = chunk * per_image;
  return 0;
}

}  // namespace

extern "C" int ehm_conv_bwd_gate(const float* g, int g_per_image, const void* y_x2, const float* scale, float* out, int N, int Ho, int Wo, int C, int H,
                                 int W, void* stream) {
  EHM_CHECK_ARG(g && y_x2 && out && al16(g) && al16(y_x2) && al16(out) && (g_per_image == 0 || g_per_image == 1));
  EHM_CHECK_ARG(N > 0 && Ho > 0 && Wo > 0 && H > 0 && W > 0 && C > 0 && C % 32 == 0);
  const bool dense = H == Ho && W == Wo;
  EHM_CHECK_ARG(dense || ((H - 1) / 2 + 1 == Ho && (W - 1) / 2 + 1 == Wo));
  EHM_CHECK_ARG((long long)N * H * W * C < (1ll << 40) && (const void*)g != (const void*)out);
  GateArgs a;
  a.g = g; a.y = (const half_t*)y_x2; a.scale = scale; a.out = out;
  a.Ho = Ho; a.Wo = Wo; a.C = C; a.H = H; a.W = W; a.dil = dense ? 1 : 2; a.per_image = g_per_image;
  a.hw = (float)(Ho * Wo);
  a.total8 = (long long)N * H * W * (C / 8);
  const long long blocks = ceil_div(a.total8, 256);
  EHM_CHECK_ARG(blocks < (1ll << 31));
  hipLaunchKernelGGL(conv_bwd_gate_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_conv_bwd_wgrad_workspace_bytes(int N, int H, int W, int Ci, int Co, int K, int stride, int pad, int64_t* bytes) {
  EHM_CHECK_ARG(bytes != nullptr);
  CwPlan pl;
  const int rc = cw_plan(N, H, W, Ci, Co, K, stride, pad, &pl);
  if (rc != 0) return rc;
  *bytes = cw_ws_floats(pl, Ci, Co) * (int64_t)sizeof(float);
  return 0;
}

extern "C" int ehm_conv_bwd_wgrad(const float* G, const void* x_x2, int64_t x_rows, float* gw, float* gbias, int N, int H, int W, int Ci, int Co, int K,
                                  int stride, int pad, void* workspace, int64_t workspace_bytes, void* stream) {
  CwPlan pl;
  const int rc = cw_plan(N, H, W, Ci, Co, K, stride, pad, &pl);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(G && (gw || gbias) && al16(G) && (!gw || (x_x2 && al16(x_x2) && x_rows >= (int64_t)N * H * W)));
  EHM_CHECK_ARG(workspace && al16(workspace) && workspace_bytes >= cw_ws_floats(pl, Ci, Co) * (int64_t)sizeof(float));
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  if (gw) {
    CwArgs a;
    a.G = G; a.X = (const half_t*)x_x2; a.part = part;
    a.H = H; a.W = W; a.Ci = Ci; a.Ho = pl.Ho; a.Wo = pl.Wo; a.Co = Co; a.KW = K; a.stride = stride; a.pad = pad; a.cit = pl.cit;
    a.P = pl.P; a.run = pl.run;
    hipLaunchKernelGGL(conv_bwd_wgrad_kernel, dim3((unsigned)pl.nsplit, (unsigned)pl.cot, (unsigned)(pl.taps * pl.cit)), dim3(256), 0, st, a);
    const long long total = (long long)Co * pl.taps * Ci;
    hipLaunchKernelGGL(conv_wgrad_finish_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, st, part, gw, total, pl.nsplit);
  }
  if (gbias) {
    float* cpart = part + (size_t)pl.nsplit * Co * pl.taps * Ci;
    hipLaunchKernelGGL(conv_bwd_colsum_kernel, dim3((unsigned)pl.chunks, (unsigned)pl.cot), dim3(256), 0, st, G, cpart, pl.P, Co, pl.crows);
    hipLaunchKernelGGL(colsum_finish_kernel, dim3((unsigned)ceil_div(Co, 256)), dim3(256), 0, st, cpart, gbias, Co, pl.chunks);
  }
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_resnet_stem_backward_workspace_bytes(int N, int H, int W, int64_t* bytes) {
  EHM_CHECK_ARG(bytes != nullptr);
  StemPlan pl;
  const int rc = stem_plan(N, H, W, &pl);
  if (rc != 0) return rc;
  *bytes = (2 * pl.zfloats + (int64_t)SB_BLOCKS * SB_K * 64) * (int64_t)sizeof(float);
  return 0;
}

extern "C" int ehm_resnet_stem_backward(const float* img, const float* Wt, const float* bias, const float* gpool, float* gW, float* gb, float* z_out,
                                        float* gz_out, int N, int H, int W, void* workspace, int64_t workspace_bytes, void* stream) {
  StemPlan pl;
  const int rc = stem_plan(N, H, W, &pl);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(img && Wt && bias && gpool && (gW || gb));
  EHM_CHECK_ARG(workspace && al16(workspace) && workspace_bytes >= (2 * pl.zfloats + (int64_t)SB_BLOCKS * SB_K * 64) * (int64_t)sizeof(float));
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  float* part = ws + 2 * pl.zfloats;
  const int Hc = H / 2, Wc = W / 2, Hq = H / 4, Wq = W / 4;
  const size_t per_image = (size_t)Hc * Wc * 64;
  for (int n0 = 0; n0 < N; n0 += pl.chunk) {
    const int nimg = N - n0 < pl.chunk ? N - n0 : pl.chunk;
    float* z = z_out ? z_out + n0 * per_image : ws;
    float* gz = gz_out ? gz_out + n0 * per_image : ws + pl.zfloats;
    const float* im = img + (size_t)n0 * 3 * H * W;
    const long long pixels = (long long)nimg * Hc * Wc;
    const unsigned blocks = (unsigned)ceil_div(pixels, 4);
    hipLaunchKernelGGL(stem_bwd_preact_kernel, dim3(blocks), dim3(256), 0, st, im, Wt, bias, z, H, W, pixels);
    hipLaunchKernelGGL(stem_bwd_route_kernel, dim3(blocks), dim3(256), 0, st, (const float*)z, gpool + (size_t)n0 * Hq * Wq * 64, gz, Hc, Wc, pixels);
    hipLaunchKernelGGL(stem_bwd_wgrad_kernel, dim3(SB_BLOCKS), dim3(256), 0, st, im, (const float*)gz, part, H, W, nimg * Hc, n0 > 0 ? 1 : 0);
  }
  hipLaunchKernelGGL(stem_bwd_finish_kernel, dim3((unsigned)ceil_div(SB_K * 64, 256)), dim3(256), 0, st, (const float*)part, gW, gb);
  EHM_LAUNCH_CHECK();
  return 0;
}

// The stem backward's three steps on their own, for the train-mode BatchNorm route (csrc/bn2d_train.hip, egohmr_amd/trunk_grad.py), which needs the batch
// sums over ALL pre-pool pixels between them: whole-batch tensors, no chunks.
extern "C" int ehm_resnet_stem_preact(const float* img, const float* Wt, const float* bias, float* z, int N, int H, int W, void* stream) {
  StemPlan pl;
  const int rc = stem_plan(N, H, W, &pl);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(img && Wt && bias && z);
  const long long pixels = (long long)N * (H / 2) * (W / 2);
  hipLaunchKernelGGL(stem_bwd_preact_kernel, dim3((unsigned)ceil_div(pixels, 4)), dim3(256), 0, (hipStream_t)stream, img, Wt, bias, z, H, W, pixels);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_resnet_stem_route(const float* z, const float* gpool, float* gz, int N, int H, int W, void* stream) {
  StemPlan pl;
  const int rc = stem_plan(N, H, W, &pl);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(z && gpool && gz && (const void*)z != (const void*)gz);
  const long long pixels = (long long)N * (H / 2) * (W / 2);
  hipLaunchKernelGGL(stem_bwd_route_kernel, dim3((unsigned)ceil_div(pixels, 4)), dim3(256), 0, (hipStream_t)stream, z, gpool, gz, H / 2, W / 2, pixels);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_resnet_stem_wgrad(const float* img, const float* gz, float* gW, float* gb, int N, int H, int W, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
  StemPlan pl;
  const int rc = stem_plan(N, H, W, &pl);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(img && gz && (gW || gb));
  EHM_CHECK_ARG(workspace && al16(workspace) && workspace_bytes >= (int64_t)SB_BLOCKS * SB_K * 64 * (int64_t)sizeof(float));
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  hipLaunchKernelGGL(stem_bwd_wgrad_kernel, dim3(SB_BLOCKS), dim3(256), 0, st, img, gz, part, H, W, N * (H / 2), 0);
  hipLaunchKernelGGL(stem_bwd_finish_kernel, dim3((unsigned)ceil_div(SB_K * 64, 256)), dim3(256), 0, st, (const float*)part, gW, gb);
  EHM_LAUNCH_CHECK();
  return 0;
}
