// Train-mode BatchNorm2d of the ResNet-50 trunk (egohmr_amd/encoders.py ResNet50Features.train_batchnorm, egohmr_amd/trunk_grad.py) for gfx950 (MI355X):
// what batch statistics add to the folded trunk and to its backward (csrc/conv_bwd.hip), in the pattern of csrc/gcn_train.hip.  z [pixels, C] is a
// conv's RAW output (no BatchNorm, no bias), either the X2 buffer ehm_conv_x2 wrote (only its first `pixels` rows count: the tile padding and the
// trailing zero row are never read) or float32 rows (the stem's pre-pool activation).
//   forward:   mu = mean_p z,  var = mean_p (z - mu)^2 (biased),  invstd = 1 / sqrt(var + eps)          bn2d_sum_kernel x 2 + bn2d_stats_finish_kernel
//              running_mean / running_var (unbiased) / num_batches_tracked as nn.BatchNorm2d updates them, in the same launch sequence.
//              Two passes (the mean first, then the centred squares), float64 accumulators: correct to float32 rounding at |mu| / sigma = 1e3.
//   backward:  with G = g (.) [y > 0] (ehm_conv_bwd_gate) and xhat = (z - mu) invstd:
//              betabar = sum_p G,  gammabar = sum_p G xhat                                                  bn2d_sum_kernel + bn2d_bwd_reduce_kernel
//              zbar = *scale gamma invstd (G - betabar / R - xhat gammabar / R)                             bn2d_zbar_kernel (dense, or zero-dilated)
// Data parallel (the *_local / *_merge entries at the end): each rank stops at [2][C] float64, the caller all-gathers, every rank merges in rank order.
// A pair is the one-call entry's own body cut at the collective: bn2d_moments / bn2d_bwd_partials issue the passes for both, and the one finish kernel
// and the one reduce kernel write out for both, from the call's own partial sums or from the gathered buffer (BnMoments, common.h).
// No atomics: a block owns a run of pixels that is a function of the shape alone, a lane adds its rows in row order, the row lanes and then the runs
// are added in index order - two calls on the same inputs give the same bits.
#include "common.h"
#include "egohmr_hip.h"
#include "gcn_dev.h"

namespace {

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

constexpr int BN_ROWL = 16;        // row lanes of a bn2d_sum_kernel block (x 16 column lanes of 8 channels = 128 columns)
constexpr int BN_MAX_RUNS = 256;

// 8 consecutive channels (c % 8 == 0) of row `row`: X2 (32 hi halves | 32 lo halves per 32 channels, value = hi + lo) or float32
template <bool X2IN>
__device__ __forceinline__ void load8(const void* __restrict__ z, size_t row, int c, int C, float (&v)[8]) {
  if (X2IN) {
    const half_t* p = (const half_t*)z + split_off<32>(row, c, C);
    const half8 hi = *(const half8*)p, lo = *(const half8*)(p + 32);
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = (float)hi[q] + (float)lo[q];
  } else {
    const float* p = (const float*)z + row * (size_t)C + c;
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) { v[q] = a[q]; v[4 + q] = b[q]; }
  }
}

// MODE 0: part[run][0][c] = sum z                       (A unused)
// MODE 1: part[run][0][c] = sum (z - mean_d)^2          (mean_d: float64 [C])
// MODE 2: part[run][0][c] = sum G, part[run][1][c] = sum G (z - mean) invstd      (mean, invstd float32 [C]; G float32 [P, C])
// grid (runs, ceil(C / 128)); thread = 8 channels x one of 16 row lanes
template <bool X2IN, int MODE>
__global__ __launch_bounds__(256) void bn2d_sum_kernel(const void* __restrict__ z, const float* __restrict__ G, const double* __restrict__ mean_d,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd, double* __restrict__ part,
                                                       long long P, int C, int run) {
  constexpr int NS = MODE == 2 ? 2 : 1;
  __shared__ double red[BN_ROWL][NS][128];
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = blockIdx.y * 128 + 8 * cl;
  const long long p0 = (long long)blockIdx.x * run;
  double acc[NS][8];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[s][q] = 0.0;
  if (c < C) {
    double m[8];
    float is[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      m[q] = MODE == 1 ? mean_d[c + q] : (MODE == 2 ? (double)mean[c + q] : 0.0);
      is[q] = MODE == 2 ? invstd[c + q] : 0.f;
    }
    for (long long r = p0 + rl; r < p0 + run && r < P; r += BN_ROWL) {
      float v[8];
      load8<X2IN>(z, (size_t)r, c, C, v);
      if (MODE == 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[0][q] += (double)v[q];
      } else if (MODE == 1) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const double d = (double)v[q] - m[q];
          acc[0][q] += d * d;
        }
      } else {
        const float* gp = G + (size_t)r * C + c;
        const f32x4 g0 = *(const f32x4*)gp, g1 = *(const f32x4*)(gp + 4);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const double g = (double)(q < 4 ? g0[q & 3] : g1[q & 3]);
          acc[0][q] += g;
          acc[1][q] += g * (((double)v[q] - m[q]) * (double)is[q]);
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int q = 0; q < 8; ++q) red[rl][s][8 * cl + q] = acc[s][q];
  __syncthreads();
  for (int t = threadIdx.x; t < NS * 128; t += 256) {
    const int s = t / 128, j = t - 128 * s;
    if (blockIdx.y * 128 + j >= C) continue;
    double sum = red[0][s][j];
#pragma unroll
    for (int r = 1; r < BN_ROWL; ++r) sum += red[r][s][j];
    part[((size_t)blockIdx.x * NS + s) * C + blockIdx.y * 128 + j] = sum;
  }
}

__global__ __launch_bounds__(256) void bn2d_mean_finish_kernel(const double* __restrict__ part, double* __restrict__ mean_d, int C, int runs, double R) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= C) return;
  mean_d[t] = ordered_sum(part + t, (size_t)C, runs) / R;
}

// (mean, M2 = sum of squares centred on that mean) of this call's own rows or of every rank's (BnMoments, common.h) -> local[0][c] = mean, local[1][c] = M2
// and nothing else (a rank's share), or what nn.BatchNorm2d keeps of the batch: mean, var, invstd (float32), the running statistics and its call count
__global__ __launch_bounds__(256) void bn2d_stats_finish_kernel(BnMoments src, double* __restrict__ local, float* __restrict__ mean, float* __restrict__ var,
                                                                float* __restrict__ invstd, float* __restrict__ running_mean,
                                                                float* __restrict__ running_var, long long* __restrict__ tracked, int C, double eps,
                                                                double momentum) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t == 0 && tracked) *tracked += 1;
  if (t >= C) return;
  double mu, M2;
  moments_of(src, t, C, &mu, &M2);
  if (local) {
    local[t] = mu;
    local[C + t] = M2;
    return;
  }
  const double R = src.rr.total, v = M2 / R;
  mean[t] = (float)mu;
  var[t] = (float)v;
  invstd[t] = (float)(1.0 / sqrt(v + eps));
  if (running_mean) running_mean[t] = (float)((1.0 - momentum) * (double)running_mean[t] + momentum * mu);
  if (running_var) running_var[t] = (float)((1.0 - momentum) * (double)running_var[t] + momentum * (v * R / (R - 1.0)));
}

// A channel's `count` pairs (sum G, sum G xhat) p[k][2][C], added in index order: a call's runs, or every rank's sums.  With `local`: that pair [2][C] in
// float64 and nothing else (a rank's share).  Without: gbeta / ggamma in float32 (zbar multiplies by 1 / R), and where asked for float32 of pair `own`
// alone - a rank's OWN parameter gradients, which the caller's gradient all-reduce completes (the batch's sums there would count `world` times).
__global__ __launch_bounds__(256) void bn2d_bwd_reduce_kernel(const double* __restrict__ p, int count, int own, int C, double* __restrict__ local,
                                                              float* __restrict__ gbeta, float* __restrict__ ggamma, float* __restrict__ gbeta_own,
                                                              float* __restrict__ ggamma_own) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= C) return;
  const double sb = ordered_sum(p + t, (size_t)2 * C, count), sg = ordered_sum(p + C + t, (size_t)2 * C, count);
  if (local) {
    local[t] = sb;
    local[C + t] = sg;
    return;
  }
  gbeta[t] = (float)sb;
  ggamma[t] = (float)sg;
  if (gbeta_own) gbeta_own[t] = (float)p[(size_t)own * 2 * C + t];
  if (ggamma_own) ggamma_own[t] = (float)p[(size_t)own * 2 * C + C + t];
}

struct ZbarArgs {
  const float* G; const void* z; const float *mean, *invstd, *gamma, *gbeta, *ggamma, *scale;
  float* out;
  int Ho, Wo, C, H, W, dil;
  float invR;
  long long total8;
};

// one thread = 8 consecutive channels of one OUTPUT pixel (h, w) of [N, H, W, C] (the form of conv_bwd_gate_kernel): one pass over G and z, 16-byte accesses
template <bool X2IN>
__global__ __launch_bounds__(256) void bn2d_zbar_kernel(ZbarArgs a) {
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
    float zv[8];
    load8<X2IN>(a.z, row, c, a.C, zv);
    const float* gp = a.G + row * (size_t)a.C + c;
    const f32x4 g0 = *(const f32x4*)gp, g1 = *(const f32x4*)(gp + 4);
    const float s = a.scale ? *a.scale : 1.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float is = a.invstd[c + q];
      const float xh = (zv[q] - a.mean[c + q]) * is;
      const float g = q < 4 ? g0[q & 3] : g1[q & 3];
      const float r = s * (a.gamma[c + q] * is) * (g - a.gbeta[c + q] * a.invR - xh * (a.ggamma[c + q] * a.invR));
      if (q < 4) v0[q & 3] = r; else v1[q & 3] = r;
    }
  }
  float* o = a.out + (size_t)(t / c8) * a.C + c;
  *(f32x4*)o = v0;
  *(f32x4*)(o + 4) = v1;
}

struct BnPlan { int run, runs, cblocks; };

// runs of whole 16-row groups, at most BN_MAX_RUNS of them: a function of the shape alone
// (a rank's share of a data-parallel batch may be ONE row - min_pixels = 1 -, and float32 rows need whole 8-channel lanes only - cmult = 8)
int bn_plan(int64_t pixels, int64_t z_rows, int C, BnPlan* pl, int64_t min_pixels = 2, int cmult = 32) {
  EHM_CHECK_ARG(pixels >= min_pixels && pixels < (1ll << 31) && z_rows >= pixels && C > 0 && C % cmult == 0 && pixels * C < (1ll << 40));
  pl->run = (int)round_up(ceil_div(pixels, BN_MAX_RUNS), BN_ROWL);
  pl->runs = (int)ceil_div(pixels, pl->run);
  pl->cblocks = (int)ceil_div(C, 128);
  return 0;
}

int64_t bn_ws_doubles(const BnPlan& pl, int C) { return (int64_t)pl.runs * 2 * C + C; }

template <int MODE>
void launch_sum(bool x2, const BnPlan& pl, hipStream_t st, const void* z, const float* G, const double* mean_d, const float* mean, const float* invstd,
                double* part, long long P, int C) {
  const dim3 grid((unsigned)pl.runs, (unsigned)pl.cblocks);
  if (x2) hipLaunchKernelGGL((bn2d_sum_kernel<true, MODE>), grid, dim3(256), 0, st, z, G, mean_d, mean, invstd, part, P, C, pl.run);
  else hipLaunchKernelGGL((bn2d_sum_kernel<false, MODE>), grid, dim3(256), 0, st, z, G, mean_d, mean, invstd, part, P, C, pl.run);
}

bool workspace_ok(const void* workspace, int64_t workspace_bytes, const BnPlan& pl, int C) {
  return workspace && al16(workspace) && workspace_bytes >= bn_ws_doubles(pl, C) * (int64_t)sizeof(double);
}

// The launches every statistics entry starts with, and their checks: z -> its mean (float64) and the runs' sums of (z - mean)^2, both in the workspace
int bn2d_moments(const void* z, int z_is_x2, const BnPlan& pl, int64_t pixels, int C, void* workspace, int64_t workspace_bytes, hipStream_t st,
                 BnMoments* own) {
  EHM_CHECK_ARG(z && al16(z) && (z_is_x2 == 0 || z_is_x2 == 1) && workspace_ok(workspace, workspace_bytes, pl, C));
  double* part = (double*)workspace;
  double* mean_d = part + (size_t)pl.runs * 2 * C;
  launch_sum<0>(z_is_x2 != 0, pl, st, z, nullptr, nullptr, nullptr, nullptr, part, pixels, C);
  hipLaunchKernelGGL(bn2d_mean_finish_kernel, dim3((unsigned)ceil_div(C, 256)), dim3(256), 0, st, (const double*)part, mean_d, C, pl.runs, (double)pixels);
  launch_sum<1>(z_is_x2 != 0, pl, st, z, nullptr, (const double*)mean_d, nullptr, nullptr, part, pixels, C);
  *own = own_moments(part, mean_d, pl.runs, (double)pixels);
  return 0;
}

// The launch every backward over a rank's own rows starts with, and its checks: the runs' (sum G, sum G xhat) [runs][2][C] in the workspace
int bn2d_bwd_partials(const float* G, const void* z, int z_is_x2, const BnPlan& pl, int64_t pixels, int C, const float* mean, const float* invstd,
                      void* workspace, int64_t workspace_bytes, hipStream_t st) {
  EHM_CHECK_ARG(G && z && mean && invstd && al16(G) && al16(z) && (z_is_x2 == 0 || z_is_x2 == 1) && workspace_ok(workspace, workspace_bytes, pl, C));
  launch_sum<2>(z_is_x2 != 0, pl, st, z, G, nullptr, mean, invstd, (double*)workspace, pixels, C);
  return 0;
}

// zbar's launch and its checks, for `total_rows` rows in the batch statistics: this call's own N Ho Wo (ehm_bn2d_train_bwd_zbar, whole 32-channel granules)
// or all ranks' (ehm_bn2d_train_bwd_zbar_rows: at least this rank's, which may be one; float32 rows need whole 8-channel lanes only)
int launch_zbar(const float* G, const void* z, int z_is_x2, int64_t z_rows, const float* mean, const float* invstd, const float* gamma, const float* gbeta,
                const float* ggamma, const float* scale, float* out, int N, int Ho, int Wo, int C, int H, int W, int cmult, int64_t total_rows,
                void* stream) {
  EHM_CHECK_ARG(G && z && mean && invstd && gamma && gbeta && ggamma && out && al16(G) && al16(z) && al16(out) && (z_is_x2 == 0 || z_is_x2 == 1));
  EHM_CHECK_ARG(N > 0 && Ho > 0 && Wo > 0 && H > 0 && W > 0 && C > 0 && C % cmult == 0);
  const bool dense = H == Ho && W == Wo;
  EHM_CHECK_ARG(dense || ((H - 1) / 2 + 1 == Ho && (W - 1) / 2 + 1 == Wo));
  const long long R = (long long)N * Ho * Wo;
  EHM_CHECK_ARG(total_rows >= 2 && total_rows >= R && total_rows < (1ll << 40) && z_rows >= R && (long long)N * H * W * C < (1ll << 40) &&
                (const void*)G != (const void*)out);
  ZbarArgs a;
  a.G = G; a.z = z; a.mean = mean; a.invstd = invstd; a.gamma = gamma; a.gbeta = gbeta; a.ggamma = ggamma; a.scale = scale; a.out = out;
  a.Ho = Ho; a.Wo = Wo; a.C = C; a.H = H; a.W = W; a.dil = dense ? 1 : 2;
  a.invR = (float)(1.0 / (double)total_rows);
  a.total8 = (long long)N * H * W * (C / 8);
  const long long blocks = ceil_div(a.total8, 256);
  EHM_CHECK_ARG(blocks < (1ll << 31));
  if (z_is_x2) hipLaunchKernelGGL(bn2d_zbar_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(bn2d_zbar_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  EHM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int ehm_bn2d_train_workspace_bytes(int64_t pixels, int C, int64_t* bytes) {
  EHM_CHECK_ARG(bytes != nullptr);
  BnPlan pl;
  const int rc = bn_plan(pixels, pixels, C, &pl);
  if (rc != 0) return rc;
  *bytes = bn_ws_doubles(pl, C) * (int64_t)sizeof(double);
  return 0;
}

extern "C" int ehm_bn2d_train_stats(const void* z, int z_is_x2, int64_t z_rows, int64_t pixels, int C, double eps, double momentum, float* mean, float* var,
                                    float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  BnPlan pl;
  BnMoments own;
  int rc = bn_plan(pixels, z_rows, C, &pl);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(mean && var && invstd && eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0);
  if ((rc = bn2d_moments(z, z_is_x2, pl, pixels, C, workspace, workspace_bytes, (hipStream_t)stream, &own)) != 0) return rc;
  hipLaunchKernelGGL(bn2d_stats_finish_kernel, dim3((unsigned)ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, own, (double*)nullptr, mean, var, invstd,
                     running_mean, running_var, (long long*)num_batches_tracked, C, eps, momentum);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_bn2d_train_bwd_sums(const float* G, const void* z, int z_is_x2, int64_t z_rows, int64_t pixels, int C, const float* mean,
                                       const float* invstd, float* gbeta, float* ggamma, void* workspace, int64_t workspace_bytes, void* stream) {
  BnPlan pl;
  int rc = bn_plan(pixels, z_rows, C, &pl);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(gbeta && ggamma);
  if ((rc = bn2d_bwd_partials(G, z, z_is_x2, pl, pixels, C, mean, invstd, workspace, workspace_bytes, (hipStream_t)stream)) != 0) return rc;
  hipLaunchKernelGGL(bn2d_bwd_reduce_kernel, dim3((unsigned)ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, pl.runs, 0, C,
                     (double*)nullptr, gbeta, ggamma, (float*)nullptr, (float*)nullptr);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_bn2d_train_bwd_zbar(const float* G, const void* z, int z_is_x2, int64_t z_rows, const float* mean, const float* invstd, const float* gamma,
                                       const float* gbeta, const float* ggamma, const float* scale, float* out, int N, int Ho, int Wo, int C, int H, int W,
                                       void* stream) {
  return launch_zbar(G, z, z_is_x2, z_rows, mean, invstd, gamma, gbeta, ggamma, scale, out, N, Ho, Wo, C, H, W, 32, (int64_t)N * Ho * Wo, stream);
}

// ---- data parallel: a rank's rows -> [2][C] float64, every rank's [world][2][C] (all-gathered by the caller, ONE collective per BatchNorm each way) -> the
// batch's.  Every rank merges the same buffer in the same order: all ranks hold the same bits.  rows [world] on the host: each rank's pixel count R_r.
// Each entry is a one-call entry's own body cut at the collective - the same helpers and kernels, another source or destination -, so with world == 1 a
// local + merge pair writes the bits of ehm_bn2d_train_stats / ehm_bn2d_train_bwd_sums, and zbar_rows with total_rows = N Ho Wo those of
// ehm_bn2d_train_bwd_zbar.  A rank may hold ONE row; float32 rows need C % 8 == 0 only (an X2 buffer C % 32 == 0, its format's granule).
extern "C" int ehm_bn2d_train_stats_local(const void* z, int z_is_x2, int64_t z_rows, int64_t pixels, int C, double* local, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
  BnPlan pl;
  BnMoments own;
  int rc = bn_plan(pixels, z_rows, C, &pl, 1, z_is_x2 ? 32 : 8);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(local && (uintptr_t)local % 8 == 0);
  if ((rc = bn2d_moments(z, z_is_x2, pl, pixels, C, workspace, workspace_bytes, (hipStream_t)stream, &own)) != 0) return rc;
  hipLaunchKernelGGL(bn2d_stats_finish_kernel, dim3((unsigned)ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, own, local, (float*)nullptr,
                     (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, (long long*)nullptr, C, 0.0, 0.0);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_bn2d_train_stats_merge(const double* gathered, const int64_t* rows, int world, int C, double eps, double momentum, float* mean, float* var,
                                          float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, void* stream) {
  BnMoments all = {nullptr, nullptr, 0, gathered, world, {}};
  const int rc = rank_rows_of(rows, world, &all.rr);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(gathered && (uintptr_t)gathered % 8 == 0 && mean && var && invstd && C > 0 && C % 8 == 0 && eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0);
  hipLaunchKernelGGL(bn2d_stats_finish_kernel, dim3((unsigned)ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, all, (double*)nullptr, mean, var, invstd,
                     running_mean, running_var, (long long*)num_batches_tracked, C, eps, momentum);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_bn2d_train_bwd_local(const float* G, const void* z, int z_is_x2, int64_t z_rows, int64_t pixels, int C, const float* mean,
                                        const float* invstd, double* local, void* workspace, int64_t workspace_bytes, void* stream) {
  BnPlan pl;
  int rc = bn_plan(pixels, z_rows, C, &pl, 1, z_is_x2 ? 32 : 8);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(local && (uintptr_t)local % 8 == 0);
  if ((rc = bn2d_bwd_partials(G, z, z_is_x2, pl, pixels, C, mean, invstd, workspace, workspace_bytes, (hipStream_t)stream)) != 0) return rc;
  hipLaunchKernelGGL(bn2d_bwd_reduce_kernel, dim3((unsigned)ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, pl.runs, 0, C,
                     local, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  EHM_LAUNCH_CHECK();
  return 0;
}

// gbeta / ggamma: the whole batch's sums, for ehm_bn2d_train_bwd_zbar_rows; gbeta_own / ggamma_own (either may be NULL): rank `rank`'s own
extern "C" int ehm_bn2d_train_bwd_merge(const double* gathered, int world, int rank, int C, float* gbeta, float* ggamma, float* gbeta_own,
                                        float* ggamma_own, void* stream) {
  EHM_CHECK_ARG(gathered && (uintptr_t)gathered % 8 == 0 && world >= 1 && world <= kMaxRanks && rank >= 0 && rank < world && C > 0 && C % 8 == 0);
  EHM_CHECK_ARG(gbeta && ggamma);
  hipLaunchKernelGGL(bn2d_bwd_reduce_kernel, dim3((unsigned)ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, gathered, world, rank, C, (double*)nullptr,
                     gbeta, ggamma, gbeta_own, ggamma_own);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_bn2d_train_bwd_zbar_rows(const float* G, const void* z, int z_is_x2, int64_t z_rows, const float* mean, const float* invstd,
                                            const float* gamma, const float* gbeta, const float* ggamma, const float* scale, float* out, int N, int Ho,
                                            int Wo, int C, int H, int W, int64_t total_rows, void* stream) {
  return launch_zbar(G, z, z_is_x2, z_rows, mean, invstd, gamma, gbeta, ggamma, scale, out, N, Ho, Wo, C, H, W, z_is_x2 ? 32 : 8, total_rows, stream);
}
