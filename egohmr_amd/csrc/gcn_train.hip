// Train-mode BatchNorm of the Modulated-GCN denoiser's graph convs for gfx950 (MI355X): batch statistics, running-statistic updates and the backward
// through the mean and the variance.  The forward it implements, per BatchNorm'd conv (input conv and every hidden conv):
//   ModulatedGraphConv.forward     models/egohmr/modulated_gcn/modulated_gcn_conv.py:39-50
//   _GraphConv / _ResGraphConv     models/egohmr/modulated_gcn/modulated_gcn.py:21-28, :38-42   (nn.BatchNorm1d(hid) on [B, hid, 24], self.training)
//
// Notation (R = 24 bodies rows, h_k = X W_k from the caller's GEMM, A = sym(adj + adj2)):
//   z[j] = A_jj M_j h0[j] + sum_{i != j} A_ji M_i h1[i] + bias,   mean = sum z / R,   var = sum (z - mean)^2 / R  (biased),   invstd = 1 / sqrt(var + eps),
//   xhat = (z - mean) invstd,   v = gamma xhat + beta,   y = relu(v),   out = y (+ res),
//   running_mean <- (1 - m) running_mean + m mean,   running_var <- (1 - m) running_var + m var R / (R - 1).
// and with g = dL/dout:  vbar = g [y > 0],  betabar = sum vbar,  gammabar = sum vbar xhat,  zbar = gamma invstd (vbar - betabar / R - xhat gammabar / R).
// From zbar on a conv's backward is the output conv's of gcn_bwd.hip (no gate, T0 = T1 = M, the full symmetrised adjacency): ehm_gcn_train_bwd_* there.
//
//   train_sym_adj_kernel      adj, adj2 -> A [24][24], once per conv and call (ehm_gcn_train_adjacency): the forward and the backward read it through scalar
//                             loads, like the eval-mode kernels read theirs.
//   train_preact_kernel       pre = X [W0 | W1] -> z.  One lane = one channel; a block walks its bodies in a fixed order and keeps the channel's sum of z in
//                             float64: partial column sums [groups][N].  HBM bound: 8 N bytes read and 4 N written per row.
//   train_colsum_kernel       z -> partial sums of z (a z that did not come from train_preact_kernel) or of (z - mean)^2, float64.  4 N bytes read per row.
//   train_mean_kernel         partial sums, added in index order -> mean (float64, in the workspace).
//   train_stats_finish        (mean, M2 = sum of squares centred on it) of the call's own rows, or of every rank's through merge_moments (BnMoments,
//                             common.h) -> mean, invstd (float32) and the running statistics; or, for a rank's share, the pair itself [2][N] float64.
//   train_normalize_kernel    z -> y = relu(gamma xhat + beta) and out = y + res.  4 N (+ 4 N) bytes read and 4 N (+ 4 N) written per row.
//   train_bnbwd_partial       g, gate, z -> partial sums of vbar and vbar xhat (float64).  12 N bytes read per row.
//   train_bwd_reduce          partial sums, or every rank's sums, added in index order -> betabar, gammabar (float32; under data parallel the rank's
//                             OWN) and betabar / R, gammabar / R in the workspace; or, for a rank's share, the two sums themselves [2][N] float64.
//   train_zbar_kernel         g, gate, z -> zbar.  12 N bytes read and 4 N written per row.
// The statistics are two-pass sums in float64 in a fixed order: exact to the float32 rounding of their results, whatever |mean| / std is.  No atomics
// anywhere: two calls on the same inputs give the same bits.  The kernels read the raw parameter arrays the handle was created on, never its
// BatchNorm-folded tables.
//
// Data parallel (ehm_gcn_train_stats_local / _stats_merge / _bwd_local / _bwd_merge): each rank runs the same passes on its own rows and stops at [2][N]
// float64; the caller all-gathers them ([world][2][N], ONE collective per BatchNorm each way) and every rank merges the same buffer in the same order, so all
// ranks hold the same bits.  The pair is the one-call entry's own body cut at the collective: train_moments / train_bwd_partials issue the passes for
// both, train_stats_finish / train_bwd_reduce write out for both (merge_moments gives ONE rank's pair back bit for bit), train_backward ends both.  So
// with world == 1 a local + merge pair gives the bits of ehm_gcn_train_stats / ehm_gcn_train_bn_backward by construction.
#include "common.h"
#include "egohmr_hip.h"
#include "gcn_dev.h"
#include "internal.h"

namespace {

constexpr int NT = 256;            // channels per block of the column kernels
constexpr int kMaxGroups = 128;    // body groups of the column kernels (a group's bodies are summed in one lane)

struct TrainConv {
  ehm_gconv_params raw;
  const float* adj;
  int N;
};

__global__ void train_sym_adj_kernel(const float* __restrict__ adj, const float* __restrict__ adj2, float* __restrict__ A) {
  const int t = threadIdx.x;
  if (t >= kJ * kJ) return;
  const int i = t / kJ, j = t % kJ;
  const float aij = adj[i * kJ + j] + adj2[i * kJ + j];
  const float aji = adj[j * kJ + i] + adj2[j * kJ + i];
  A[t] = (i == j) ? aij : (aji + aij) / 2;                    // (adj.T + adj)/2, modulated_gcn_conv.py:44
}

__global__ __launch_bounds__(NT) void train_preact_kernel(const float* __restrict__ pre, int ld_pre, TrainConv c, const float* __restrict__ A,
                                                          float* __restrict__ z, double* __restrict__ part, int bodies, int groups, int chunks) {
  const int N = c.N;
  const int chunk = blockIdx.x % chunks, grp = blockIdx.x / chunks;
  const int n = chunk * NT + threadIdx.x;
  if (n >= N) return;
  float Mj[kJ];
#pragma unroll
  for (int j = 0; j < kJ; ++j) Mj[j] = c.raw.M[(size_t)j * N + n];
  const float bias = c.raw.bias ? c.raw.bias[n] : 0.f;
  double s = 0.0;
  for (int b = grp; b < bodies; b += groups) {
    const size_t row0 = (size_t)b * kJ;
    float h0[kJ], u1[kJ];
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
      h0[j] = pre[(row0 + j) * ld_pre + n];
      u1[j] = pre[(row0 + j) * ld_pre + N + n];
    }
#pragma unroll
    for (int j = 0; j < kJ; ++j) u1[j] *= Mj[j];
    // A is wave-uniform: scalar loads through the constant address space (gcn_dev.h, gcn_mix_store).  The pointer is made opaque per body, or hipcc hoists
    // all 576 coefficients out of the body loop and spills SGPRs into VGPR lanes
    typedef const float __attribute__((address_space(4))) cfloat;
    const float* Ab = A;
    asm volatile("" : "+s"(Ab));
    const cfloat* Ac = (const cfloat*)(uintptr_t)Ab;
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
      float zj = fmaf(Ac[j * kJ + j], Mj[j] * h0[j], bias);
#pragma unroll
      for (int i = 0; i < kJ; ++i)
        if (i != j) zj = fmaf(Ac[j * kJ + i], u1[i], zj);
      z[(row0 + j) * N + n] = zj;
      s += (double)zj;
    }
  }
  part[(size_t)grp * N + n] = s;
}

template <bool SQ>
__global__ __launch_bounds__(NT) void train_colsum_kernel(const float* __restrict__ z, const double* __restrict__ meand, double* __restrict__ part, int N,
                                                          int bodies, int groups, int chunks) {
  const int chunk = blockIdx.x % chunks, grp = blockIdx.x / chunks;
  const int n = chunk * NT + threadIdx.x;
  if (n >= N) return;
  const double mean = SQ ? meand[n] : 0.0;
  double s = 0.0;
  for (int b = grp; b < bodies; b += groups) {
    const size_t row0 = (size_t)b * kJ;
    float v[kJ];
#pragma unroll
    for (int j = 0; j < kJ; ++j) v[j] = z[(row0 + j) * N + n];
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
      const double d = (double)v[j] - mean;
      s += SQ ? d * d : d;
    }
  }
  part[(size_t)grp * N + n] = s;
}

__global__ __launch_bounds__(256) void train_mean_kernel(const double* __restrict__ part, double* __restrict__ meand, int N, int groups, double R) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n < N) meand[n] = ordered_sum(part + n, N, groups) / R;
}

// (mean, M2 = sum of squares centred on that mean) of this call's own rows or of every rank's (BnMoments, common.h) -> local[0][n] = mean, local[1][n] = M2
// and nothing else (a rank's share), or the batch's mean, invstd (float32) and the running statistics
__global__ __launch_bounds__(256) void train_stats_finish(BnMoments src, int N, double eps, double momentum, double* __restrict__ local,
                                                          float* __restrict__ mean, float* __restrict__ invstd, float* __restrict__ running_mean,
                                                          float* __restrict__ running_var) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double mu, M2;
  moments_of(src, n, N, &mu, &M2);
  if (local) {
    local[n] = mu;
    local[N + n] = M2;
    return;
  }
  const double R = src.rr.total, var = M2 / R;
  mean[n] = (float)mu;
  invstd[n] = (float)(1.0 / sqrt(var + eps));
  if (running_mean) running_mean[n] = (float)((1.0 - momentum) * (double)running_mean[n] + momentum * mu);
  if (running_var) running_var[n] = (float)((1.0 - momentum) * (double)running_var[n] + momentum * var * (R / (R - 1.0)));
}

// four channels per lane (N % 4 == 0: train_conv_of)
__global__ __launch_bounds__(256) void train_normalize_kernel(const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ res, float* __restrict__ y, float* __restrict__ out, int N4,
                                                              long long total4) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total4) return;
  const int n4 = (int)(t % N4);
  const f32x4 zv = ((const f32x4*)z)[t], mu = ((const f32x4*)mean)[n4], is = ((const f32x4*)invstd)[n4], ga = ((const f32x4*)gamma)[n4],
              be = ((const f32x4*)beta)[n4];
  f32x4 yv;
#pragma unroll
  for (int q = 0; q < 4; ++q) yv[q] = fmaxf(fmaf(ga[q], (zv[q] - mu[q]) * is[q], be[q]), 0.f);
  if (y) ((f32x4*)y)[t] = yv;
  if (out) ((f32x4*)out)[t] = res ? yv + ((const f32x4*)res)[t] : yv;
}

__global__ __launch_bounds__(NT) void train_bnbwd_partial(const float* __restrict__ gout, const float* __restrict__ gate, const float* __restrict__ z,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd, double* __restrict__ bpart,
                                                          double* __restrict__ gpart, int N, int bodies, int groups, int chunks) {
  const int chunk = blockIdx.x % chunks, grp = blockIdx.x / chunks;
  const int n = chunk * NT + threadIdx.x;
  if (n >= N) return;
  const float mu = mean[n], is = invstd[n];
  double sb = 0.0, sg = 0.0;
  for (int b = grp; b < bodies; b += groups) {
    const size_t row0 = (size_t)b * kJ;
    float v[kJ], yv[kJ], zv[kJ];
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
      v[j] = gout[(row0 + j) * N + n];
      yv[j] = gate[(row0 + j) * N + n];
      zv[j] = z[(row0 + j) * N + n];
    }
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
      const float vb = yv[j] > 0.f ? v[j] : 0.f;
      sb += (double)vb;
      sg += (double)vb * (double)((zv[j] - mu) * is);
    }
  }
  bpart[(size_t)grp * N + n] = sb;
  gpart[(size_t)grp * N + n] = sg;
}

// A channel's `count` float64 entries b[k stride] and g[k stride] (sums of vbar and of vbar xhat), added in index order: a call's partial sums (count =
// groups) or every rank's sums (count = world).  With `local`: that pair [2][N] in float64, a rank's share, and nothing else.  Without: betabar / R and
// gammabar / R for train_zbar_kernel, and the float32 parameter gradients - of the total, or with own >= 0 of entry `own` alone (the rank's OWN sums: the
// caller's gradient all-reduce completes them).
__global__ __launch_bounds__(256) void train_bwd_reduce(const double* __restrict__ b, const double* __restrict__ g, size_t stride, int count, int own,
                                                        int N, double R, double* __restrict__ local, float* __restrict__ gbn_weight,
                                                        float* __restrict__ gbn_bias, float* __restrict__ bR, float* __restrict__ gR) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const double sb = ordered_sum(b + n, stride, count), sg = ordered_sum(g + n, stride, count);
  if (local) {
    local[n] = sb;
    local[N + n] = sg;
    return;
  }
  if (gbn_bias) gbn_bias[n] = (float)(own < 0 ? sb : b[own * stride + n]);
  if (gbn_weight) gbn_weight[n] = (float)(own < 0 ? sg : g[own * stride + n]);
  bR[n] = (float)(sb / R);
  gR[n] = (float)(sg / R);
}

__global__ __launch_bounds__(256) void train_zbar_kernel(const float* __restrict__ gout, const float* __restrict__ gate, const float* __restrict__ z,
                                                         const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                         const float* __restrict__ bR, const float* __restrict__ gR, float* __restrict__ zbar, int N4,
                                                         long long total4) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total4) return;
  const int n4 = (int)(t % N4);
  const f32x4 g = ((const f32x4*)gout)[t], yv = ((const f32x4*)gate)[t], zv = ((const f32x4*)z)[t];
  const f32x4 mu = ((const f32x4*)mean)[n4], is = ((const f32x4*)invstd)[n4], ga = ((const f32x4*)gamma)[n4], b = ((const f32x4*)bR)[n4],
              gr = ((const f32x4*)gR)[n4];
  f32x4 o;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float vb = yv[q] > 0.f ? g[q] : 0.f;
    const float xh = (zv[q] - mu[q]) * is[q];
    o[q] = (ga[q] * is[q]) * ((vb - b[q]) - xh * gr[q]);
  }
  ((f32x4*)zbar)[t] = o;
}

// the handle's BatchNorm'd conv `conv` (EHM_GCN_CONV_INPUT or a hidden conv's index)
int train_conv_of(const ehm_gcn* h, int conv, TrainConv* c) {
  EHM_CHECK_ARG(h && (conv == EHM_GCN_CONV_INPUT || (conv >= 0 && conv < h->num_hidden)));
  c->raw = conv == EHM_GCN_CONV_INPUT ? h->raw_input : h->raw_hidden[conv];
  c->adj = h->adj;
  c->N = c->raw.out_dim;
  EHM_CHECK_ARG(c->adj && c->raw.M && c->raw.adj2 && c->raw.bn_weight && c->raw.bn_bias && c->N > 0 && c->N % 4 == 0);
  return 0;
}

int groups_of(int bodies) { return bodies < kMaxGroups ? bodies : kMaxGroups; }

// workspace: part0, part1 [groups][N] float64 | mean [N] float64 | betabar / R, gammabar / R [N] float
int64_t train_bytes(int N, int bodies) { return ((int64_t)2 * groups_of(bodies) * N + N) * 8 + (int64_t)2 * N * 4; }

// the workspace cut up, and the two grids of a conv's launches: (body group, 256-channel chunk) blocks of the column kernels, one lane per channel
struct TrainPlan {
  double* part0; double* part1; double* meand; float* bR; float* gR;
  int groups, chunks;
  dim3 cgrid, ngrid;
};

TrainPlan plan_of(void* workspace, int N, int bodies) {
  TrainPlan w;
  w.groups = groups_of(bodies);
  w.chunks = (int)ceil_div(N, NT);
  w.part0 = (double*)workspace;
  w.part1 = w.part0 + (size_t)w.groups * N;
  w.meand = w.part1 + (size_t)w.groups * N;
  w.bR = (float*)(w.meand + N);
  w.gR = w.bR + N;
  w.cgrid = dim3((unsigned)(w.groups * w.chunks));
  w.ngrid = dim3((unsigned)ceil_div(N, 256));
  return w;
}

bool workspace_ok(const void* workspace, int64_t workspace_bytes, int N, int bodies) {
  return workspace && (uintptr_t)workspace % 16 == 0 && workspace_bytes >= train_bytes(N, bodies);
}

// The launches every statistics entry starts with, and their checks: z -> its mean (float64, w->meand) and the partial sums of (z - mean)^2 (w->part1)
int train_moments(const TrainConv& c, const float* z, int bodies, int have_sums, void* workspace, int64_t workspace_bytes, hipStream_t st, TrainPlan* w) {
  EHM_CHECK_ARG(z && bodies > 0 && (have_sums == 0 || have_sums == 1));
  EHM_CHECK_ARG(workspace_ok(workspace, workspace_bytes, c.N, bodies));
  *w = plan_of(workspace, c.N, bodies);
  if (!have_sums)
    hipLaunchKernelGGL(train_colsum_kernel<false>, w->cgrid, dim3(NT), 0, st, z, (const double*)nullptr, w->part0, c.N, bodies, w->groups, w->chunks);
  hipLaunchKernelGGL(train_mean_kernel, w->ngrid, dim3(256), 0, st, (const double*)w->part0, w->meand, c.N, w->groups, (double)bodies * kJ);
  hipLaunchKernelGGL(train_colsum_kernel<true>, w->cgrid, dim3(NT), 0, st, z, (const double*)w->meand, w->part1, c.N, bodies, w->groups, w->chunks);
  return 0;
}

// The launch every backward over a rank's own rows starts with, and its checks: partial sums of vbar (w->part0) and of vbar xhat (w->part1)
int train_bwd_partials(const TrainConv& c, const float* gout, const float* gate, const float* z, const float* mean, const float* invstd, int bodies,
                       void* workspace, int64_t workspace_bytes, hipStream_t st, TrainPlan* w) {
  EHM_CHECK_ARG(gout && gate && z && mean && invstd && bodies > 0);
  EHM_CHECK_ARG(workspace_ok(workspace, workspace_bytes, c.N, bodies));
  *w = plan_of(workspace, c.N, bodies);
  hipLaunchKernelGGL(train_bnbwd_partial, w->cgrid, dim3(NT), 0, st, gout, gate, z, mean, invstd, w->part0, w->part1, c.N, bodies, w->groups, w->chunks);
  return 0;
}

// The backward from the sums on: betabar / R, gammabar / R, the parameter gradients and zbar, with every check of zbar's launch made before the first
// launch.  gathered == NULL (ehm_gcn_train_bn_backward): this call's own sums over R = 24 bodies rows, computed here.  Else (ehm_gcn_train_bwd_merge):
// every rank's [world][2][N] over R rows in all, and the parameter gradients are rank `rank`'s own.
int train_backward(const TrainConv& c, const double* gathered, int world, int rank, double R, const float* gout, const float* gate, const float* z,
                   const float* mean, const float* invstd, int bodies, float* zbar, float* gbn_weight, float* gbn_bias, void* workspace,
                   int64_t workspace_bytes, hipStream_t st) {
  EHM_CHECK_ARG(gout && gate && z && mean && invstd && zbar && bodies > 0);
  EHM_CHECK_ARG((const void*)zbar != (const void*)gate && (const void*)zbar != (const void*)z);
  EHM_CHECK_ARG(((uintptr_t)gout | (uintptr_t)gate | (uintptr_t)z | (uintptr_t)mean | (uintptr_t)invstd | (uintptr_t)zbar |
                 (uintptr_t)c.raw.bn_weight) % 16 == 0);
  const long long total4 = (long long)bodies * kJ * (c.N / 4);
  EHM_CHECK_ARG(ceil_div(total4, 256) < (1ll << 31));
  TrainPlan w;
  const bool own = !gathered;
  if (own) {
    const int rc = train_bwd_partials(c, gout, gate, z, mean, invstd, bodies, workspace, workspace_bytes, st, &w);
    if (rc != 0) return rc;
  } else {
    EHM_CHECK_ARG(workspace_ok(workspace, workspace_bytes, c.N, bodies));
    w = plan_of(workspace, c.N, bodies);
  }
  hipLaunchKernelGGL(train_bwd_reduce, w.ngrid, dim3(256), 0, st, own ? (const double*)w.part0 : gathered, own ? (const double*)w.part1 : gathered + c.N,
                     (size_t)(own ? c.N : 2 * c.N), own ? w.groups : world, own ? -1 : rank, c.N, R, (double*)nullptr, gbn_weight, gbn_bias, w.bR, w.gR);
  hipLaunchKernelGGL(train_zbar_kernel, dim3((unsigned)ceil_div(total4, 256)), dim3(256), 0, st, gout, gate, z, mean, invstd, c.raw.bn_weight,
                     (const float*)w.bR, (const float*)w.gR, zbar, c.N / 4, total4);
  EHM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int ehm_gcn_train_adjacency(const ehm_gcn* h, int conv, float* A, void* stream) {
  TrainConv c;
  const int rc = train_conv_of(h, conv, &c);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(A);
  hipLaunchKernelGGL(train_sym_adj_kernel, dim3(1), dim3(kJ * kJ), 0, (hipStream_t)stream, c.adj, c.raw.adj2, A);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_gcn_train_workspace_bytes(const ehm_gcn* h, int conv, int bodies, int64_t* bytes) {
  TrainConv c;
  const int rc = train_conv_of(h, conv, &c);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(bytes && bodies > 0);
  *bytes = train_bytes(c.N, bodies);
  return 0;
}

extern "C" int ehm_gcn_train_preact(const ehm_gcn* h, int conv, const float* pre, int ld_pre, int bodies, const float* A, float* z, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  TrainConv c;
  const int rc = train_conv_of(h, conv, &c);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(pre && A && z && bodies > 0 && ld_pre >= 2 * c.N && (const void*)pre != (const void*)z);
  EHM_CHECK_ARG(workspace_ok(workspace, workspace_bytes, c.N, bodies));
  const TrainPlan w = plan_of(workspace, c.N, bodies);
  hipLaunchKernelGGL(train_preact_kernel, w.cgrid, dim3(NT), 0, (hipStream_t)stream, pre, ld_pre, c, A, z, w.part0, bodies, w.groups, w.chunks);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_gcn_train_stats(const ehm_gcn* h, int conv, const float* z, int bodies, int have_sums, double eps, double momentum, float* mean,
                                   float* invstd, float* running_mean, float* running_var, void* workspace, int64_t workspace_bytes, void* stream) {
  TrainConv c;
  int rc = train_conv_of(h, conv, &c);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(mean && invstd && eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0);
  EHM_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr));
  TrainPlan w;
  if ((rc = train_moments(c, z, bodies, have_sums, workspace, workspace_bytes, (hipStream_t)stream, &w)) != 0) return rc;
  hipLaunchKernelGGL(train_stats_finish, w.ngrid, dim3(256), 0, (hipStream_t)stream, own_moments(w.part1, w.meand, w.groups, (double)bodies * kJ), c.N, eps,
                     momentum, (double*)nullptr, mean, invstd, running_mean, running_var);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_gcn_train_normalize(const ehm_gcn* h, int conv, const float* z, const float* mean, const float* invstd, const float* residual,
                                       float* y, float* out, int bodies, void* stream) {
  TrainConv c;
  const int rc = train_conv_of(h, conv, &c);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(z && mean && invstd && bodies > 0 && (y || out) && (!residual || out));
  EHM_CHECK_ARG(((uintptr_t)z | (uintptr_t)mean | (uintptr_t)invstd | (uintptr_t)residual | (uintptr_t)y | (uintptr_t)out |
                 (uintptr_t)c.raw.bn_weight | (uintptr_t)c.raw.bn_bias) % 16 == 0);
  const long long total4 = (long long)bodies * kJ * (c.N / 4);
  EHM_CHECK_ARG(ceil_div(total4, 256) < (1ll << 31));
  hipLaunchKernelGGL(train_normalize_kernel, dim3((unsigned)ceil_div(total4, 256)), dim3(256), 0, (hipStream_t)stream, z, mean, invstd, c.raw.bn_weight,
                     c.raw.bn_bias, residual, y, out, c.N / 4, total4);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_gcn_train_bn_backward(const ehm_gcn* h, int conv, const float* gout, const float* gate, const float* z, const float* mean,
                                         const float* invstd, int bodies, float* zbar, float* gbn_weight, float* gbn_bias, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
  TrainConv c;
  const int rc = train_conv_of(h, conv, &c);
  if (rc != 0) return rc;
  return train_backward(c, nullptr, 1, 0, (double)bodies * kJ, gout, gate, z, mean, invstd, bodies, zbar, gbn_weight, gbn_bias, workspace, workspace_bytes,
                        (hipStream_t)stream);
}

// ---- data parallel: a rank's rows -> [2][N] float64, every rank's [world][2][N] -> the batch's.  rows [world] on the host: each rank's R_r = 24 bodies_r.
// Each entry is the one-call entry's own body cut at the collective: the same helpers, the same kernels, another source or destination.
extern "C" int ehm_gcn_train_stats_local(const ehm_gcn* h, int conv, const float* z, int bodies, int have_sums, double* local, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
  TrainConv c;
  int rc = train_conv_of(h, conv, &c);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(local && (uintptr_t)local % 8 == 0);
  TrainPlan w;
  if ((rc = train_moments(c, z, bodies, have_sums, workspace, workspace_bytes, (hipStream_t)stream, &w)) != 0) return rc;
  hipLaunchKernelGGL(train_stats_finish, w.ngrid, dim3(256), 0, (hipStream_t)stream, own_moments(w.part1, w.meand, w.groups, (double)bodies * kJ), c.N, 0.0,
                     0.0, local, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_gcn_train_stats_merge(const ehm_gcn* h, int conv, const double* gathered, const int64_t* rows, int world, double eps, double momentum,
                                         float* mean, float* invstd, float* running_mean, float* running_var, void* stream) {
  TrainConv c;
  int rc = train_conv_of(h, conv, &c);
  if (rc != 0) return rc;
  BnMoments all = {nullptr, nullptr, 0, gathered, world, {}};
  if ((rc = rank_rows_of(rows, world, &all.rr)) != 0) return rc;
  EHM_CHECK_ARG(gathered && (uintptr_t)gathered % 8 == 0 && mean && invstd && eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0);
  EHM_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr));
  for (int k = 0; k < world; ++k) EHM_CHECK_ARG(rows[k] % kJ == 0);
  hipLaunchKernelGGL(train_stats_finish, dim3((unsigned)ceil_div(c.N, 256)), dim3(256), 0, (hipStream_t)stream, all, c.N, eps, momentum, (double*)nullptr,
                     mean, invstd, running_mean, running_var);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_gcn_train_bwd_local(const ehm_gcn* h, int conv, const float* gout, const float* gate, const float* z, const float* mean,
                                       const float* invstd, int bodies, double* local, void* workspace, int64_t workspace_bytes, void* stream) {
  TrainConv c;
  int rc = train_conv_of(h, conv, &c);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(local && (uintptr_t)local % 8 == 0);
  TrainPlan w;
  if ((rc = train_bwd_partials(c, gout, gate, z, mean, invstd, bodies, workspace, workspace_bytes, (hipStream_t)stream, &w)) != 0) return rc;
  hipLaunchKernelGGL(train_bwd_reduce, w.ngrid, dim3(256), 0, (hipStream_t)stream, (const double*)w.part0, (const double*)w.part1, (size_t)c.N, w.groups, -1,
                     c.N, 0.0, local, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_gcn_train_bwd_merge(const ehm_gcn* h, int conv, const double* gathered, const int64_t* rows, int world, int rank, const float* gout,
                                       const float* gate, const float* z, const float* mean, const float* invstd, int bodies, float* zbar,
                                       float* gbn_weight, float* gbn_bias, void* workspace, int64_t workspace_bytes, void* stream) {
  TrainConv c;
  int rc = train_conv_of(h, conv, &c);
  if (rc != 0) return rc;
  RankRows rr;
  if ((rc = rank_rows_of(rows, world, &rr)) != 0) return rc;
  EHM_CHECK_ARG(gathered && (uintptr_t)gathered % 8 == 0 && rank >= 0 && rank < world && bodies > 0 && rows[rank] == (int64_t)bodies * kJ);
  return train_backward(c, gathered, world, rank, rr.total, gout, gate, z, mean, invstd, bodies, zbar, gbn_weight, gbn_bias, workspace, workspace_bytes,
                        (hipStream_t)stream);
}
