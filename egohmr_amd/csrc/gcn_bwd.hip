// Vector-Jacobian product of the Modulated-GCN denoiser's graph convs for gfx950 (MI355X): everything of a conv's backward that is not a GEMM.
// The forward it differentiates (eval-mode BatchNorm, first derivatives):
//   ModulatedGraphConv.forward     models/egohmr/modulated_gcn/modulated_gcn_conv.py:39-50
//   _GraphConv / _ResGraphConv     models/egohmr/modulated_gcn/modulated_gcn.py:21-28, :38-42
//   ModulatedGCN.forward           modulated_gcn.py:99-116
//
// Notation (X [b,24,K], h_k = X W_k, u_k = M (.) h_k, A = sym(adj + adj2), c = gamma / sqrt(var + eps)):
//   z[j] = A_jj u0[j] + sum_{i != j} A_ji u1[i] + bias,   v = c (z - mean) + beta,   y = relu(v)  (output conv: y = z),   out = y (+ res)
// and with g = dL/dout:  vbar = g [y > 0] (output conv: zbar = g),  zbar = c vbar,  u0bar[j] = A_jj zbar[j],  u1bar[i] = sum_{j != i} A_ji zbar[j],
//   hbar_k = M (.) ukbar,  Mbar = sum_b (u0bar h0 + u1bar h1),  Abar_jj = sum zbar[j] u0[j],  Abar_ji = sum zbar[j] u1[i],  adj2bar = (Abar + Abar^T) / 2,
//   biasbar = sum zbar,  betabar = sum vbar,  gammabar = sum vbar (z - mean) / sqrt(var + eps).
// The three GEMMs of a conv's backward (recompute X [W0|W1], Xbar = G [W0;W1]^T, Wbar = X^T G) run on ehm_conv_nhwc_split.
//
//   gcn_bwd_epilogue_kernel   g, gate -> G [rows, 2N] = [h0bar | h1bar].  One lane = one channel of one body: 24 gated cotangents in registers, the
//                             24 x 24 transposed-adjacency mix as scalar-broadcast FMAs (the adjacency through scalar loads, like the forward epilogue), the
//                             folded coefficients D = A_jj M c and M1 = M c of the handle.  HBM bound: 2 x 4 N bytes read and 8 N written per row.
//   gcn_bwd_params_kernel     g, gate, recomputed pre-activations -> per-block partial sums.  One lane = one channel; a block walks its bodies in a fixed
//                             order; Abar = Zbar U1^T (24 x NT x 24 per body) goes through LDS: 4 k-groups x 64 lanes x (3 x 3) register blocks.
//   gcn_bwd_params_finish     adds the partial sums in index order (float64) -> Mbar, adj2bar, biasbar, gammabar, betabar.
// No atomics anywhere: two calls on the same inputs give the same bits.
#include "common.h"
#include "egohmr_hip.h"
#include "gcn_dev.h"
#include "internal.h"

namespace {

constexpr int NT = 256;            // channels per block of the parameter kernel
constexpr int LDT = NT + 4;        // LDS row stride (floats): 16-byte aligned rows, rows 4 banks apart
constexpr int kMaxGroups = 128;    // body groups of the parameter kernel (a group's bodies are summed in registers)

// One conv as the backward kernels read it.  OUT (the output conv): T0 = T1 = M [24][N], A = the full symmetrised adjacency; else T0 = D, T1 = M1 (BatchNorm
// folded in) and A = Aoff (zero diagonal).  The diagonal of A is never read through A: i == j is skipped at compile time.
struct BwdConv {
  const float* T0; const float* T1; const float* A;
  ehm_gconv_params raw;      // M, adj2, bias, bn_*: the parameter reductions' own arithmetic (nothing folded)
  const float* adj;
  int N, bn, out;
};

template <bool OUT>
__global__ __launch_bounds__(256) void gcn_bwd_epilogue_kernel(const float* __restrict__ gout, const float* __restrict__ gate,
                                                               const float* __restrict__ T0, const float* __restrict__ T1,
                                                               const float* __restrict__ A, float* __restrict__ G, int N, int ldg,
                                                               long long total) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long long b = t / N;
  const int n = (int)(t - b * N);
  const float* g = gout + b * kJ * N + n;
  float v[kJ];
#pragma unroll
  for (int j = 0; j < kJ; ++j) v[j] = g[(size_t)j * N];
  if (gate) {                                     // [y > 0] of the forward's activation BEFORE the residual add
    const float* y = gate + b * kJ * N + n;
    float yv[kJ];
#pragma unroll
    for (int j = 0; j < kJ; ++j) yv[j] = y[(size_t)j * N];
#pragma unroll
    for (int j = 0; j < kJ; ++j) v[j] = yv[j] > 0.f ? v[j] : 0.f;
  }
  float* o = G + b * kJ * ldg + n;
#pragma unroll
  for (int i = 0; i < kJ; ++i) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kJ; ++j)
      if (j != i) s = fmaf(A[i * kJ + j], v[j], s);          // A symmetric: A_ji = A_ij
    const float d = OUT ? A[i * kJ + i] * T0[(size_t)i * N + n] : T0[(size_t)i * N + n];
    o[(size_t)i * ldg] = d * v[i];
    o[(size_t)i * ldg + N] = T1[(size_t)i * N + n] * s;
  }
}

struct ParamArgs {
  const float* gout; const float* gate; const float* pre;
  BwdConv c;
  int ld_pre, bodies, groups, chunks;
  float* Mpart;     // [groups][24][N]
  float* bpart;     // [groups][N]   sum vbar
  float* gpart;     // [groups][N]   sum vbar (z - mean) / sqrt(var + eps)
  float* Apart;     // [groups * chunks][24 * 24]
};

__global__ __launch_bounds__(NT) void gcn_bwd_params_kernel(ParamArgs p) {
  __shared__ __attribute__((aligned(16))) float Zs[kJ * LDT];
  __shared__ __attribute__((aligned(16))) float Us[kJ * LDT];
  const int tid = threadIdx.x, N = p.c.N;
  const int chunk = blockIdx.x % p.chunks, grp = blockIdx.x / p.chunks;
  const int n = chunk * NT + tid;
  const bool live = n < N;
  const int nn = live ? n : 0;
  const float* __restrict__ A = p.c.A;
  const float* __restrict__ adj = p.c.adj;
  const float* __restrict__ adj2 = p.c.raw.adj2;

  float Mj[kJ], macc[kJ], dacc[kJ];
#pragma unroll
  for (int j = 0; j < kJ; ++j) {
    Mj[j] = live ? p.c.raw.M[(size_t)j * N + nn] : 0.f;
    macc[j] = 0.f;
    dacc[j] = 0.f;
  }
  float c = 1.f, mean = 0.f, rstd = 1.f;
  const float bias = (live && p.c.raw.bias) ? p.c.raw.bias[nn] : 0.f;
  if (p.c.bn) {
    rstd = 1.f / sqrtf(p.c.raw.bn_var[nn] + 1e-5f);          // BatchNorm1d eval, eps = 1e-5
    c = p.c.raw.bn_weight[nn] * rstd;
    mean = p.c.raw.bn_mean[nn];
  }
  float bacc = 0.f, gacc = 0.f;
  float acc[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int e = 0; e < 3; ++e) acc[a][e] = 0.f;
  const int kg = tid >> 6, l = tid & 63, jb = l >> 3, ib = l & 7;

  for (int b = grp; b < p.bodies; b += p.groups) {
    float v[kJ], h0[kJ], h1[kJ];
    const size_t row0 = (size_t)b * kJ;
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
      v[j] = live ? p.gout[(row0 + j) * N + nn] : 0.f;
      h0[j] = live ? p.pre[(row0 + j) * p.ld_pre + nn] : 0.f;
      h1[j] = live ? p.pre[(row0 + j) * p.ld_pre + N + nn] : 0.f;
    }
    if (p.gate) {
#pragma unroll
      for (int j = 0; j < kJ; ++j) v[j] = (live && p.gate[(row0 + j) * N + nn] > 0.f) ? v[j] : 0.f;
    }
    float u1[kJ];
#pragma unroll
    for (int j = 0; j < kJ; ++j) u1[j] = Mj[j] * h1[j];
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
      const float ajj = (adj[j * kJ + j] + adj2[j * kJ + j]);        // diagonal of (a + a^T) / 2
      const float u0 = Mj[j] * h0[j];
      float z = fmaf(ajj, u0, bias), ub = 0.f;
#pragma unroll
      for (int i = 0; i < kJ; ++i)
        if (i != j) {
          z = fmaf(A[j * kJ + i], u1[i], z);
          ub = fmaf(A[j * kJ + i], v[i], ub);                          // u1bar[j] / c
        }
      bacc += v[j];
      gacc = fmaf(v[j], (z - mean) * rstd, gacc);
      const float zb = c * v[j];
      macc[j] += (ajj * zb) * h0[j] + (c * ub) * h1[j];
      dacc[j] = fmaf(zb, u0, dacc[j]);
      Zs[j * LDT + tid] = zb;
      Us[j * LDT + tid] = u1[j];
    }
    __syncthreads();
    // Abar[3 jb + a][3 ib + e] += sum over this k-group's 64 channels
    for (int k = kg * 64; k < kg * 64 + 64; k += 4) {
      f32x4 zr[3], ur[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        zr[a] = *(const f32x4*)(Zs + (3 * jb + a) * LDT + k);
        ur[a] = *(const f32x4*)(Us + (3 * ib + a) * LDT + k);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int e = 0; e < 3; ++e) acc[a][e] = fmaf(zr[a][q], ur[e][q], acc[a][e]);
    }
    __syncthreads();
  }

  if (live) {
#pragma unroll
    for (int j = 0; j < kJ; ++j) p.Mpart[((size_t)grp * kJ + j) * N + n] = macc[j];
    p.bpart[(size_t)grp * N + n] = bacc;
    p.gpart[(size_t)grp * N + n] = gacc;
  }
  // the four k-groups' blocks and the lanes' diagonal terms, added in index order
  float* red = Zs;                                   // [4][576] floats <= 24 * LDT
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int e = 0; e < 3; ++e) red[kg * (kJ * kJ) + (3 * jb + a) * kJ + 3 * ib + e] = acc[a][e];
#pragma unroll
  for (int j = 0; j < kJ; ++j) Us[j * LDT + tid] = dacc[j];
  __syncthreads();
  float* out = p.Apart + (size_t)blockIdx.x * (kJ * kJ);
  for (int e = tid; e < kJ * kJ; e += NT) {
    if (e / kJ == e % kJ) continue;
    out[e] = ((red[e] + red[kJ * kJ + e]) + red[2 * kJ * kJ + e]) + red[3 * kJ * kJ + e];
  }
  if (tid < kJ) {
    float s = 0.f;
    for (int k = 0; k < NT; ++k) s += Us[tid * LDT + k];
    out[tid * kJ + tid] = s;
  }
}

struct FinishArgs {
  const float* Mpart; const float* bpart; const float* gpart; const float* Apart;
  ehm_gconv_params raw;
  int N, bn, groups, chunks;
  float* gM; float* gadj2; float* gbias; float* gbn_weight; float* gbn_bias;
};

// sum of n floats `stride` apart, in index order; the loads go out 16 at a time (one after the other they cost a memory latency each)
__device__ __forceinline__ double strided_sum(const float* __restrict__ p, size_t stride, int n) {
  double s = 0.0;
  int g = 0;
  for (; g + 16 <= n; g += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = p[(size_t)(g + u) * stride];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += (double)v[u];
  }
  for (; g < n; ++g) s += (double)p[(size_t)g * stride];
  return s;
}

__global__ __launch_bounds__(256) void gcn_bwd_params_finish(FinishArgs p) {
  const int t = blockIdx.x * 256 + threadIdx.x, N = p.N;
  if (t < kJ * N) p.gM[t] = (float)strided_sum(p.Mpart + t, (size_t)kJ * N, p.groups);
  if (t < N) {
    const double sb = strided_sum(p.bpart + t, N, p.groups);
    double c = 1.0;
    if (p.bn) {
      c = (double)p.raw.bn_weight[t] * (double)(1.f / sqrtf(p.raw.bn_var[t] + 1e-5f));
      p.gbn_weight[t] = (float)strided_sum(p.gpart + t, N, p.groups);
      p.gbn_bias[t] = (float)sb;
    }
    p.gbias[t] = (float)(c * sb);
  }
  // the adjacency entries on the LAST blocks (the first ones carry all three kinds of work otherwise)
  const int ta = ((int)gridDim.x - 1 - (int)blockIdx.x) * 256 + threadIdx.x;
  if (ta < kJ * kJ) {
    const int j = ta / kJ, i = ta % kJ;
    const double s = strided_sum(p.Apart + ta, kJ * kJ, p.groups * p.chunks), st = strided_sum(p.Apart + i * kJ + j, kJ * kJ, p.groups * p.chunks);
    p.gadj2[ta] = (float)((s + st) * 0.5);
  }
}

// the handle's conv `conv` (EHM_GCN_CONV_INPUT, a hidden conv's index, EHM_GCN_CONV_OUTPUT)
int conv_of(const ehm_gcn* h, int conv, BwdConv* c) {
  EHM_CHECK_ARG(h && (conv == EHM_GCN_CONV_INPUT || conv == EHM_GCN_CONV_OUTPUT || (conv >= 0 && conv < h->num_hidden)));
  c->adj = h->adj;
  if (conv == EHM_GCN_CONV_OUTPUT) {
    c->T0 = c->T1 = h->out.M;
    c->A = h->out.A;
    c->raw = h->raw_out;
    c->N = 6; c->bn = 0; c->out = 1;
  } else {
    const LayerDev& L = conv == EHM_GCN_CONV_INPUT ? h->input : h->hidden[conv];
    c->T0 = L.D; c->T1 = L.M1; c->A = L.Aoff;
    c->raw = conv == EHM_GCN_CONV_INPUT ? h->raw_input : h->raw_hidden[conv];
    c->N = L.N; c->bn = L.relu; c->out = 0;
  }
  EHM_CHECK_ARG(c->adj && c->raw.M && c->raw.adj2);
  return 0;
}

int param_groups(int bodies) { return bodies < kMaxGroups ? bodies : kMaxGroups; }

int64_t param_floats(int N, int bodies) {
  const int64_t groups = param_groups(bodies), chunks = ceil_div(N, NT);
  return groups * ((int64_t)kJ * N + 2 * N) + groups * chunks * kJ * kJ;
}

}  // namespace

extern "C" int ehm_gcn_bwd_epilogue(const ehm_gcn* h, int conv, const float* gout, const float* gate, float* G, int ldg, int bodies,
                                    void* stream) {
  BwdConv c;
  const int rc = conv_of(h, conv, &c);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(gout && G && bodies > 0 && ldg >= 2 * c.N);
  EHM_CHECK_ARG(c.bn ? gate != nullptr : gate == nullptr);     // the gate exists exactly where the conv has a ReLU
  EHM_CHECK_ARG((const void*)gout != (const void*)G && (const void*)gate != (const void*)G);
  const long long total = (long long)bodies * c.N;
  EHM_CHECK_ARG(ceil_div(total, 256) < (1ll << 31));
  const dim3 grid((unsigned)ceil_div(total, 256));
  if (c.out) hipLaunchKernelGGL(gcn_bwd_epilogue_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, gout, gate, c.T0, c.T1, c.A, G, c.N, ldg, total);
  else hipLaunchKernelGGL(gcn_bwd_epilogue_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, gout, gate, c.T0, c.T1, c.A, G, c.N, ldg, total);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_gcn_bwd_params_workspace_bytes(const ehm_gcn* h, int conv, int bodies, int64_t* bytes) {
  BwdConv c;
  const int rc = conv_of(h, conv, &c);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(bytes && bodies > 0);
  *bytes = param_floats(c.N, bodies) * (int64_t)sizeof(float);
  return 0;
}

extern "C" int ehm_gcn_bwd_params(const ehm_gcn* h, int conv, const float* gout, const float* gate, const float* pre, int ld_pre, int bodies,
                                  float* gM, float* gadj2, float* gbias, float* gbn_weight, float* gbn_bias, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  BwdConv c;
  const int rc = conv_of(h, conv, &c);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(gout && pre && bodies > 0 && ld_pre >= 2 * c.N && gM && gadj2 && gbias && workspace);
  EHM_CHECK_ARG(c.bn ? (gate && gbn_weight && gbn_bias && c.raw.bn_weight && c.raw.bn_mean && c.raw.bn_var) : (!gate && !gbn_weight && !gbn_bias));
  EHM_CHECK_ARG(workspace_bytes >= param_floats(c.N, bodies) * (int64_t)sizeof(float) && (uintptr_t)workspace % 4 == 0);
  ParamArgs a;
  a.gout = gout; a.gate = gate; a.pre = pre;
  a.c = c;
  a.ld_pre = ld_pre; a.bodies = bodies;
  a.groups = param_groups(bodies);
  a.chunks = (int)ceil_div(c.N, NT);
  float* w = (float*)workspace;
  a.Mpart = w;  w += (size_t)a.groups * kJ * c.N;
  a.bpart = w;  w += (size_t)a.groups * c.N;
  a.gpart = w;  w += (size_t)a.groups * c.N;
  a.Apart = w;
  hipLaunchKernelGGL(gcn_bwd_params_kernel, dim3((unsigned)(a.groups * a.chunks)), dim3(NT), 0, (hipStream_t)stream, a);
  FinishArgs f;
  f.Mpart = a.Mpart; f.bpart = a.bpart; f.gpart = a.gpart; f.Apart = a.Apart;
  f.raw = c.raw;
  f.N = c.N; f.bn = c.bn; f.groups = a.groups; f.chunks = a.chunks;
  f.gM = gM; f.gadj2 = gadj2; f.gbias = gbias; f.gbn_weight = gbn_weight; f.gbn_bias = gbn_bias;
  const int items = kJ * c.N > kJ * kJ ? kJ * c.N : kJ * kJ;
  hipLaunchKernelGGL(gcn_bwd_params_finish, dim3((unsigned)ceil_div(items, 256)), dim3(256), 0, (hipStream_t)stream, f);
  EHM_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------- train-mode BatchNorm (gcn_train.hip)
// Behind ehm_gcn_train_bn_backward a BatchNorm'd conv's backward is the output conv's algebra on its own M and N: zbar = the cotangent, no gate, T0 = T1 = M,
// the full symmetrised adjacency A of ehm_gcn_train_adjacency.  The OUT instantiations above run unchanged (the parameter kernel's bias / BatchNorm sums
// come out unused: the bias gradient is zero on this route and the BatchNorm ones are ehm_gcn_train_bn_backward's).
namespace {

int train_conv_of(const ehm_gcn* h, int conv, const float* A, BwdConv* c) {
  EHM_CHECK_ARG(h && (conv == EHM_GCN_CONV_INPUT || (conv >= 0 && conv < h->num_hidden)));
  c->raw = conv == EHM_GCN_CONV_INPUT ? h->raw_input : h->raw_hidden[conv];
  c->adj = h->adj;
  c->T0 = c->T1 = c->raw.M;
  c->A = A;
  c->N = c->raw.out_dim; c->bn = 0; c->out = 1;
  EHM_CHECK_ARG(c->adj && c->raw.M && c->raw.adj2 && c->N > 0);
  return 0;
}

// workspace of ehm_gcn_train_bwd_params: the unused bias sums [N] | ehm_gcn_bwd_params' partial sums
int64_t train_param_floats(int N, int bodies) { return N + param_floats(N, bodies); }

}  // namespace

extern "C" int ehm_gcn_train_bwd_epilogue(const ehm_gcn* h, int conv, const float* zbar, const float* A, float* G, int ldg, int bodies, void* stream) {
  BwdConv c;
  const int rc = train_conv_of(h, conv, A, &c);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(zbar && G && A && bodies > 0 && ldg >= 2 * c.N && (const void*)zbar != (const void*)G);
  const long long total = (long long)bodies * c.N;
  EHM_CHECK_ARG(ceil_div(total, 256) < (1ll << 31));
  hipLaunchKernelGGL(gcn_bwd_epilogue_kernel<true>, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, zbar, (const float*)nullptr,
                     c.T0, c.T1, c.A, G, c.N, ldg, total);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_gcn_train_bwd_params_workspace_bytes(const ehm_gcn* h, int conv, int bodies, int64_t* bytes) {
  BwdConv c;
  const int rc = train_conv_of(h, conv, nullptr, &c);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(bytes && bodies > 0);
  *bytes = train_param_floats(c.N, bodies) * (int64_t)sizeof(float);
  return 0;
}

extern "C" int ehm_gcn_train_bwd_params(const ehm_gcn* h, int conv, const float* zbar, const float* A, const float* pre, int ld_pre, int bodies, float* gM,
                                        float* gadj2, void* workspace, int64_t workspace_bytes, void* stream) {
  BwdConv c;
  const int rc = train_conv_of(h, conv, A, &c);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(zbar && A && pre && bodies > 0 && ld_pre >= 2 * c.N && gM && gadj2 && workspace);
  EHM_CHECK_ARG(workspace_bytes >= train_param_floats(c.N, bodies) * (int64_t)sizeof(float) && (uintptr_t)workspace % 4 == 0);
  float* w = (float*)workspace;
  float* gbias = w;  w += c.N;       // sum zbar: zero up to rounding (the batch mean removes the bias), not handed out
  ParamArgs a;
  a.gout = zbar; a.gate = nullptr; a.pre = pre;
  a.c = c;
  a.ld_pre = ld_pre; a.bodies = bodies;
  a.groups = param_groups(bodies);
  a.chunks = (int)ceil_div(c.N, NT);
  a.Mpart = w;  w += (size_t)a.groups * kJ * c.N;
  a.bpart = w;  w += (size_t)a.groups * c.N;
  a.gpart = w;  w += (size_t)a.groups * c.N;
  a.Apart = w;
  hipLaunchKernelGGL(gcn_bwd_params_kernel, dim3((unsigned)(a.groups * a.chunks)), dim3(NT), 0, (hipStream_t)stream, a);
  FinishArgs f;
  f.Mpart = a.Mpart; f.bpart = a.bpart; f.gpart = a.gpart; f.Apart = a.Apart;
  f.raw = c.raw;
  f.N = c.N; f.bn = 0; f.groups = a.groups; f.chunks = a.chunks;
  f.gM = gM; f.gadj2 = gadj2; f.gbias = gbias; f.gbn_weight = nullptr; f.gbn_bias = nullptr;
  const int items = kJ * c.N > kJ * kJ ? kJ * c.N : kJ * kJ;
  hipLaunchKernelGGL(gcn_bwd_params_finish, dim3((unsigned)ceil_div(items, 256)), dim3(256), 0, (hipStream_t)stream, f);
  EHM_LAUNCH_CHECK();
  return 0;
}
