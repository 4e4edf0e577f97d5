// Vector-Jacobian product of the non-local block's joint attention for gfx950 (MI355X): the one step of the block's backward that is not a GEMM or a
// BatchNorm sum.  The forward it differentiates (nonlocal_attention_kernel, csrc/linear.hip):
//   NONLocalBlock2D.forward        models/egohmr/modulated_gcn/nets/non_local_embedded_gaussian.py:68-79
//   ModulatedGCN.forward           models/egohmr/modulated_gcn/modulated_gcn.py:104-110 (the block on the joint axis)
//
// Per body, with theta, phi, g [24, Ci] and ybar the cotangent of y = P g, P = softmax(theta phi^T, dim = -1):
//   Pbar = ybar g^T,   D_a = sum_b P_ab Pbar_ab,   Fbar = P (.) (Pbar - D)          (the softmax's Jacobian on the logits F = theta phi^T)
//   thetabar = Fbar phi,   phibar = Fbar^T theta,   gbar = P^T ybar
//
//   nonlocal_attention_bwd_kernel   one block per body, so no sum crosses a block.  Pass 1 accumulates the 24 x 24 logits and Pbar over 64-channel slabs
//                                   of theta, phi, g, ybar staged in LDS (the forward's slab loop and summation order: P has the forward's bits); 24 lanes
//                                   then take the softmax with the max-subtraction, D and Fbar.  Pass 2: one lane = one channel of one of the three outputs,
//                                   its 24 input values in registers against a 24 x 24 matrix in LDS (Fbar, Fbar^T or P^T).  Every element is read
//                                   once per pass: HBM / L2 bound.
//   nonlocal_bn_residual_kernel     the block's tail on the autograd routes, out = BatchNorm2d(u) + x with given statistics (element-wise, HBM bound).
// No atomics, every sum in index order: two calls on the same inputs give the same bits.
#include "common.h"
#include "egohmr_hip.h"

namespace {

constexpr int kSlab = 64;           // channels staged per step of pass 1
constexpr int kPairs = kJ * kJ;     // 576 (query joint, key joint) pairs: three per lane

__global__ __launch_bounds__(256) void nonlocal_attention_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ gy,
                                                                     float* __restrict__ gqkv, int Ci) {
  __shared__ float sT[kJ][kSlab + 1], sP[kJ][kSlab + 1], sG[kJ][kSlab + 1], sY[kJ][kSlab + 1];
  __shared__ float sF[kJ][kJ + 1], sB[kJ][kJ + 1];      // logits -> P;  Pbar -> Fbar
  __shared__ float sM[3][kJ][kJ + 1];                   // pass 2: out[i] = sum_j sM[t][i][j] in[j]  (Fbar, Fbar^T, P^T)
  const int tid = threadIdx.x;
  const size_t row0 = (size_t)blockIdx.x * kJ;
  const size_t ld = 3 * (size_t)Ci;
  float f[3] = {0.f, 0.f, 0.f}, pb[3] = {0.f, 0.f, 0.f};      // pairs tid, tid + 256, tid + 512 (< 576)
  for (int c0 = 0; c0 < Ci; c0 += kSlab) {
    for (int i = tid; i < kJ * kSlab; i += 256) {
      const int j = i >> 6, c = i & 63;
      const bool ok = c0 + c < Ci;                            // the ragged last slab: zeros add nothing
      const float* q = qkv + (row0 + j) * ld + c0 + c;
      sT[j][c] = ok ? q[0] : 0.f;
      sP[j][c] = ok ? q[Ci] : 0.f;
      sG[j][c] = ok ? q[2 * (size_t)Ci] : 0.f;
      sY[j][c] = ok ? gy[(row0 + j) * Ci + c0 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int pr = tid + 256 * k;
      if (pr < kPairs) {
        const int a = pr / kJ, b = pr % kJ;
        float s = f[k], p = pb[k];
        for (int c = 0; c < kSlab; ++c) {
          s = fmaf(sT[a][c], sP[b][c], s);
          p = fmaf(sY[a][c], sG[b][c], p);
        }
        f[k] = s;
        pb[k] = p;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int pr = tid + 256 * k;
    if (pr < kPairs) {
      sF[pr / kJ][pr % kJ] = f[k];
      sB[pr / kJ][pr % kJ] = pb[k];
    }
  }
  __syncthreads();
  if (tid < kJ) {                                     // one lane = one query joint: softmax over the key joints, D, Fbar
    float m = -3.4e38f;
    for (int b = 0; b < kJ; ++b) m = fmaxf(m, sF[tid][b]);
    float z = 0.f;
    for (int b = 0; b < kJ; ++b) { const float e = expf(sF[tid][b] - m); sF[tid][b] = e; z += e; }
    const float inv = 1.f / z;
    float d = 0.f;
    for (int b = 0; b < kJ; ++b) {
      const float p = sF[tid][b] * inv;
      sF[tid][b] = p;
      d = fmaf(p, sB[tid][b], d);
    }
    for (int b = 0; b < kJ; ++b) {
      const float p = sF[tid][b], fb = p * (sB[tid][b] - d);
      sM[0][tid][b] = fb;
      sM[1][b][tid] = fb;
      sM[2][b][tid] = p;
    }
  }
  __syncthreads();
  for (int i = tid; i < 3 * Ci; i += 256) {           // column i of gqkv: t = 0 thetabar <- phi, 1 phibar <- theta, 2 gbar <- ybar
    const int t = i / Ci, c = i - t * Ci;
    const float* in = t == 0 ? qkv + row0 * ld + Ci + c : t == 1 ? qkv + row0 * ld + c : gy + row0 * Ci + c;
    const size_t lin = t == 2 ? (size_t)Ci : ld;
    float v[kJ];
#pragma unroll
    for (int j = 0; j < kJ; ++j) v[j] = in[(size_t)j * lin];
    float* o = gqkv + row0 * ld + i;
#pragma unroll 2
    for (int r = 0; r < kJ; ++r) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < kJ; ++j) s = fmaf(sM[t][r][j], v[j], s);
      o[(size_t)r * ld] = s;
    }
  }
}

// The block's tail on float32 rows (non_local_embedded_gaussian.py:81-82): out = BatchNorm(u) + x with the statistics given (the batch's, or the running
// ones), unfolded - the backward needs u itself, so the autograd route cannot use the inference route's folded GEMM.
__global__ __launch_bounds__(256) void nonlocal_bn_residual_kernel(const float* __restrict__ u, const float* __restrict__ mean,
                                                                   const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, const float* __restrict__ res,
                                                                   float* __restrict__ out, long long total, int C) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  out[i] = fmaf((u[i] - mean[c]) * invstd[c], gamma[c], beta[c]) + res[i];
}

}  // namespace

extern "C" int ehm_nonlocal_bn_residual(const float* u, const float* mean, const float* invstd, const float* gamma, const float* beta, const float* res,
                                        float* out, int64_t rows, int C, void* stream) {
  EHM_CHECK_ARG(u && mean && invstd && gamma && beta && res && out);
  EHM_CHECK_ARG(rows > 0 && C > 0 && rows < (1ll << 31) && ceil_div(rows * C, 256) < (1ll << 31));
  hipLaunchKernelGGL(nonlocal_bn_residual_kernel, dim3((unsigned)ceil_div(rows * C, 256)), dim3(256), 0, (hipStream_t)stream, u, mean, invstd, gamma,
                     beta, res, out, (long long)rows * C, C);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_nonlocal_attention_backward(const float* qkv, const float* gy, float* gqkv, int64_t bodies, int Ci, void* stream) {
  EHM_CHECK_ARG(qkv && gy && gqkv);
  EHM_CHECK_ARG(bodies > 0 && bodies < (1ll << 31));
  EHM_CHECK_ARG(Ci > 0 && Ci <= (1 << 24));
  hipLaunchKernelGGL(nonlocal_attention_bwd_kernel, dim3((unsigned)bodies), dim3(256), 0, (hipStream_t)stream, qkv, gy, gqkv, Ci);
  EHM_LAUNCH_CHECK();
  return 0;
}
