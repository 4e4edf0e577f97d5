// Evaluation block of the reference's driver on gfx950 (test_egohmr.py:399-494) and the axis-angle conversion of the
// COAP / VolSMPL call sites (utils/konia_transform.py:316-340, called at models/egohmr/egohmr.py:495, :540).
//
//   rotmat_to_angle_axis (+ VJP)   one thread per 3 x 3 matrix: rotation_matrix_to_quaternion's four branches (:349-443) and quaternion_to_angle_axis
//                                  (:560-630) in registers; the VJP differentiates the branch the forward took (what autograd does through torch.where)
//   point_errors                   one 256-thread block per (item, sample): |pred - gt| per point (optionally origin-aligned), mean over the points,
//                                  sums over the visible / invisible points (G-MPJPE :399-407, MPJPE :409-417, V2V :441-449)
//   procrustes                     one thread per (item, sample), float64 in registers as the reference's numpy loop (utils/pose_utils.py:10-66): centred
//                                  24 x 3 clouds, K = X1^T X2, 3 x 3 SVD by one-sided Jacobi, R = V Z U^T, scale, translation -> per-joint error :419-437
//   procrustes_vis                 the same solve on clouds whose invisible joints are zeroed (pose_utils.py:75-107, --eval_with_vis_mask_pa), any J
//   diversity                      one wave per item, lane = joint: unbiased std over the samples and the pairwise-distance sum (:453-494), masked means
//
// These are latency-bound reductions over a few MB (the largest, V2V at B x S = 1280 bodies, reads 106 MB once: HBM-bound, ~25 us at 5 TB/s); what the
// reference does with them is dozens of eager ops + a per-sample numpy SVD loop on the CPU with a device -> host copy in front.
#include "common.h"
#include "egohmr_hip.h"
#include "procrustes_solve.h"

namespace {

constexpr float kEps = 1.0e-6f;   // konia_transform.py: eps of rotation_matrix_to_quaternion / quaternion_to_angle_axis / safe_zero_division

__device__ __forceinline__ float safe_div(float num, float den) {   // konia_transform.py:343-346
  if (fabsf(den) < kEps) den += kEps;
  return num / den;
}

// branch: 0 = trace > 0; 1, 2, 3 = the x / y / z leading cases.  lead = the clamped radicand's argument, n0..n2 = the three numerators in quaternion
// order with the leading component left out.
struct QuatBranch { int br; float lead, n[3]; };

__device__ __forceinline__ QuatBranch quat_branch(const float* m) {
  const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
  const float trace = m00 + m11 + m22;
  QuatBranch b;
  if (trace > 0.f) { b.br = 0; b.lead = trace + 1.f; b.n[0] = m21 - m12; b.n[1] = m02 - m20; b.n[2] = m10 - m01; }                       // (w) x y z
  else if (m00 > m11 && m00 > m22) { b.br = 1; b.lead = 1.f + m00 - m11 - m22; b.n[0] = m21 - m12; b.n[1] = m01 + m10; b.n[2] = m02 + m20; }   // w (x) y z
  else if (m11 > m22) { b.br = 2; b.lead = 1.f + m11 - m00 - m22; b.n[0] = m02 - m20; b.n[1] = m01 + m10; b.n[2] = m12 + m21; }              // w x (y) z
  else { b.br = 3; b.lead = 1.f + m22 - m00 - m11; b.n[0] = m10 - m01; b.n[1] = m02 + m20; b.n[2] = m12 + m21; }                           // w x y (z)
  return b;
}

// q = (w, x, y, z) from a branch
__device__ __forceinline__ void quat_of(const QuatBranch& b, float& sq, float* q) {
  sq = sqrtf(fmaxf(b.lead, kEps)) * 2.f;
  const float lead = 0.25f * sq;
  const float a = safe_div(b.n[0], sq), c = safe_div(b.n[1], sq), d = safe_div(b.n[2], sq);
  switch (b.br) {
    case 0: q[0] = lead; q[1] = a; q[2] = c; q[3] = d; break;
    case 1: q[0] = a; q[1] = lead; q[2] = c; q[3] = d; break;
    case 2: q[0] = a; q[1] = c; q[2] = lead; q[3] = d; break;
    default: q[0] = a; q[1] = c; q[2] = d; q[3] = lead; break;
  }
}

__device__ __forceinline__ float safe_atan2(float y, float x) {   // konia_transform.py:44-47
  if (fabsf(y) < kEps && fabsf(x) < kEps) y += kEps;
  return atan2f(y, x);
}

__global__ void rotmat_to_aa_kernel(const float* __restrict__ R, float* __restrict__ aa, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = R[i * 9 + k];
  float sq, q[4];
  quat_of(quat_branch(m), sq, q);
  const float s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const float sn = sqrtf(fmaxf(s2, kEps));
  const float two_theta = 2.f * (q[0] < 0.f ? safe_atan2(-sn, -q[0]) : safe_atan2(sn, q[0]));
  const float k = s2 > 0.f ? safe_div(two_theta, sn) : 2.f;
  aa[i * 3 + 0] = q[1] * k; aa[i * 3 + 1] = q[2] * k; aa[i * 3 + 2] = q[3] * k;
}

__global__ void rotmat_to_aa_bwd_kernel(const float* __restrict__ R, const float* __restrict__ gaa, float* __restrict__ gR, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = R[i * 9 + k];
  const QuatBranch b = quat_branch(m);
  float sq, q[4];
  quat_of(b, sq, q);
  const float g0 = gaa[i * 3 + 0], g1 = gaa[i * 3 + 1], g2 = gaa[i * 3 + 2];
  // ---- aa = (x, y, z) k(w, sn(x, y, z))
  const float s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const float sn = sqrtf(fmaxf(s2, kEps));
  float gq[4] = {0.f, 0.f, 0.f, 0.f};
  if (s2 > 0.f) {
    const float w = q[0];
    const float two_theta = 2.f * (w < 0.f ? safe_atan2(-sn, -w) : safe_atan2(sn, w));
    float den = sn;
    if (fabsf(den) < kEps) den += kEps;
    const float k = two_theta / den;
    const float gk = g0 * q[1] + g1 * q[2] + g2 * q[3];
    const float r2 = sn * sn + w * w;
    // atan2(+-sn, +-w): d/dsn = w / r2, d/dw = -sn / r2 in both sign branches
    const float dk_dsn = (2.f * w / r2) / den - two_theta / (den * den);
    const float dk_dw = (-2.f * sn / r2) / den;
    const float gsn = gk * dk_dsn;
    gq[0] = gk * dk_dw;
    const float dsn = s2 > kEps ? 1.f / sn : 0.f;            // sqrt(clamp_min(s2, eps)): the clamp passes no gradient below eps
    gq[1] = g0 * k + gsn * q[1] * dsn;
    gq[2] = g1 * k + gsn * q[2] * dsn;
    gq[3] = g2 * k + gsn * q[3] * dsn;
  } else {
    gq[1] = 2.f * g0; gq[2] = 2.f * g1; gq[3] = 2.f * g2;
  }
  // ---- q from (lead, n0, n1, n2): leading component sq / 4, the others n_j / sq (sq >= 2e-3: safe_div's guard never fires)
  float gn[3], glead_q;
  switch (b.br) {
    case 0: glead_q = gq[0]; gn[0] = gq[1]; gn[1] = gq[2]; gn[2] = gq[3]; break;
    case 1: glead_q = gq[1]; gn[0] = gq[0]; gn[1] = gq[2]; gn[2] = gq[3]; break;
    case 2: glead_q = gq[2]; gn[0] = gq[0]; gn[1] = gq[1]; gn[2] = gq[3]; break;
    default: glead_q = gq[3]; gn[0] = gq[0]; gn[1] = gq[1]; gn[2] = gq[2]; break;
  }
  float gsq = 0.25f * glead_q;
#pragma unroll
  for (int j = 0; j < 3; ++j) { gsq -= gn[j] * b.n[j] / (sq * sq); gn[j] /= sq; }
  const float glead = b.lead >= kEps ? gsq * 2.f / sq : 0.f;   // sq = 2 sqrt(clamp_min(lead, eps))
  float g[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // index: m00 0, m01 1, m02 2, m10 3, m11 4, m12 5, m20 6, m21 7, m22 8
  switch (b.br) {
    case 0: g[0] += glead; g[4] += glead; g[8] += glead;
            g[7] += gn[0]; g[5] -= gn[0]; g[2] += gn[1]; g[6] -= gn[1]; g[3] += gn[2]; g[1] -= gn[2]; break;
    case 1: g[0] += glead; g[4] -= glead; g[8] -= glead;
            g[7] += gn[0]; g[5] -= gn[0]; g[1] += gn[1]; g[3] += gn[1]; g[2] += gn[2]; g[6] += gn[2]; break;
    case 2: g[4] += glead; g[0] -= glead; g[8] -= glead;
            g[2] += gn[0]; g[6] -= gn[0]; g[1] += gn[1]; g[3] += gn[1]; g[5] += gn[2]; g[7] += gn[2]; break;
    default: g[8] += glead; g[0] -= glead; g[4] -= glead;
            g[3] += gn[0]; g[1] -= gn[0]; g[2] += gn[1]; g[6] += gn[1]; g[5] += gn[2]; g[7] += gn[2]; break;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) gR[i * 9 + k] = g[k];
}

// ------------------------------------------------------------------------------------------------ point errors
__device__ __forceinline__ float block_sum_256(float v, float* red) {   // 4 waves; every thread returns the block's sum
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void point_errors_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ opred,
                                                           const float* __restrict__ ogt, const uint8_t* __restrict__ mask, float* __restrict__ per_point,
                                                           float* __restrict__ mean, float* __restrict__ vis_sum, float* __restrict__ invis_sum, int S, int P,
                                                           int pred_stride, int gt_stride, int origin_point) {
  __shared__ float red[4];
  const int bs = blockIdx.x, b = bs / S, tid = threadIdx.x;
  const float* p = pred + (size_t)bs * pred_stride * 3;
  const float* g = gt + (size_t)b * gt_stride * 3;
  float op[3] = {0.f, 0.f, 0.f}, og[3] = {0.f, 0.f, 0.f};
  if (opred) { op[0] = opred[(size_t)bs * 3]; op[1] = opred[(size_t)bs * 3 + 1]; op[2] = opred[(size_t)bs * 3 + 2]; }
  if (ogt) { og[0] = ogt[(size_t)b * 3]; og[1] = ogt[(size_t)b * 3 + 1]; og[2] = ogt[(size_t)b * 3 + 2]; }
  if (origin_point >= 0) {                                   // each cloud's own point `origin_point` (the pelvis, test_egohmr.py:409: joint 0)
    for (int c = 0; c < 3; ++c) { op[c] = p[3 * origin_point + c]; og[c] = g[3 * origin_point + c]; }
  }
  float s_all = 0.f, s_vis = 0.f;
  for (int i = tid; i < P; i += 256) {
    const float dx = (p[3 * i] - op[0]) - (g[3 * i] - og[0]), dy = (p[3 * i + 1] - op[1]) - (g[3 * i + 1] - og[1]), dz = (p[3 * i + 2] - op[2]) - (g[3 * i + 2] - og[2]);
    const float e = sqrtf(dx * dx + dy * dy + dz * dz);
    if (per_point) per_point[(size_t)bs * P + i] = e;
    s_all += e;
    if (mask && mask[(size_t)b * P + i]) s_vis += e;
  }
  s_all = block_sum_256(s_all, red);
  s_vis = block_sum_256(s_vis, red);
  if (tid == 0) {
    mean[bs] = s_all / (float)P;
    if (vis_sum) vis_sum[bs] = mask ? s_vis : s_all;
    if (invis_sum) invis_sum[bs] = mask ? s_all - s_vis : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ Procrustes
// The solve (3 x 3 Jacobi SVD, R = V Z U^T, scale, translation) is csrc/procrustes_solve.h, shared with tools/procrustes_check.cpp.
__global__ __launch_bounds__(64) void procrustes_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const uint8_t* __restrict__ mask,
                                                        float* __restrict__ aligned, float* __restrict__ per_joint, float* __restrict__ mean,
                                                        float* __restrict__ vis_sum, float* __restrict__ invis_sum, int n, int S, int J) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int b = i / S;
  const float* p = pred + (size_t)i * J * 3;
  const float* g = gt + (size_t)b * J * 3;
  double mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0};
  for (int j = 0; j < J; ++j)
    for (int c = 0; c < 3; ++c) { mu1[c] += (double)p[3 * j + c]; mu2[c] += (double)g[3 * j + c]; }
  for (int c = 0; c < 3; ++c) { mu1[c] /= J; mu2[c] /= J; }
  double K[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var1 = 0.0;
  for (int j = 0; j < J; ++j) {
    double x1[3], x2[3];
    for (int c = 0; c < 3; ++c) { x1[c] = (double)p[3 * j + c] - mu1[c]; x2[c] = (double)g[3 * j + c] - mu2[c]; var1 += x1[c] * x1[c]; }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) K[r][c] += x1[r] * x2[c];                  // K = X1 X2^T in the reference's 3 x N layout (pose_utils.py:36)
  }
  double Rm[3][3], scale, t[3];
  procrustes_solve::similarity(K, var1, mu1, mu2, Rm, &scale, t);
  double s_all = 0.0, s_vis = 0.0;
  for (int j = 0; j < J; ++j) {
    double e2 = 0.0;
    for (int r = 0; r < 3; ++r) {
      const double h = scale * (Rm[r][0] * (double)p[3 * j] + Rm[r][1] * (double)p[3 * j + 1] + Rm[r][2] * (double)p[3 * j + 2]) + t[r];
      if (aligned) aligned[((size_t)i * J + j) * 3 + r] = (float)h;
      const double d = h - (double)g[3 * j + r];
      e2 += d * d;
    }
    const double e = sqrt(e2);
    if (per_joint) per_joint[(size_t)i * J + j] = (float)e;
    s_all += e;
    if (mask && mask[(size_t)b * J + j]) s_vis += e;
  }
  if (mean) mean[i] = (float)(s_all / J);
  if (vis_sum) vis_sum[i] = (float)(mask ? s_vis : s_all);
  if (invis_sum) invis_sum[i] = (float)(mask ? s_all - s_vis : 0.0);
}

// The --eval_with_vis_mask_pa alignment (utils/pose_utils.py:75-107): the same float64 solve as procrustes_kernel on MASKED copies of both clouds - an
// invisible joint is multiplied by 0, i.e. it stays in the means over all J as a point at the origin - and the similarity applied to the unmasked
// prediction.  Three passes over the J joints in global memory (means, K / var1, errors): no per-joint arrays, so J is not bounded.
__global__ __launch_bounds__(64) void procrustes_vis_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const uint8_t* __restrict__ amask,
                                                            float* __restrict__ aligned, float* __restrict__ per_joint, float* __restrict__ mean,
                                                            float* __restrict__ vis_sum, float* __restrict__ invis_sum, int n, int S, int J) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int b = i / S;
  const float* p = pred + (size_t)i * J * 3;
  const float* g = gt + (size_t)b * J * 3;
  const uint8_t* m = amask + (size_t)b * J;
  double mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0};
  for (int j = 0; j < J; ++j) {
    const double w = m[j] ? 1.0 : 0.0;
    for (int c = 0; c < 3; ++c) { mu1[c] += w * (double)p[3 * j + c]; mu2[c] += w * (double)g[3 * j + c]; }
  }
  for (int c = 0; c < 3; ++c) { mu1[c] /= J; mu2[c] /= J; }
  double K[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var1 = 0.0;
  for (int j = 0; j < J; ++j) {
    const double w = m[j] ? 1.0 : 0.0;
    double x1[3], x2[3];
    for (int c = 0; c < 3; ++c) { x1[c] = w * (double)p[3 * j + c] - mu1[c]; x2[c] = w * (double)g[3 * j + c] - mu2[c]; var1 += x1[c] * x1[c]; }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) K[r][c] += x1[r] * x2[c];
  }
  double Rm[3][3], scale, t[3];
  procrustes_solve::similarity(K, var1, mu1, mu2, Rm, &scale, t);   // no visible joint: var1 = 0, scale = 0 / 0 = NaN, as the reference
  double s_all = 0.0, s_vis = 0.0, s_inv = 0.0;
  for (int j = 0; j < J; ++j) {
    double e2 = 0.0;
    for (int r = 0; r < 3; ++r) {
      const double h = scale * (Rm[r][0] * (double)p[3 * j] + Rm[r][1] * (double)p[3 * j + 1] + Rm[r][2] * (double)p[3 * j + 2]) + t[r];
      if (aligned) aligned[((size_t)i * J + j) * 3 + r] = (float)h;
      const double d = h - (double)g[3 * j + r];
      e2 += d * d;
    }
    const double e = sqrt(e2), w = m[j] ? 1.0 : 0.0;
    if (per_joint) per_joint[(size_t)i * J + j] = (float)e;
    s_all += e;
    s_vis += e * w;                                                          // products, not a branch: a NaN error reaches both sums (test_egohmr.py:433-436)
    s_inv += e * (1.0 - w);
  }
  if (mean) mean[i] = (float)(s_all / J);
  if (vis_sum) vis_sum[i] = (float)s_vis;
  if (invis_sum) invis_sum[i] = (float)s_inv;
}

// ------------------------------------------------------------------------------------------------ diversity
__global__ __launch_bounds__(64) void diversity_kernel(const float* __restrict__ joints, const uint8_t* __restrict__ mask, int invert, float* __restrict__ std_out,
                                                       float* __restrict__ apd_out, int S, int J) {
  const int b = blockIdx.x, j = threadIdx.x;
  const float* a = joints + (size_t)b * S * J * 3;
  float sd = 0.f, pd = 0.f, sel = 0.f;
  if (j < J) {
    bool on = true;
    if (mask) on = (mask[(size_t)b * J + j] != 0) != (invert != 0);
    sel = on ? 1.f : 0.f;
    // unbiased std over the samples per coordinate (two passes), mean over the three coordinates (test_egohmr.py:453-455)
    float mu[3] = {0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s)
      for (int c = 0; c < 3; ++c) mu[c] += a[((size_t)s * J + j) * 3 + c];
    for (int c = 0; c < 3; ++c) mu[c] /= (float)S;
    float var[3] = {0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s)
      for (int c = 0; c < 3; ++c) { const float d = a[((size_t)s * J + j) * 3 + c] - mu[c]; var[c] += d * d; }
    sd = (sqrtf(var[0] / (float)(S - 1)) + sqrtf(var[1] / (float)(S - 1)) + sqrtf(var[2] / (float)(S - 1))) / 3.f;      // (S = 1: 0 / 0 = NaN, as torch.std)
    // sum over ORDERED sample pairs of the joint distance (:471-476)
    for (int s = 0; s < S; ++s)
      for (int t = s + 1; t < S; ++t) {
        const float* u = a + ((size_t)s * J + j) * 3;
        const float* v = a + ((size_t)t * J + j) * 3;
        const float dx = u[0] - v[0], dy = u[1] - v[1], dz = u[2] - v[2];
        pd += 2.f * sqrtf(dx * dx + dy * dy + dz * dz);
      }
  }
  const float cnt = wave_sum(sel);
  const float ssd = wave_sum(sel > 0.f ? sd : 0.f), spd = wave_sum(sel > 0.f ? pd : 0.f);
  if (j == 0) {
    if (std_out) std_out[b] = ssd / cnt;                                        // no selected joint: 0 / 0 = NaN like the reference's empty mean
    if (apd_out) apd_out[b] = spd / cnt / (float)S / (float)(S - 1) / 2.f;
  }
}

}  // namespace

extern "C" int ehm_rotmat_to_angle_axis(const float* R, float* aa, int64_t n, void* stream) {
  EHM_CHECK_ARG(R && aa && n >= 0);
  if (n == 0) return 0;
  hipLaunchKernelGGL(rotmat_to_aa_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, R, aa, n);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_rotmat_to_angle_axis_bwd(const float* R, const float* gaa, float* gR, int64_t n, void* stream) {
  EHM_CHECK_ARG(R && gaa && gR && n >= 0);
  if (n == 0) return 0;
  hipLaunchKernelGGL(rotmat_to_aa_bwd_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, R, gaa, gR, n);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_eval_point_errors(const ehm_eval_points_desc* d, void* stream) {
  EHM_CHECK_ARG(d && d->pred && d->gt && d->mean && d->B > 0 && d->S > 0 && d->P > 0);
  EHM_CHECK_ARG(d->pred_points >= d->P && d->gt_points >= d->P && d->origin_point < d->P);
  EHM_CHECK_ARG(d->origin_point < 0 || (!d->pred_origin && !d->gt_origin));
  hipLaunchKernelGGL(point_errors_kernel, dim3((unsigned)(d->B * d->S)), dim3(256), 0, (hipStream_t)stream, d->pred, d->gt, d->pred_origin, d->gt_origin, d->mask,
                     d->per_point, d->mean, d->vis_sum, d->invis_sum, d->S, d->P, d->pred_points, d->gt_points, d->origin_point);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_eval_procrustes(const float* pred, const float* gt, const uint8_t* mask, float* aligned, float* per_joint, float* mean, float* vis_sum,
                                   float* invis_sum, int B, int S, int J, void* stream) {
  EHM_CHECK_ARG(pred && gt && B > 0 && S > 0 && J >= 3 && (aligned || per_joint || mean));   // any J: the kernel has no J-sized array
  EHM_CHECK_ARG((int64_t)B * S <= INT32_MAX);
  const int n = B * S;
  hipLaunchKernelGGL(procrustes_kernel, dim3((unsigned)ceil_div(n, 64)), dim3(64), 0, (hipStream_t)stream, pred, gt, mask, aligned, per_joint, mean, vis_sum,
                     invis_sum, n, S, J);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_eval_procrustes_vis(const float* pred, const float* gt, const uint8_t* align_mask, float* aligned, float* per_joint, float* mean,
                                       float* vis_sum, float* invis_sum, int B, int S, int J, void* stream) {
  EHM_CHECK_ARG(pred && gt && align_mask && B > 0 && S > 0 && J >= 1 && (aligned || per_joint || mean));
  EHM_CHECK_ARG((int64_t)B * S <= INT32_MAX);
  const int n = B * S;
  hipLaunchKernelGGL(procrustes_vis_kernel, dim3((unsigned)ceil_div(n, 64)), dim3(64), 0, (hipStream_t)stream, pred, gt, align_mask, aligned, per_joint, mean,
                     vis_sum, invis_sum, n, S, J);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_eval_diversity(const float* joints, const uint8_t* mask, int invert, float* std_out, float* apd_out, int B, int S, int J, void* stream) {
  EHM_CHECK_ARG(joints && (std_out || apd_out) && B > 0 && S > 0 && J > 0 && J <= 64);
  hipLaunchKernelGGL(diversity_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, joints, mask, invert, std_out, apd_out, S, J);
  EHM_LAUNCH_CHECK();
  return 0;
}
