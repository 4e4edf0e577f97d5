// Device-side view of the SMPL constants, shared by smpl.hip (forward) and guidance.hip (backward).
#pragma once
#include <stddef.h>

#include "common.h"

constexpr int kBG = 8;       // bodies per block of the skinning VJP (guidance.hip)
constexpr int kBGF = 16;     // bodies per block of the forward skinning kernel: halves the L2 re-reads of the 17 MB pose basis
constexpr int kVT = 256;     // vertices per skinning block
constexpr int kPoseBasis = 207;

struct Tree {
  int8_t parent[kJ];
  int8_t depth[kJ];
  int max_depth;
};

struct SmplDev {
  int V;
  int n_extra;
  float* v_template;   // [V*3]
  float* shape_t;      // [10][V*3]   shapedirs transposed (basis-major like posedirs)
  const float* posedirs;  // [207][V*3] caller-owned (smplx layout already streams well)
  float* w_t;          // [24][V]     lbs_weights transposed
  int sparse4;         // 1 when every vertex has <= 4 non-zero skinning weights (true for SMPL): use w_idx / w_val
  int32_t* w_idx;      // [4][V]      joint ids of the non-zero weights (padding: joint 0 with weight 0)
  float* w_val;        // [4][V]
  float* J_template;   // [24][3]     J_regressor . v_template
  float* J_shape;      // [24][3][10] J_regressor . shapedirs
  int32_t* extra_idx;  // [n_extra]
  // blend basis [posedirs; shapedirs] (K = 207 + 10 -> 224) as split-f16 MFMA B fragments (skin_mfma_kernel):
  // PDf[vertex tile of 32][k-step of 16][coord][hi/lo][lane][8 halves], values x pd_scale (power of two)
  const void* PDf;
  float pd_scale;
  Tree tree;
};

constexpr int kBlendK = 224;          // 207 pose-corrective + 10 shape coefficients, padded to 14 MFMA k-steps of 16
constexpr int kBlendSteps = kBlendK / 16;


static __device__ __forceinline__ void rot6d_to_R(float a1x, float a1y, float a1z, float a2x, float a2y, float a2z, float (&R)[9]) {
  // utils/geometry.py:61-66; F.normalize = x / max(||x||_2, 1e-12).  Every product / sum is rounded separately
  // (no FMA contraction) like the eager torch ops, so the cancellation in a2 - (b1.a2) b1 for nearly parallel
  // a1, a2 behaves as in the reference.
  const float n1 = fmaxf(sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(a1x, a1x), __fmul_rn(a1y, a1y)), __fmul_rn(a1z, a1z))), 1e-12f);
  const float b1x = __fdiv_rn(a1x, n1), b1y = __fdiv_rn(a1y, n1), b1z = __fdiv_rn(a1z, n1);
  const float d = __fadd_rn(__fadd_rn(__fmul_rn(b1x, a2x), __fmul_rn(b1y, a2y)), __fmul_rn(b1z, a2z));
  const float ux = __fsub_rn(a2x, __fmul_rn(d, b1x)), uy = __fsub_rn(a2y, __fmul_rn(d, b1y)), uz = __fsub_rn(a2z, __fmul_rn(d, b1z));
  const float n2 = fmaxf(sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(ux, ux), __fmul_rn(uy, uy)), __fmul_rn(uz, uz))), 1e-12f);
  const float b2x = __fdiv_rn(ux, n2), b2y = __fdiv_rn(uy, n2), b2z = __fdiv_rn(uz, n2);
  const float b3x = __fsub_rn(__fmul_rn(b1y, b2z), __fmul_rn(b1z, b2y));
  const float b3y = __fsub_rn(__fmul_rn(b1z, b2x), __fmul_rn(b1x, b2z));
  const float b3z = __fsub_rn(__fmul_rn(b1x, b2y), __fmul_rn(b1y, b2x));
  R[0] = b1x; R[1] = b2x; R[2] = b3x;
  R[3] = b1y; R[4] = b2y; R[5] = b3y;
  R[6] = b1z; R[7] = b2z; R[8] = b3z;
}

// VJP of R = rot6d_to_rotmat(a1, a2) (utils/geometry.py:59-66): gR [9] row-major -> (ga1, ga2)
static __device__ __forceinline__ void rot6d_bwd(float a1x, float a1y, float a1z, float a2x, float a2y, float a2z, const float (&gR)[9],
                                                 float (&ga1)[3], float (&ga2)[3]) {
  const float n1r = sqrtf(a1x * a1x + a1y * a1y + a1z * a1z), n1 = fmaxf(n1r, 1e-12f);
  const float b1[3] = {a1x / n1, a1y / n1, a1z / n1};
  const float a2[3] = {a2x, a2y, a2z};
  const float d = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
  const float u[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
  const float n2r = sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), n2 = fmaxf(n2r, 1e-12f);
  const float b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
  float g1[3] = {gR[0], gR[3], gR[6]}, g2[3] = {gR[1], gR[4], gR[7]};
  const float g3[3] = {gR[2], gR[5], gR[8]};
  // b3 = b1 x b2
  g1[0] += b2[1] * g3[2] - b2[2] * g3[1]; g1[1] += b2[2] * g3[0] - b2[0] * g3[2]; g1[2] += b2[0] * g3[1] - b2[1] * g3[0];
  g2[0] += g3[1] * b1[2] - g3[2] * b1[1]; g2[1] += g3[2] * b1[0] - g3[0] * b1[2]; g2[2] += g3[0] * b1[1] - g3[1] * b1[0];
  // b2 = u / max(|u|, eps); like clamp_min's backward, the gradient takes the |u| path where |u| >= eps (ties included)
  float gu[3];
  if (n2r >= 1e-12f) {
    const float t = b2[0] * g2[0] + b2[1] * g2[1] + b2[2] * g2[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) gu[c] = (g2[c] - b2[c] * t) / n2;
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) gu[c] = g2[c] / n2;
  }
  // u = a2 - (b1.a2) b1
  const float gub1 = gu[0] * b1[0] + gu[1] * b1[1] + gu[2] * b1[2];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    ga2[c] = gu[c] - gub1 * b1[c];
    g1[c] += -d * gu[c] - gub1 * a2[c];
  }
  // b1 = a1 / max(|a1|, eps), the same tie rule
  if (n1r >= 1e-12f) {
    const float t = b1[0] * g1[0] + b1[1] * g1[1] + b1[2] * g1[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) ga1[c] = (g1[c] - b1[c] * t) / n1;
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) ga1[c] = g1[c] / n1;
  }
}


struct ehm_smpl {
  SmplDev d{};
  float* arena = nullptr;      // packed constants
  float* ws = nullptr;         // per-call scratch: R [cap,24,9] + A [cap,24,12] (+ backward scratch)
  int ws_cap = 0;
  void* pdf = nullptr;         // SmplDev::PDf storage
  void* pf = nullptr;          // blend coefficients of the current batch as MFMA A fragments [ceil(B/32)][14][hi/lo][64][8 halves]
  int pf_cap = 0;              // bodies
  int32_t* coll_faces = nullptr;   // ehm_smpl_set_collision_mesh: the handle's own device copy of the faces [coll_F,3], or nullptr (vertex proxy)
  int coll_F = 0;
};
// tests/test_smpl_autograd_cpu.py hands the argument checks of ehm_smpl_backward a host stand-in for a handle that holds V and n_extra only:
// the two ints lead the handle.  Moving them fails the build here, not the test in host code that reads garbage.
static_assert(offsetof(ehm_smpl, d) == 0 && offsetof(SmplDev, V) == 0 && offsetof(SmplDev, n_extra) == sizeof(int),
              "ehm_smpl must start with SmplDev{int V; int n_extra; ...}");
