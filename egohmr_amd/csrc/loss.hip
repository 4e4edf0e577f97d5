// Validation losses of EgoHMR.compute_loss on gfx950: models/egohmr/egohmr.py:307-449 in the evaluation branch (self.training == False), with
// models/egohmr/losses.py:20-25 (Keypoint2DLoss), :44-50 (Keypoint3DLoss), :86-88 (ParameterLoss).  include/egohmr_hip.h lists the terms and their lines.
//
//   v2v_partial_kernel   the only term with traffic: B V 3 floats of prediction + the same of ONE ground truth per item (male or female by gender[b]; the
//                        other array is never touched).  An item's 3 V floats are cut into 16-byte pieces of the FLAT array (an item starts at float
//                        3 V b, which is 16-byte aligned only for every fourth item when V is odd): up to 3 head and 3 tail floats go to block 0 of the item
//                        as scalars, the aligned middle as float4 loads, 4 per thread and array, all issued before the first use.  One block = 4096
//                        floats of an item (6 blocks per 6890-vertex body: 1536 blocks at B = 256); its float64 sum goes to one slot of the slab.
//   item_terms_kernel    one wave per item: the joint / parameter terms (a few hundred floats), the item's slab slots added in index order, the
//                        per-item row in float64 (workspace) and float32 (per_item)
//   batch_reduce_kernel  one block: the B per-item float64 rows added in a fixed order -> the eleven batch scalars and the visible-joint count
//   scene_cap_kernel     the point cap of the penetration term (:406-412), see ehm_scene_cap_points
//   v2v_grad_kernel, item_grad_kernel   the VJP of the total (ehm_val_losses_backward), at the end of this file
//
// Every element is widened to float64 before the first subtraction and every sum is a float64 sum in a fixed order - no atomics, so two runs give the same
// bits.  Memory bound: 2 x 82.7 KB per 6890-vertex item (42 MB at B = 256, 5 us at 8 TB/s); the float64 work is 5 flops per loaded float.
#include "common.h"
#include "egohmr_hip.h"

namespace {

constexpr int kTerms = EHM_LOSS_TERMS;
constexpr int kQuadsPerThread = 4;                       // float4 loads per thread and array
constexpr int kQuadsPerBlock = 256 * kQuadsPerThread;    // 4096 floats of an item per block
__constant__ int kSmplToOpenpose[25] = {24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34};   // egohmr.py:108-109

__device__ __forceinline__ double wave_sum_f64(double v) {   // fixed butterfly: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__host__ __device__ inline int v2v_blocks(int V) {        // blocks per item: the aligned middle has at most 3 V / 4 quads
  const int q = (3 * V) / 4;
  return q < kQuadsPerBlock ? 1 : (q + kQuadsPerBlock - 1) / kQuadsPerBlock;
}

__global__ __launch_bounds__(256) void v2v_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt_m, const float* __restrict__ gt_f,
                                                          const float* __restrict__ pred_j, const float* __restrict__ j_m, const float* __restrict__ j_f,
                                                          const int64_t* __restrict__ gender, double* __restrict__ slab, int V, int pred_joints,
                                                          int gt_joints, int nblk) {
  __shared__ double red[4];
  const int b = blockIdx.x / nblk, x = blockIdx.x - b * nblk, tid = threadIdx.x;
  const bool fem = gender[b] == 1;                                            // egohmr.py:350-351
  const float* __restrict__ gt = fem ? gt_f : gt_m;
  const float* gj = (fem ? j_f : j_m) + (size_t)b * gt_joints * 3;
  const float* pj = pred_j + (size_t)b * pred_joints * 3;
  double pp[3], gp[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { pp[c] = (double)pj[c]; gp[c] = (double)gj[c]; }
  const int64_t start = (int64_t)b * V * 3, end = start + (int64_t)V * 3;
  int64_t a0 = (start + 3) / 4 * 4, a1 = end / 4 * 4;                         // aligned middle [a0, a1) of the flat arrays
  if (a0 > end) a0 = end;
  if (a1 < a0) a1 = a0;
  double acc = 0.0;
  if (x == 0 && tid < 6) {                                                    // head [start, a0) and tail [a1, end): at most 3 floats each
    const int64_t i = tid < 3 ? start + tid : a1 + (tid - 3);
    if (tid < 3 ? i < a0 : i < end) {
      const int c = (int)((i - start) % 3);
      acc = fabs(((double)pred[i] - pp[c]) - ((double)gt[i] - gp[c]));
    }
  }
  const int64_t q0 = a0 / 4 + (int64_t)x * kQuadsPerBlock + tid, qend = a1 / 4;
  f32x4 P[kQuadsPerThread], G[kQuadsPerThread];
#pragma unroll
  for (int u = 0; u < kQuadsPerThread; ++u) {
    const int64_t q = q0 + 256 * u;
    if (q < qend) {
      P[u] = *reinterpret_cast<const f32x4*>(pred + q * 4);
      G[u] = *reinterpret_cast<const f32x4*>(gt + q * 4);
    }
  }
#pragma unroll
  for (int u = 0; u < kQuadsPerThread; ++u) {
    const int64_t q = q0 + 256 * u;
    if (q < qend) {
      int c = (int)((q * 4 - start) % 3);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double po = c == 0 ? pp[0] : (c == 1 ? pp[1] : pp[2]), go = c == 0 ? gp[0] : (c == 1 ? gp[1] : gp[2]);
        acc += fabs(((double)P[u][i] - po) - ((double)G[u][i] - go));
        c = c == 2 ? 0 : c + 1;
      }
    }
  }
  acc = wave_sum_f64(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) slab[(size_t)b * nblk + x] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct ItemArgs {
  const float *pred_j, *pred_jf, *pred_2d, *pred_go, *pred_bp, *pred_betas, *pred_6d;
  const float *kp2d, *kp3d, *kp3d_full, *j_m, *j_f;
  const int64_t* gender;
  const float *gt_go, *gt_bp, *gt_betas, *focal, *center, *penetration;
  double w[9];
  const double* slab;
  double* item64;
  float* per_item;
  int64_t* per_item_vis;
  uint8_t* vis_mask;
  int V, pred_joints, gt_joints, kp3d_points, kp3d_full_points, kp2d_points, nblk;
};

__global__ __launch_bounds__(64) void item_terms_kernel(const ItemArgs a) {
  const int b = blockIdx.x, j = threadIdx.x;
  const bool fem = a.gender[b] == 1;
  const float* pj = a.pred_j + (size_t)b * a.pred_joints * 3;
  const float* pf = a.pred_jf + (size_t)b * a.pred_joints * 3;
  const float* p2 = a.pred_2d + (size_t)b * a.pred_joints * 2;
  const float* g3 = a.kp3d + (size_t)b * a.kp3d_points * 3;
  const float* gf = a.kp3d_full + (size_t)b * a.kp3d_full_points * 3;
  const float* g2 = a.kp2d + (size_t)b * a.kp2d_points * 3;
  const float* gj = (fem ? a.j_f : a.j_m) + (size_t)b * a.gt_joints * 3;
  double kp3d = 0.0, kp3d_full = 0.0, kp2d = 0.0, betas = 0.0, bp = 0.0, go = 0.0, ortho = 0.0, vis_err = 0.0;
  int visible = 0;
  if (j < 24) {
    double e2 = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double d = ((double)pj[3 * j + c] - (double)pj[c]) - ((double)g3[3 * j + c] - (double)g3[c]);   // losses.py:47-48, egohmr.py:360-361
      kp3d += fabs(d);
      e2 += d * d;
      kp3d_full += fabs((double)pf[3 * j + c] - (double)gf[3 * j + c]);
    }
    // utils/geometry.py:78-116 with zero translation and identity rotation: p / p_z, then K p
    const double X = (double)gj[3 * j], Y = (double)gj[3 * j + 1], Z = (double)gj[3 * j + 2];
    const double u = (double)a.focal[2 * b] * (X / Z) + (double)a.center[2 * b] * (Z / Z);
    const double v = (double)a.focal[2 * b + 1] * (Y / Z) + (double)a.center[2 * b + 1] * (Z / Z);
    visible = (u >= 0.0 && u < 1920.0 && v >= 0.0 && v < 1080.0) ? 1 : 0;                                  // :368-369
    vis_err = sqrt(e2) * (double)visible;                                                                 // :370 - a product, not a selection
    if (a.vis_mask) a.vis_mask[(size_t)b * 24 + j] = (uint8_t)visible;
    const float* x = a.pred_6d + (size_t)b * 144 + 6 * j;                                                  // :386-387, x[r][c] = x[2 r + c]
    const double x00 = x[0], x01 = x[1], x10 = x[2], x11 = x[3], x20 = x[4], x21 = x[5];
    const double m00 = x00 * x00 + x10 * x10 + x20 * x20 - 1.0, m11 = x01 * x01 + x11 * x11 + x21 * x21 - 1.0, m01 = x00 * x01 + x10 * x11 + x20 * x21;
    ortho = m00 * m00 + m11 * m11 + 2.0 * (m01 * m01);
  }
  if (j < 25) {
    const double conf = (j == 1 || j == 9 || j == 12) ? 0.0 : (double)g2[3 * j + 2];                        // losses.py:22-23
    const int s = kSmplToOpenpose[j];
    kp2d = conf * fabs((double)p2[2 * s] - (double)g2[3 * j]) + conf * fabs((double)p2[2 * s + 1] - (double)g2[3 * j + 1]);
  }
  if (j < 10) { const double d = (double)a.pred_betas[(size_t)b * 10 + j] - (double)a.gt_betas[(size_t)b * 10 + j]; betas = d * d; }
  if (j < 9) { const double d = (double)a.pred_go[(size_t)b * 9 + j] - (double)a.gt_go[(size_t)b * 9 + j]; go = d * d; }
  for (int i = j; i < 207; i += 64) { const double d = (double)a.pred_bp[(size_t)b * 207 + i] - (double)a.gt_bp[(size_t)b * 207 + i]; bp += d * d; }
  kp3d = wave_sum_f64(kp3d); kp3d_full = wave_sum_f64(kp3d_full); kp2d = wave_sum_f64(kp2d); betas = wave_sum_f64(betas); bp = wave_sum_f64(bp);
  go = wave_sum_f64(go); ortho = wave_sum_f64(ortho); vis_err = wave_sum_f64(vis_err);
  const int nvis = __popcll(__ballot(visible != 0));
  if (j == 0) {
    double v2v = 0.0;
    for (int x = 0; x < a.nblk; ++x) v2v += a.slab[(size_t)b * a.nblk + x];
    double t[kTerms];
    t[EHM_LOSS_V2V] = v2v / (3.0 * (double)a.V);
    t[EHM_LOSS_KP3D] = kp3d; t[EHM_LOSS_KP3D_FULL] = kp3d_full; t[EHM_LOSS_KP2D_FULL] = kp2d;
    t[EHM_LOSS_BETAS] = betas; t[EHM_LOSS_BODY_POSE] = bp; t[EHM_LOSS_GLOBAL_ORIENT] = go;
    t[EHM_LOSS_POSE_6D_ORTHO] = ortho / 96.0;
    t[EHM_LOSS_PENETRATION] = a.penetration ? (double)a.penetration[b] : 0.0;
    t[EHM_LOSS_KP3D_VIS_SUM] = vis_err;
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) tot += a.w[k] * t[1 + k];                                                 // :422-430
    t[EHM_LOSS_TOTAL] = tot;
#pragma unroll
    for (int k = 0; k < kTerms; ++k) {
      a.item64[(size_t)b * kTerms + k] = t[k];
      a.per_item[(size_t)b * kTerms + k] = (float)t[k];
    }
    a.per_item_vis[b] = nvis;
  }
}

struct BatchArgs { double w[9]; };

__global__ __launch_bounds__(256) void batch_reduce_kernel(const double* __restrict__ item64, const int64_t* __restrict__ per_item_vis, const BatchArgs w,
                                                           float* __restrict__ losses, int64_t* __restrict__ joint_vis_num, int B) {
  __shared__ double red[256];
  __shared__ double total[kTerms];
  __shared__ long long cnt[256];
  const int tid = threadIdx.x;
  for (int k = 1; k < kTerms; ++k) {
    double s = 0.0;
    for (int i = tid; i < B; i += 256) s += item64[(size_t)i * kTerms + k];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) total[k] = k == EHM_LOSS_KP3D_VIS_SUM ? red[0] : red[0] / (double)B;
    __syncthreads();
  }
  long long c = 0;
  for (int i = tid; i < B; i += 256) c += per_item_vis[i];
  cnt[tid] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) cnt[tid] += cnt[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    double tot = 0.0;
    for (int k = 0; k < 9; ++k) tot += w.w[k] * total[1 + k];
    losses[EHM_LOSS_TOTAL] = (float)tot;
    for (int k = 1; k < kTerms; ++k) losses[k] = (float)total[k];
    *joint_vis_num = cnt[0];
  }
}

// egohmr.py:406-412.  The box is the one bbox_kernel (guidance.hip) finds: float32 min / max, NaN vertices ignored.
__global__ __launch_bounds__(256) void scene_cap_kernel(const float* __restrict__ verts, const float* __restrict__ scene, float* __restrict__ out,
                                                        int* __restrict__ count, int V, int N, int cap) {
  __shared__ float red[6][256];
  __shared__ int n_in;
  const int b = blockIdx.x, tid = threadIdx.x;
  float lo[3] = {3.4e38f, 3.4e38f, 3.4e38f}, hi[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
  for (int v = tid; v < V; v += 256) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float x = verts[((size_t)b * V + v) * 3 + c];
      lo[c] = fminf(lo[c], x);
      hi[c] = fmaxf(hi[c], x);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { red[c][tid] = lo[c]; red[3 + c][tid] = hi[c]; }
  if (tid == 0) n_in = 0;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        red[c][tid] = fminf(red[c][tid], red[c][tid + o]);
        red[3 + c][tid] = fmaxf(red[3 + c][tid], red[3 + c][tid + o]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { lo[c] = red[c][0]; hi[c] = red[3 + c][0]; }
  const float* s = scene + (size_t)b * N * 3;
  float* o = out + (size_t)b * N * 3;
  int mine = 0;
  for (int i = tid; i < N; i += 256) {
    const float x = s[3 * i], y = s[3 * i + 1], z = s[3 * i + 2];
    mine += (x >= lo[0] && x <= hi[0] && y >= lo[1] && y <= hi[1] && z >= lo[2] && z <= hi[2]) ? 1 : 0;
  }
  atomicAdd(&n_in, mine);                                                    // (integer, in LDS: order-independent)
  __syncthreads();
  const int n = n_in;
  if (tid == 0) count[b] = n;
  const bool capped = n > cap;                                               // :411-412: inds[:, 4000:] = False
  for (int i = tid; i < N; i += 256) {
    const bool drop = capped && i >= cap;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[3 * i + c] = drop ? 3.0e38f : s[3 * i + c];
  }
}

int64_t workspace_bytes(int B, int V) { return ((int64_t)B * v2v_blocks(V) + (int64_t)B * kTerms) * (int64_t)sizeof(double); }

}  // namespace

extern "C" int ehm_val_losses_workspace_bytes(int B, int V, int64_t* bytes) {
  EHM_CHECK_ARG(B >= 1 && V >= 1 && bytes);
  *bytes = workspace_bytes(B, V);
  return 0;
}

extern "C" int ehm_val_losses(const ehm_val_losses_desc* d, void* stream) {
  EHM_CHECK_ARG(d != nullptr);
  EHM_CHECK_ARG(d->B >= 1 && d->V >= 1);
  EHM_CHECK_ARG((int64_t)d->B * d->V * 3 < ((int64_t)1 << 40) && (int64_t)d->B * v2v_blocks(d->V) <= INT32_MAX);
  EHM_CHECK_ARG(d->pred_joints >= 45 && d->gt_joints >= 24 && d->kp3d_points >= 24 && d->kp3d_full_points >= 24 && d->kp2d_points >= 25);
  EHM_CHECK_ARG(d->pred_vertices && d->pred_keypoints_3d && d->pred_keypoints_3d_full && d->pred_keypoints_2d_full);
  EHM_CHECK_ARG(d->pred_global_orient && d->pred_body_pose && d->pred_betas && d->pred_pose_6d);
  EHM_CHECK_ARG(d->keypoints_2d && d->keypoints_3d && d->keypoints_3d_full);
  EHM_CHECK_ARG(d->gt_vertices_male && d->gt_vertices_female && d->gt_joints_male && d->gt_joints_female && d->gender);
  EHM_CHECK_ARG(d->gt_global_orient && d->gt_body_pose && d->gt_betas && d->focal && d->center);
  EHM_CHECK_ARG(d->losses && d->joint_vis_num && d->per_item && d->per_item_vis);
  EHM_CHECK_ARG(((uintptr_t)d->pred_vertices & 15) == 0 && ((uintptr_t)d->gt_vertices_male & 15) == 0 && ((uintptr_t)d->gt_vertices_female & 15) == 0);
  EHM_CHECK_ARG(d->workspace && ((uintptr_t)d->workspace & 7) == 0 && d->workspace_bytes >= workspace_bytes(d->B, d->V));
  const hipStream_t st = (hipStream_t)stream;
  const int nblk = v2v_blocks(d->V);
  double* slab = (double*)d->workspace;
  double* item64 = slab + (size_t)d->B * nblk;
  hipLaunchKernelGGL(v2v_partial_kernel, dim3((unsigned)(d->B * nblk)), dim3(256), 0, st, d->pred_vertices, d->gt_vertices_male, d->gt_vertices_female,
                     d->pred_keypoints_3d, d->gt_joints_male, d->gt_joints_female, d->gender, slab, d->V, d->pred_joints, d->gt_joints, nblk);
  ItemArgs a;
  a.pred_j = d->pred_keypoints_3d; a.pred_jf = d->pred_keypoints_3d_full; a.pred_2d = d->pred_keypoints_2d_full;
  a.pred_go = d->pred_global_orient; a.pred_bp = d->pred_body_pose; a.pred_betas = d->pred_betas; a.pred_6d = d->pred_pose_6d;
  a.kp2d = d->keypoints_2d; a.kp3d = d->keypoints_3d; a.kp3d_full = d->keypoints_3d_full; a.j_m = d->gt_joints_male; a.j_f = d->gt_joints_female;
  a.gender = d->gender; a.gt_go = d->gt_global_orient; a.gt_bp = d->gt_body_pose; a.gt_betas = d->gt_betas;
  a.focal = d->focal; a.center = d->center; a.penetration = d->penetration;
  BatchArgs w;
  for (int k = 0; k < 9; ++k) a.w[k] = w.w[k] = d->weights[k];
  a.slab = slab; a.item64 = item64; a.per_item = d->per_item; a.per_item_vis = d->per_item_vis; a.vis_mask = d->vis_mask;
  a.V = d->V; a.pred_joints = d->pred_joints; a.gt_joints = d->gt_joints; a.kp3d_points = d->kp3d_points; a.kp3d_full_points = d->kp3d_full_points;
  a.kp2d_points = d->kp2d_points; a.nblk = nblk;
  hipLaunchKernelGGL(item_terms_kernel, dim3((unsigned)d->B), dim3(64), 0, st, a);
  hipLaunchKernelGGL(batch_reduce_kernel, dim3(1), dim3(256), 0, st, (const double*)item64, (const int64_t*)d->per_item_vis, w, d->losses,
                     d->joint_vis_num, d->B);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_scene_cap_points(const float* verts, const float* scene, float* scene_out, int32_t* count, int B, int V, int N, int cap,
                                    void* stream) {
  EHM_CHECK_ARG(verts && scene && scene_out && count && B >= 1 && V >= 1 && N >= 1 && cap >= 0);
  hipLaunchKernelGGL(scene_cap_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, verts, scene, scene_out, count, V, N, cap);
  EHM_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------ the VJP of losses[EHM_LOSS_TOTAL]
//   v2v_grad_kernel    v2v_partial_kernel's cut of the flat vertex array (head / tail scalars in block 0 of the item, the aligned middle as float4, 4 per
//                      thread and array, all loads before the first use): d in float64 in the forward's expression order, g = s_0 / (3 V) sign(d) stored
//                      as float4; the block's integer sums of sign(d) per component and its NaN flags go to one 16-byte slot of the workspace
//   item_grad_kernel   one wave per item: every other array, and the pelvis joint's three sources (its own KP3D sign, -s_1 sum_j sign, -s_0 / (3 V) sum_v
//                      sign from the item's slots in index order) added in float64 and rounded once
// Integer sign sums are exact in any order, no float atomics: two calls give the same bits.  Memory bound: 2 reads + 1 write of 4 B V 3 bytes.
namespace {

__device__ __forceinline__ double sign_f64(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : (d == 0.0 ? 0.0 : d)); }   // torch.sign; NaN stays NaN

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// d -> its gradient element; adds sign(d) to the thread's integer sum of component c (a NaN sets the component's flag instead)
__device__ __forceinline__ float v2v_grad_elem(double d, double cv, int c, int (&sum)[3], int& nan_bits) {
  const double s = sign_f64(d);
  if (s != s) nan_bits |= 1 << c;
  else { const int k = (int)s; sum[0] += c == 0 ? k : 0; sum[1] += c == 1 ? k : 0; sum[2] += c == 2 ? k : 0; }
  return (float)(cv * s);
}

__global__ __launch_bounds__(256) void v2v_grad_kernel(const float* __restrict__ pred, const float* __restrict__ gt_m, const float* __restrict__ gt_f,
                                                       const float* __restrict__ pred_j, const float* __restrict__ j_m, const float* __restrict__ j_f,
                                                       const int64_t* __restrict__ gender, const float* __restrict__ gloss, double w0,
                                                       float* __restrict__ g_pred, int* __restrict__ slots, int B, int V, int pred_joints, int gt_joints,
                                                       int nblk) {
  __shared__ int red[4][4];
  const int b = blockIdx.x / nblk, x = blockIdx.x - b * nblk, tid = threadIdx.x;
  const bool fem = gender[b] == 1;
  const float* __restrict__ gt = fem ? gt_f : gt_m;
  const float* gj = (fem ? j_f : j_m) + (size_t)b * gt_joints * 3;
  const float* pj = pred_j + (size_t)b * pred_joints * 3;
  double pp[3], gp[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { pp[c] = (double)pj[c]; gp[c] = (double)gj[c]; }
  const double cv = ((gloss ? (double)*gloss : 1.0) * w0 / (double)B) / (3.0 * (double)V);
  const int64_t start = (int64_t)b * V * 3, end = start + (int64_t)V * 3;
  int64_t a0 = (start + 3) / 4 * 4, a1 = end / 4 * 4;                         // the forward's cut: aligned middle [a0, a1) of the flat arrays
  if (a0 > end) a0 = end;
  if (a1 < a0) a1 = a0;
  int sum[3] = {0, 0, 0}, nan_bits = 0;
  if (x == 0 && tid < 6) {                                                    // head [start, a0) and tail [a1, end)
    const int64_t i = tid < 3 ? start + tid : a1 + (tid - 3);
    if (tid < 3 ? i < a0 : i < end) {
      const int c = (int)((i - start) % 3);
      const float g = v2v_grad_elem(((double)pred[i] - pp[c]) - ((double)gt[i] - gp[c]), cv, c, sum, nan_bits);
      if (g_pred) g_pred[i] = g;
    }
  }
  const int64_t q0 = a0 / 4 + (int64_t)x * kQuadsPerBlock + tid, qend = a1 / 4;
  f32x4 P[kQuadsPerThread], G[kQuadsPerThread];
#pragma unroll
  for (int u = 0; u < kQuadsPerThread; ++u) {
    const int64_t q = q0 + 256 * u;
    if (q < qend) {
      P[u] = *reinterpret_cast<const f32x4*>(pred + q * 4);
      G[u] = *reinterpret_cast<const f32x4*>(gt + q * 4);
    }
  }
#pragma unroll
  for (int u = 0; u < kQuadsPerThread; ++u) {
    const int64_t q = q0 + 256 * u;
    if (q < qend) {
      int c = (int)((q * 4 - start) % 3);
      f32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double po = c == 0 ? pp[0] : (c == 1 ? pp[1] : pp[2]), go = c == 0 ? gp[0] : (c == 1 ? gp[1] : gp[2]);
        o[i] = v2v_grad_elem(((double)P[u][i] - po) - ((double)G[u][i] - go), cv, c, sum, nan_bits);
        c = c == 2 ? 0 : c + 1;
      }
      if (g_pred) *reinterpret_cast<f32x4*>(g_pred + q * 4) = o;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) sum[c] = wave_sum_i32(sum[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nan_bits |= __shfl_xor(nan_bits, o);
  if ((tid & 63) == 0) { red[tid >> 6][0] = sum[0]; red[tid >> 6][1] = sum[1]; red[tid >> 6][2] = sum[2]; red[tid >> 6][3] = nan_bits; }
  __syncthreads();
  if (tid < 4) {
    const int v = tid < 3 ? red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid] : (red[0][3] | red[1][3] | red[2][3] | red[3][3]);
    slots[((size_t)b * nblk + x) * 4 + tid] = v;
  }
}

struct ItemGradArgs {
  const float *pred_j, *pred_jf, *pred_2d, *pred_go, *pred_bp, *pred_betas, *pred_6d;
  const float *kp2d, *kp3d, *kp3d_full;
  const float *gt_go, *gt_bp, *gt_betas, *gloss;
  double w[9];
  const int* slots;           // NULL: the vertex pass did not run (g_pj not asked for)
  float *g_pj, *g_pjf, *g_p2, *g_go, *g_bp, *g_betas, *g_6d, *g_pen;
  int B, V, pred_joints, kp3d_points, kp3d_full_points, kp2d_points, nblk;
};

__global__ __launch_bounds__(64) void item_grad_kernel(const ItemGradArgs a) {
  __shared__ double sg[24 * 3];
  const int b = blockIdx.x, j = threadIdx.x;
  const double gl = a.gloss ? (double)*a.gloss : 1.0;
  double s[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = gl * a.w[k] / (double)a.B;
  if (a.g_pj) {
    const float* pj = a.pred_j + (size_t)b * a.pred_joints * 3;
    const float* g3 = a.kp3d + (size_t)b * a.kp3d_points * 3;
    double sj[3] = {0.0, 0.0, 0.0};
    if (j < 24) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        sj[c] = sign_f64(((double)pj[3 * j + c] - (double)pj[c]) - ((double)g3[3 * j + c] - (double)g3[c]));   // the forward's expression
        sg[3 * j + c] = sj[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) sj[c] = wave_sum_f64(sj[c]);        // small integers: exact; a NaN comes through
    __syncthreads();
    float* g = a.g_pj + (size_t)b * a.pred_joints * 3;
    for (int e = j; e < a.pred_joints * 3; e += 64) {
      double v = 0.0;
      if (e < 3) {                                                  // the pelvis joint: its own sign, minus the joints' sum, minus the vertices' sum
        long long n = 0;
        int nan_bits = 0;
        for (int x = 0; x < a.nblk; ++x) {
          n += a.slots[((size_t)b * a.nblk + x) * 4 + e];
          nan_bits |= a.slots[((size_t)b * a.nblk + x) * 4 + 3];
        }
        const double sv = (nan_bits >> e) & 1 ? __builtin_nan("") : (double)n;
        const double cv = s[0] / (3.0 * (double)a.V);
        v = (s[1] * sg[e] - s[1] * (e == 0 ? sj[0] : (e == 1 ? sj[1] : sj[2]))) - cv * sv;
      } else if (e < 72) {
        v = s[1] * sg[e];
      }
      g[e] = (float)v;
    }
  }
  if (a.g_pjf) {
    const float* pf = a.pred_jf + (size_t)b * a.pred_joints * 3;
    const float* gf = a.kp3d_full + (size_t)b * a.kp3d_full_points * 3;
    float* g = a.g_pjf + (size_t)b * a.pred_joints * 3;
    for (int e = j; e < a.pred_joints * 3; e += 64)
      g[e] = e < 72 ? (float)(s[2] * sign_f64((double)pf[e] - (double)gf[e])) : 0.0f;
  }
  if (a.g_p2) {
    const float* p2 = a.pred_2d + (size_t)b * a.pred_joints * 2;
    const float* g2 = a.kp2d + (size_t)b * a.kp2d_points * 3;
    float* g = a.g_p2 + (size_t)b * a.pred_joints * 2;
    for (int e = j; e < a.pred_joints * 2; e += 64) {
      const int sjoint = e >> 1, c = e & 1;
      int o = -1;
#pragma unroll
      for (int k = 0; k < 25; ++k) o = kSmplToOpenpose[k] == sjoint ? k : o;   // the map is injective: at most one openpose joint per prediction joint
      float v = 0.0f;
      if (o >= 0) {
        const double conf = (o == 1 || o == 9 || o == 12) ? 0.0 : (double)g2[3 * o + 2];
        v = (float)(s[3] * (conf * sign_f64((double)p2[e] - (double)g2[3 * o + c])));
      }
      g[e] = v;
    }
  }
  if (a.g_betas && j < 10)
    a.g_betas[(size_t)b * 10 + j] = (float)(2.0 * s[4] * ((double)a.pred_betas[(size_t)b * 10 + j] - (double)a.gt_betas[(size_t)b * 10 + j]));
  if (a.g_bp)
    for (int i = j; i < 207; i += 64)
      a.g_bp[(size_t)b * 207 + i] = (float)(2.0 * s[5] * ((double)a.pred_bp[(size_t)b * 207 + i] - (double)a.gt_bp[(size_t)b * 207 + i]));
  if (a.g_go && j < 9)
    a.g_go[(size_t)b * 9 + j] = (float)(2.0 * s[6] * ((double)a.pred_go[(size_t)b * 9 + j] - (double)a.gt_go[(size_t)b * 9 + j]));
  if (a.g_6d && j < 24) {
    const float* x = a.pred_6d + (size_t)b * 144 + 6 * j;                                                  // x[r][c] = x[2 r + c]
    float* g = a.g_6d + (size_t)b * 144 + 6 * j;
    const double x00 = x[0], x01 = x[1], x10 = x[2], x11 = x[3], x20 = x[4], x21 = x[5];
    const double m00 = x00 * x00 + x10 * x10 + x20 * x20 - 1.0, m11 = x01 * x01 + x11 * x11 + x21 * x21 - 1.0, m01 = x00 * x01 + x10 * x11 + x20 * x21;
    const double k = s[7] * (4.0 / 96.0);                                                                  // d/dx of (m00^2 + m11^2 + 2 m01^2) / 96
    g[0] = (float)(k * (m00 * x00 + m01 * x01)); g[1] = (float)(k * (m11 * x01 + m01 * x00));
    g[2] = (float)(k * (m00 * x10 + m01 * x11)); g[3] = (float)(k * (m11 * x11 + m01 * x10));
    g[4] = (float)(k * (m00 * x20 + m01 * x21)); g[5] = (float)(k * (m11 * x21 + m01 * x20));
  }
  if (a.g_pen && j == 0) a.g_pen[b] = (float)s[8];
}

int64_t grad_workspace_bytes(int B, int V) { return (int64_t)B * v2v_blocks(V) * 4 * (int64_t)sizeof(int); }

}  // namespace

extern "C" int ehm_val_losses_backward_workspace_bytes(int B, int V, int64_t* bytes) {
  EHM_CHECK_ARG(B >= 1 && V >= 1 && bytes);
  *bytes = grad_workspace_bytes(B, V);
  return 0;
}

extern "C" int ehm_val_losses_backward(const ehm_val_losses_bwd_desc* d, void* stream) {
  EHM_CHECK_ARG(d != nullptr);
  EHM_CHECK_ARG(d->B >= 1 && d->V >= 1);
  EHM_CHECK_ARG((int64_t)d->B * d->V * 3 < ((int64_t)1 << 40) && (int64_t)d->B * v2v_blocks(d->V) <= INT32_MAX);
  EHM_CHECK_ARG(d->pred_joints >= 45 && d->gt_joints >= 24 && d->kp3d_points >= 24 && d->kp3d_full_points >= 24 && d->kp2d_points >= 25);
  EHM_CHECK_ARG(d->pred_vertices && d->pred_keypoints_3d && d->pred_keypoints_3d_full && d->pred_keypoints_2d_full);
  EHM_CHECK_ARG(d->pred_global_orient && d->pred_body_pose && d->pred_betas && d->pred_pose_6d);
  EHM_CHECK_ARG(d->keypoints_2d && d->keypoints_3d && d->keypoints_3d_full);
  EHM_CHECK_ARG(d->gt_vertices_male && d->gt_vertices_female && d->gt_joints_male && d->gt_joints_female && d->gender);
  EHM_CHECK_ARG(d->gt_global_orient && d->gt_body_pose && d->gt_betas);
  EHM_CHECK_ARG(((uintptr_t)d->pred_vertices & 15) == 0 && ((uintptr_t)d->gt_vertices_male & 15) == 0 && ((uintptr_t)d->gt_vertices_female & 15) == 0);
  EHM_CHECK_ARG(((uintptr_t)d->g_pred_vertices & 15) == 0);
  EHM_CHECK_ARG(d->workspace && ((uintptr_t)d->workspace & 3) == 0 && d->workspace_bytes >= grad_workspace_bytes(d->B, d->V));
  const hipStream_t st = (hipStream_t)stream;
  const int nblk = v2v_blocks(d->V);
  int* slots = (int*)d->workspace;
  const bool vertex_pass = d->g_pred_vertices || d->g_pred_keypoints_3d;
  if (vertex_pass)
    hipLaunchKernelGGL(v2v_grad_kernel, dim3((unsigned)(d->B * nblk)), dim3(256), 0, st, d->pred_vertices, d->gt_vertices_male, d->gt_vertices_female,
                       d->pred_keypoints_3d, d->gt_joints_male, d->gt_joints_female, d->gender, d->gloss, d->weights[0], d->g_pred_vertices, slots, d->B,
                       d->V, d->pred_joints, d->gt_joints, nblk);
  if (d->g_pred_keypoints_3d || d->g_pred_keypoints_3d_full || d->g_pred_keypoints_2d_full || d->g_pred_global_orient || d->g_pred_body_pose ||
      d->g_pred_betas || d->g_pred_pose_6d || d->g_penetration) {
    ItemGradArgs a;
    a.pred_j = d->pred_keypoints_3d; a.pred_jf = d->pred_keypoints_3d_full; a.pred_2d = d->pred_keypoints_2d_full;
    a.pred_go = d->pred_global_orient; a.pred_bp = d->pred_body_pose; a.pred_betas = d->pred_betas; a.pred_6d = d->pred_pose_6d;
    a.kp2d = d->keypoints_2d; a.kp3d = d->keypoints_3d; a.kp3d_full = d->keypoints_3d_full;
    a.gt_go = d->gt_global_orient; a.gt_bp = d->gt_body_pose; a.gt_betas = d->gt_betas; a.gloss = d->gloss;
    for (int k = 0; k < 9; ++k) a.w[k] = d->weights[k];
    a.slots = slots;
    a.g_pj = d->g_pred_keypoints_3d; a.g_pjf = d->g_pred_keypoints_3d_full; a.g_p2 = d->g_pred_keypoints_2d_full; a.g_go = d->g_pred_global_orient;
    a.g_bp = d->g_pred_body_pose; a.g_betas = d->g_pred_betas; a.g_6d = d->g_pred_pose_6d; a.g_pen = d->g_penetration;
    a.B = d->B; a.V = d->V; a.pred_joints = d->pred_joints; a.kp3d_points = d->kp3d_points; a.kp3d_full_points = d->kp3d_full_points;
    a.kp2d_points = d->kp2d_points; a.nblk = nblk;
    hipLaunchKernelGGL(item_grad_kernel, dim3((unsigned)d->B), dim3(64), 0, st, a);
  }
  EHM_LAUNCH_CHECK();
  return 0;
}
