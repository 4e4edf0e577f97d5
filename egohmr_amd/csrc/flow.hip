// Stage 1 (ProHMR-scene) pose flow on gfx950: nflows' ConditionalGlow(144, 1024, 4, 2, context) of models/prohmr/smpl_flow.py, both directions,
// inference only.  The arithmetic is a sequential chain of small float32 GEMMs ([R, 72 | 144 | 1024] x [., 72 | 144 | 1024], R = items x samples)
// with element-wise steps between them; every per-row product is one launch of flow_gemm_kernel, which carries the element-wise step in front of it
// as a prologue and the one behind it as an epilogue, so a direction is ~29 launches and no torch op.  The terms that depend on the item only (the
// context slices of every first layer and GLU gate) are ONE ehm_skinny_gemm_f32 over the row ehm_flow_context writes.
//
//   flow_context_kernel   the conditioning row [cam centre | bbox | fx | img | scene] of prohmr_scene.py:111-130, zero-padded to a multiple of 32
//   flow_gemm_kernel      skinny_gemm_f32_kernel (linear.hip) with the flow's prologues and epilogues: 32 x 32 output tile per block, the waves
//                         split K, one k-ordered chain per wave, a fixed-order LDS reduction - exact float32, no atomics, two calls give the same bits
//   flow_finish_kernel    log_prob of a row and, on the sampling side, pred_pose_6d and the 24 rotation matrices ('prohmr' rot6d rule)
#include "common.h"
#include "egohmr_hip.h"
#include "smpl_dev.h"

namespace {

__global__ __launch_bounds__(256) void flow_context_kernel(const ehm_flow_context_desc d) {
  const int b = blockIdx.y;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= d.ctx_pad) return;
  const int n_cc = d.with_cam_center ? 2 : 0, n_bb = d.with_bbox_info ? 3 : 0, n_fl = d.with_focal_length ? 1 : 0;
  const int n_lead = n_cc + n_bb + n_fl;
  float v = 0.f;
  if (k < n_lead) {
    // the leading features in the reference's order (each group concatenated IN FRONT of the previous context), as ehm_stage1_head forms them
    const float fx = d.fx[b], ofx = fx * d.fx_norm;
    if (k < n_cc) v = (k == 0 ? d.cam_cx[b] : d.cam_cy[b]) / ofx;
    else if (k < n_cc + n_bb) {
      const int j = k - n_cc;
      v = (j == 0 ? d.box_center[2 * b] : (j == 1 ? d.box_center[2 * b + 1] : d.box_size[b])) / ofx;
    } else v = fx;
  } else if (k < n_lead + d.img_dim) v = d.img_feats[(size_t)b * d.img_dim + (k - n_lead)];
  else if (k < n_lead + d.img_dim + d.scene_dim) v = d.scene_feats[(size_t)b * d.scene_dim + (k - n_lead - d.img_dim)];
  d.out[(size_t)b * d.ctx_pad + k] = v;
}

// A fragment: lane (row = l & 31, h = l >> 5) holds X[row][k + 4 h .. + 3]; MFMA i of an 8-k group contracts k + i and k + 4 + i (linear.hip).
template <int NW, int PRO>
__global__ __launch_bounds__(64 * NW) void flow_gemm_kernel(const ehm_flow_gemm_desc d) {
  __shared__ float red[NW - 1][32][33];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int mi = lane & 31, h = lane >> 5;
  const int n0 = 32 * blockIdx.x, m0 = 32 * blockIdx.y;
  const int G = d.K / 8;
  const int k_begin = 8 * (int)((long long)wave * G / NW), kq = 8 * (int)((long long)(wave + 1) * G / NW) - k_begin;
  const int row = m0 + mi;
  const bool row_ok = row < d.R;
  const float* xrow = d.X + (size_t)(row_ok ? row : 0) * d.ldx;
  const float* wb = d.W + (size_t)(k_begin + 4 * h) * d.ldw + n0 + mi;
  const int32_t* gather = d.gather;                              // (block-uniform)
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 8
  for (int k = 0; k < kq; k += 8) {
    const int kk = k_begin + 4 * h + k;
    f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
    if (row_ok) {                                                // rows >= R are not read
      if (gather) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = gather[kk + i];
          a[i] = (unsigned)c < (unsigned)d.ldx ? xrow[c] : 0.f;
        }
      } else a = *(const f32x4*)(xrow + kk);
      if constexpr (PRO == EHM_FLOW_PRO_RELU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = fmaxf(a[i], 0.f);
      } else if constexpr (PRO == EHM_FLOW_PRO_BN_RELU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = fmaxf(fmaf(d.pro_scale[kk + i], a[i], d.pro_shift[kk + i]), 0.f);
      } else if constexpr (PRO == EHM_FLOW_PRO_SHIFT) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = a[i] - d.pro_shift[kk + i];
      }
    }
    float b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = wb[(size_t)(k + i) * d.ldw];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[i], acc, 0, 0, 0);
  }
  // accumulator layout: column = mi, row = (r & 3) + 8 (r >> 2) + 4 h
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave - 1][(r & 3) + 8 * (r >> 2) + 4 * h][mi] = acc[r];
  }
  __syncthreads();
  if (wave == 0) {
    const int n = n0 + mi;
    const bool n_ok = n < d.N;
    const float add = (d.bias && n_ok) ? d.bias[n] : 0.f;
    const int epi = d.epilogue;
    int col = n;                                                 // the column of Y this lane writes
    if (epi >= EHM_FLOW_EPI_SCATTER_ADD) col = n_ok ? d.scatter[n] : -1;
    const bool col_ok = n_ok && (unsigned)col < (unsigned)d.ldy;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = (r & 3) + 8 * (r >> 2) + 4 * h;
      float v = acc[r];
#pragma unroll
      for (int w = 0; w < NW - 1; ++w) v += red[w][rr][mi];          // (k order: wave 0, 1, 2, ...)
      v += add;
      const int ro = m0 + rr;
      if (ro >= d.R || !col_ok) continue;
      float* y = d.Y + (size_t)ro * d.ldy + col;
      if (epi == EHM_FLOW_EPI_BIAS) *y = v;
      else if (epi == EHM_FLOW_EPI_ITEM_ADD) *y = v + d.item[(size_t)(ro / d.S) * d.ld_item + n];
      else if (epi == EHM_FLOW_EPI_GLU_RES) {
        const float g = d.item[(size_t)(ro / d.S) * d.ld_item + n];
        *y = fmaf(v, 1.f / (1.f + expf(-g)), *y);
      } else if (epi == EHM_FLOW_EPI_SCATTER_ADD) *y = *y + v;
      else *y = *y - v;
    }
  }
}

// one wave per row, four rows per block: lanes 0 .. 23 a joint's rotation each, lane 24 the row's norm
__global__ __launch_bounds__(256) void flow_finish_kernel(const float* __restrict__ z, double log_prob_const, float* __restrict__ log_prob,
                                                          const float* __restrict__ pose, float* __restrict__ pose6d_out,
                                                          float* __restrict__ global_orient, float* __restrict__ body_pose, int R) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= R) return;
  if (lane == 24) {
    const float* zr = z + (size_t)row * kPoseDim;
    float ss = 0.f;
    for (int i = 0; i < kPoseDim; ++i) ss = fmaf(zr[i], zr[i], ss);
    log_prob[row] = (float)(log_prob_const - 0.5 * (double)ss);
  }
  if (pose && lane < kJ) {
    const float* p = pose + (size_t)row * kPoseDim + 6 * lane;
    float q[6], Rm[9];
#pragma unroll
    for (int i = 0; i < 6; ++i) q[i] = p[i];
    rot6d_to_R(q[0], q[1], q[2], q[3], q[4], q[5], Rm);           // 'prohmr' (mode 0 of ehm_rot6d_to_rotmat)
    float* o6 = pose6d_out + (size_t)row * kPoseDim + 6 * lane;
#pragma unroll
    for (int i = 0; i < 6; ++i) o6[i] = q[i];
    float* o = lane == 0 ? global_orient + (size_t)row * 9 : body_pose + ((size_t)row * (kJ - 1) + (lane - 1)) * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = Rm[i];
  }
}

template <int NW>
void launch_flow_gemm(const ehm_flow_gemm_desc& d, dim3 grid, hipStream_t st) {
  switch (d.prologue) {
    case EHM_FLOW_PRO_NONE: hipLaunchKernelGGL((flow_gemm_kernel<NW, EHM_FLOW_PRO_NONE>), grid, dim3(64 * NW), 0, st, d); break;
    case EHM_FLOW_PRO_RELU: hipLaunchKernelGGL((flow_gemm_kernel<NW, EHM_FLOW_PRO_RELU>), grid, dim3(64 * NW), 0, st, d); break;
    case EHM_FLOW_PRO_BN_RELU: hipLaunchKernelGGL((flow_gemm_kernel<NW, EHM_FLOW_PRO_BN_RELU>), grid, dim3(64 * NW), 0, st, d); break;
    default: hipLaunchKernelGGL((flow_gemm_kernel<NW, EHM_FLOW_PRO_SHIFT>), grid, dim3(64 * NW), 0, st, d); break;
  }
}

}  // namespace

extern "C" int ehm_flow_context(const ehm_flow_context_desc* d, void* stream) {
  EHM_CHECK_ARG(d && d->B > 0 && d->img_feats && d->scene_feats && d->fx && d->cam_cx && d->cam_cy && d->box_center && d->box_size && d->out);
  EHM_CHECK_ARG(d->img_dim > 0 && d->scene_dim > 0 && (int64_t)d->img_dim + d->scene_dim + 6 <= (1 << 24));
  const int K = d->img_dim + d->scene_dim + (d->with_cam_center ? 2 : 0) + (d->with_bbox_info ? 3 : 0) + (d->with_focal_length ? 1 : 0);
  if (d->ctx_pad < K || d->B > 65535) {
    ehm_set_error("ehm_flow_context: ctx_pad = %d is shorter than the context (%d columns), or B = %d > 65535", d->ctx_pad, K, d->B);
    return EHM_EINVAL;
  }
  hipLaunchKernelGGL(flow_context_kernel, dim3((unsigned)ceil_div(d->ctx_pad, 256), (unsigned)d->B), dim3(256), 0, (hipStream_t)stream, *d);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_flow_gemm(const ehm_flow_gemm_desc* d, void* stream) {
  EHM_CHECK_ARG(d && d->X && d->W && d->Y && d->R > 0 && d->K > 0 && d->N > 0 && d->S > 0);
  EHM_CHECK_ARG((const void*)d->X != (const void*)d->Y);
  if (d->K % 8 != 0 || d->ldw % 32 != 0 || d->ldw < d->N || d->ldy <= 0 || d->ldx <= 0) {
    ehm_set_error("ehm_flow_gemm needs K %% 8 == 0, ldw %% 32 == 0, ldw >= N and positive ldx, ldy (K = %d, N = %d, ldw = %d, ldx = %d, ldy = %d)",
                  d->K, d->N, d->ldw, d->ldx, d->ldy);
    return EHM_EINVAL;
  }
  if (!d->gather && (d->ldx < d->K || d->ldx % 4 != 0 || ((uintptr_t)d->X % 16) != 0)) {
    ehm_set_error("ehm_flow_gemm without a gather list needs ldx >= K, ldx %% 4 == 0 and a 16-byte aligned X (K = %d, ldx = %d)", d->K, d->ldx);
    return EHM_EINVAL;
  }
  EHM_CHECK_ARG(d->prologue >= EHM_FLOW_PRO_NONE && d->prologue <= EHM_FLOW_PRO_SHIFT);
  EHM_CHECK_ARG(d->prologue != EHM_FLOW_PRO_BN_RELU || (d->pro_scale && d->pro_shift));
  EHM_CHECK_ARG(d->prologue != EHM_FLOW_PRO_SHIFT || d->pro_shift);
  EHM_CHECK_ARG(d->epilogue >= EHM_FLOW_EPI_BIAS && d->epilogue <= EHM_FLOW_EPI_SCATTER_SUB);
  const bool per_item = d->epilogue == EHM_FLOW_EPI_ITEM_ADD || d->epilogue == EHM_FLOW_EPI_GLU_RES;
  const bool scatter = d->epilogue >= EHM_FLOW_EPI_SCATTER_ADD;
  EHM_CHECK_ARG(!per_item || (d->item && d->ld_item >= d->N));
  EHM_CHECK_ARG(!scatter || d->scatter);
  EHM_CHECK_ARG(scatter || d->ldy >= d->N);
  const dim3 grid((unsigned)ceil_div(d->N, 32), (unsigned)ceil_div(d->R, 32));   // (ldw >= N, ldw % 32 == 0: every tile's 32 columns of W exist)
  EHM_CHECK_ARG(grid.y <= 65535);
  if (d->K >= 1024) launch_flow_gemm<16>(*d, grid, (hipStream_t)stream);
  else launch_flow_gemm<4>(*d, grid, (hipStream_t)stream);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_flow_finish(const float* z, double log_prob_const, float* log_prob, const float* pose, float* pose6d_out, float* global_orient,
                               float* body_pose, int R, void* stream) {
  EHM_CHECK_ARG(z && log_prob && R > 0);
  const int n_pose = (pose != nullptr) + (pose6d_out != nullptr) + (global_orient != nullptr) + (body_pose != nullptr);
  EHM_CHECK_ARG(n_pose == 0 || n_pose == 4);
  hipLaunchKernelGGL(flow_finish_kernel, dim3((unsigned)ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, z, log_prob_const, log_prob, pose,
                     pose6d_out, global_orient, body_pose, R);
  EHM_LAUNCH_CHECK();
  return 0;
}
