// Stage 1 (ProHMR-scene) pose flow on gfx950: nflows' ConditionalGlow(144, 1024, 4, 2, context) of models/prohmr/smpl_flow.py, both directions,
// and the first derivatives of both (egohmr_amd/flow_grad.py walks them).  The arithmetic is a sequential chain of small float32 GEMMs
// ([R, 72 | 144 | 1024] x [., 72 | 144 | 1024], R = items x samples)
// with element-wise steps between them; every per-row product is one launch of flow_gemm_kernel, which carries the element-wise step in front of it
// as a prologue and the one behind it as an epilogue, so a direction is ~29 launches and no torch op.  The terms that depend on the item only (the
// context slices of every first layer and GLU gate) are ONE ehm_skinny_gemm_f32 over the row ehm_flow_context writes.
//
//   flow_context_kernel   the conditioning row [cam centre | bbox | fx | img | scene] of prohmr_scene.py:111-130, zero-padded to a multiple of 32
//   flow_gemm_kernel      skinny_gemm_f32_kernel (linear.hip) with the flow's prologues and epilogues: 32 x 32 output tile per block, the waves
//                         split K, one k-ordered chain per wave, a fixed-order LDS reduction - exact float32, no atomics, two calls give the same bits
//   flow_finish_kernel    log_prob of a row and, on the sampling side, pred_pose_6d and the 24 rotation matrices ('prohmr' rot6d rule)
// The backward adds no GEMM kernel for its data gradients: dY W^T is flow_gemm_kernel on the torch-layout weight ([out, in] is the [K, N] operand) with
// the gate prologue and the ReLU-mask epilogues.  What is new:
//   flow_wgrad_kernel     out[n][k] = alpha sum_r G'[r][n] act(X[r][k]) + beta out: the contraction over the rows straight from the row-major operands,
//                         one wave per 32 x 32 tile, ONE r-ordered chain per tile (the order depends on R alone)
//   flow_colsum_kernel / flow_item_reduce_kernel   bias gradients, per-item sums and the gate term, summed in row order
//   flow_finish_bwd_kernel / flow_sum_kernel       the VJP of flow_finish_kernel
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

// the GLU gate: one expression, shared by the forward epilogue and every backward step that reads the gate again
static __device__ __forceinline__ float flow_sigmoid(float g) { return 1.f / (1.f + expf(-g)); }

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
  const bool w_ok = n0 + mi < d.N;                               // columns >= N of W are not read (w_window: ldw >= N is all the operand offers)
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
      } else if constexpr (PRO == EHM_FLOW_PRO_GATE) {
        const float* gate = d.item + (size_t)(row / d.S) * d.ld_item + kk;
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = a[i] * flow_sigmoid(gate[i]);
      }
    }
    float b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = w_ok ? wb[(size_t)(k + i) * d.ldw] : 0.f;
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
    if (epi == EHM_FLOW_EPI_SCATTER_ADD || epi == EHM_FLOW_EPI_SCATTER_SUB) col = n_ok ? d.scatter[n] : -1;
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
        if (d.aux) d.aux[(size_t)ro * d.ldy + n] = v;
        *y = fmaf(v, flow_sigmoid(g), d.add ? d.add[(size_t)ro * d.ld_add + n] : *y);
      } else if (epi == EHM_FLOW_EPI_SCATTER_ADD) *y = *y + v;
      else if (epi == EHM_FLOW_EPI_SCATTER_SUB) *y = *y - v;
      else if (epi == EHM_FLOW_EPI_MASK) *y = d.mask[(size_t)ro * d.ld_mask + n] > 0.f ? v : 0.f;
      else if (epi == EHM_FLOW_EPI_MASK_ADD) *y = d.add[(size_t)ro * d.ld_add + n] + (d.mask[(size_t)ro * d.ld_mask + n] > 0.f ? v : 0.f);
      else *y = d.add[(size_t)ro * d.ld_add + n] + v;               // EHM_FLOW_EPI_ADD
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

// ---------------------------------------------------------------------------------------------- backward
// One wave per 32 x 32 tile of out [Cg, Ca], four tiles (2 x 2) per block, no shared memory.  MFMA i of a 16-row step contracts rows r0 + 2 i (lane
// half 0) and r0 + 2 i + 1 (half 1): A[n][r] = G'[r][n0 + lane & 31], B[r][k] = X'[r][k0 + lane & 31], both read along a row of the row-major
// operand.  Rows >= R and columns >= Cg / >= Ca enter as zeros and are never read.
__global__ __launch_bounds__(256) void flow_wgrad_kernel(const ehm_flow_wgrad_desc d) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int mi = lane & 31, h = lane >> 5;
  const int n0 = 32 * (2 * blockIdx.y + (wave >> 1)), k0 = 32 * (2 * blockIdx.x + (wave & 1));
  if (n0 >= d.Cg || k0 >= d.Ca) return;                          // (wave-uniform; the kernel has no barrier)
  const int n = n0 + mi, k = k0 + mi;
  const bool n_ok = n < d.Cg, k_ok = k < d.Ca;
  int gcol = n_ok ? (d.gather_g ? d.gather_g[n] : n) : -1, xcol = k_ok ? (d.gather_x ? d.gather_x[k] : k) : -1;
  if ((unsigned)gcol >= (unsigned)d.ldg) gcol = -1;              // an index outside the row reads as 0, as in ehm_flow_gemm
  if ((unsigned)xcol >= (unsigned)d.ldx) xcol = -1;
  const float shift = (d.x_shift && k_ok) ? d.x_shift[k] : 0.f;
  const bool relu = d.act == EHM_FLOW_ACT_RELU;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int r0 = 0; r0 < d.R; r0 += 16) {
    float a[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = r0 + 2 * i + h;
      const bool ok = row < d.R;
      float g = (ok && gcol >= 0) ? d.G[(size_t)row * d.ldg + gcol] : 0.f;
      if (d.item && ok && n_ok) g = g * flow_sigmoid(d.item[(size_t)(row / d.S) * d.ld_item + n]);
      float x = 0.f;
      if (ok && xcol >= 0) {
        x = d.X[(size_t)row * d.ldx + xcol] - shift;
        if (relu) x = fmaxf(x, 0.f);
      }
      a[i] = g;
      b[i] = x;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[i], acc, 0, 0, 0);
  }
  if (!k_ok) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int nn = n0 + (r & 3) + 8 * (r >> 2) + 4 * h;          // accumulator layout: column = lane & 31 (k), row as in flow_gemm_kernel (n)
    if (nn >= d.Cg) continue;
    float* o = d.out + (size_t)nn * d.ld_out + k;
    const float v = d.alpha * acc[r];
    *o = d.beta != 0.f ? fmaf(d.beta, *o, v) : v;
  }
}

// column sums over all rows: lane = column, 16 waves take 16 consecutive runs of rows, their sums are added in wave order
__global__ __launch_bounds__(1024) void flow_colsum_kernel(const ehm_flow_reduce_desc d) {
  __shared__ float red[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = 64 * blockIdx.x + lane;
  const int run = (d.R + 15) / 16;
  const int r_begin = wave * run, r_end = min(d.R, r_begin + run);
  float s = 0.f;
  if (n < d.N) {
    int col = d.gather ? d.gather[n] : n;
    if ((unsigned)col >= (unsigned)d.ldg) col = -1;
    if (col >= 0) {
      for (int r = r_begin; r < r_end; ++r) {
        float g = d.G[(size_t)r * d.ldg + col];
        if (d.item) g = g * flow_sigmoid(d.item[(size_t)(r / d.S) * d.ld_item + n]);
        s += g;
      }
    }
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && n < d.N) {
    float t = red[0][lane];
#pragma unroll
    for (int w = 1; w < 16; ++w) t += red[w][lane];
    d.out[n] = d.scale * t;
  }
}

// per-item sums over an item's S rows (row order): EHM_FLOW_RED_ITEM sum G, EHM_FLOW_RED_GATE sum G u2 sigma (1 - sigma), sigma = sigmoid(item[i][n])
__global__ __launch_bounds__(256) void flow_item_reduce_kernel(const ehm_flow_reduce_desc d) {
  const int n = 256 * blockIdx.x + threadIdx.x, i = blockIdx.y;
  if (n >= d.N) return;
  const int r_begin = i * d.S, r_end = min(d.R, r_begin + d.S);
  float s = 0.f;
  if (d.mode == EHM_FLOW_RED_GATE) {
    const float sg = flow_sigmoid(d.item[(size_t)i * d.ld_item + n]);
    const float w = sg * (1.f - sg);
    for (int r = r_begin; r < r_end; ++r) s += d.G[(size_t)r * d.ldg + n] * d.U2[(size_t)r * d.ldu + n] * w;
  } else {
    for (int r = r_begin; r < r_end; ++r) s += d.G[(size_t)r * d.ldg + n];
  }
  d.out[(size_t)i * d.ld_out + n] = d.scale * s;
}

// sum of v[0 .. R): lane l adds rows l, l + 64, ...; lane 0 adds the 64 partial sums in lane order
__global__ __launch_bounds__(64) void flow_sum_kernel(const float* __restrict__ v, float* __restrict__ out, int R) {
  __shared__ float part[64];
  float s = 0.f;
  for (int r = threadIdx.x; r < R; r += 64) s += v[r];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = part[0];
    for (int l = 1; l < 64; ++l) t += part[l];
    *out = t;
  }
}

// thread = (row, joint | column): dz = dz_add - dlp z over the 144 columns, and the rot6d VJP of a row's 24 joints plus the direct pred_pose_6d term
__global__ __launch_bounds__(256) void flow_finish_bwd_kernel(const float* __restrict__ g_lp, const float* __restrict__ z, const float* __restrict__ dz_add,
                                                              float* __restrict__ dz, const float* __restrict__ pose, const float* __restrict__ g_p6,
                                                              const float* __restrict__ g_go, const float* __restrict__ g_bp, float* __restrict__ dpose,
                                                              int R) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (dz && t < (int64_t)R * kPoseDim) {
    const float add = dz_add ? dz_add[t] : 0.f;
    dz[t] = g_lp ? fmaf(-g_lp[t / kPoseDim], z[t], add) : add;
  }
  if (dpose && t < (int64_t)R * kJ) {
    const int64_t row = t / kJ;
    const int j = (int)(t % kJ);
    float ga1[3] = {0.f, 0.f, 0.f}, ga2[3] = {0.f, 0.f, 0.f};
    const float* gR = j == 0 ? (g_go ? g_go + row * 9 : nullptr) : (g_bp ? g_bp + (row * (kJ - 1) + (j - 1)) * 9 : nullptr);
    if (gR) {
      const float* p = pose + t * 6;
      float g[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) g[i] = gR[i];
      rot6d_bwd(p[0], p[1], p[2], p[3], p[4], p[5], g, ga1, ga2);   // 'prohmr' (mode 0 of ehm_rot6d_to_rotmat_bwd)
    }
    float* o = dpose + t * 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      o[c] = ga1[c] + (g_p6 ? g_p6[t * 6 + c] : 0.f);
      o[3 + c] = ga2[c] + (g_p6 ? g_p6[t * 6 + 3 + c] : 0.f);
    }
  }
}

template <int NW>
void launch_flow_gemm(const ehm_flow_gemm_desc& d, dim3 grid, hipStream_t st) {
  switch (d.prologue) {
    case EHM_FLOW_PRO_NONE: hipLaunchKernelGGL((flow_gemm_kernel<NW, EHM_FLOW_PRO_NONE>), grid, dim3(64 * NW), 0, st, d); break;
    case EHM_FLOW_PRO_RELU: hipLaunchKernelGGL((flow_gemm_kernel<NW, EHM_FLOW_PRO_RELU>), grid, dim3(64 * NW), 0, st, d); break;
    case EHM_FLOW_PRO_BN_RELU: hipLaunchKernelGGL((flow_gemm_kernel<NW, EHM_FLOW_PRO_BN_RELU>), grid, dim3(64 * NW), 0, st, d); break;
    case EHM_FLOW_PRO_SHIFT: hipLaunchKernelGGL((flow_gemm_kernel<NW, EHM_FLOW_PRO_SHIFT>), grid, dim3(64 * NW), 0, st, d); break;
    default: hipLaunchKernelGGL((flow_gemm_kernel<NW, EHM_FLOW_PRO_GATE>), grid, dim3(64 * NW), 0, st, d); break;
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
  if (d->K % 8 != 0 || (d->ldw % 32 != 0 && !d->w_window) || d->ldw < d->N || d->ldy <= 0 || d->ldx <= 0) {
    ehm_set_error("ehm_flow_gemm needs K %% 8 == 0, ldw %% 32 == 0 (or w_window), ldw >= N and positive ldx, ldy (K = %d, N = %d, ldw = %d, ldx = %d, "
                  "ldy = %d)", d->K, d->N, d->ldw, d->ldx, d->ldy);
    return EHM_EINVAL;
  }
  if (!d->gather && (d->ldx < d->K || d->ldx % 4 != 0 || ((uintptr_t)d->X % 16) != 0)) {
    ehm_set_error("ehm_flow_gemm without a gather list needs ldx >= K, ldx %% 4 == 0 and a 16-byte aligned X (K = %d, ldx = %d)", d->K, d->ldx);
    return EHM_EINVAL;
  }
  EHM_CHECK_ARG(d->prologue >= EHM_FLOW_PRO_NONE && d->prologue <= EHM_FLOW_PRO_GATE);
  EHM_CHECK_ARG(d->prologue != EHM_FLOW_PRO_BN_RELU || (d->pro_scale && d->pro_shift));
  EHM_CHECK_ARG(d->prologue != EHM_FLOW_PRO_SHIFT || d->pro_shift);
  EHM_CHECK_ARG(d->epilogue >= EHM_FLOW_EPI_BIAS && d->epilogue <= EHM_FLOW_EPI_ADD);
  const bool per_item = d->epilogue == EHM_FLOW_EPI_ITEM_ADD || d->epilogue == EHM_FLOW_EPI_GLU_RES;
  const bool scatter = d->epilogue == EHM_FLOW_EPI_SCATTER_ADD || d->epilogue == EHM_FLOW_EPI_SCATTER_SUB;
  const bool masked = d->epilogue == EHM_FLOW_EPI_MASK || d->epilogue == EHM_FLOW_EPI_MASK_ADD;
  const bool adds = d->epilogue == EHM_FLOW_EPI_MASK_ADD || d->epilogue == EHM_FLOW_EPI_ADD;
  EHM_CHECK_ARG(!per_item || (d->item && d->ld_item >= d->N));
  EHM_CHECK_ARG(d->prologue != EHM_FLOW_PRO_GATE || (d->item && d->ld_item >= d->K && !per_item));   // (one `item`: the gate's or the epilogue's)
  EHM_CHECK_ARG(!masked || (d->mask && d->ld_mask >= d->N && (const void*)d->mask != (const void*)d->Y));
  EHM_CHECK_ARG(!adds || (d->add && d->ld_add >= d->N));
  EHM_CHECK_ARG(d->epilogue == EHM_FLOW_EPI_GLU_RES || adds || !d->add);
  EHM_CHECK_ARG(d->epilogue == EHM_FLOW_EPI_GLU_RES || !d->aux);
  EHM_CHECK_ARG(!d->add || d->ld_add >= d->N);
  EHM_CHECK_ARG((const void*)d->aux != (const void*)d->Y && (const void*)d->aux != (const void*)d->X);
  EHM_CHECK_ARG(!scatter || d->scatter);
  EHM_CHECK_ARG(scatter || d->ldy >= d->N);
  const dim3 grid((unsigned)ceil_div(d->N, 32), (unsigned)ceil_div(d->R, 32));
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

extern "C" int ehm_flow_wgrad(const ehm_flow_wgrad_desc* d, void* stream) {
  EHM_CHECK_ARG(d && d->G && d->X && d->out && d->R > 0 && d->Cg > 0 && d->Ca > 0 && d->S > 0);
  EHM_CHECK_ARG((const void*)d->out != (const void*)d->G && (const void*)d->out != (const void*)d->X);
  if (d->ldg <= 0 || d->ldx <= 0 || d->ld_out < d->Ca || (!d->gather_g && d->ldg < d->Cg) || (!d->gather_x && d->ldx < d->Ca)) {
    ehm_set_error("ehm_flow_wgrad needs ld_out >= Ca and, without a gather list, ldg >= Cg and ldx >= Ca (Cg = %d, Ca = %d, ldg = %d, ldx = %d, ld_out = %d)",
                  d->Cg, d->Ca, d->ldg, d->ldx, d->ld_out);
    return EHM_EINVAL;
  }
  EHM_CHECK_ARG(!d->item || d->ld_item >= d->Cg);
  EHM_CHECK_ARG(d->act == EHM_FLOW_ACT_NONE || d->act == EHM_FLOW_ACT_RELU);
  const dim3 grid((unsigned)ceil_div(d->Ca, 64), (unsigned)ceil_div(d->Cg, 64));
  EHM_CHECK_ARG(grid.y <= 65535);
  hipLaunchKernelGGL(flow_wgrad_kernel, grid, dim3(256), 0, (hipStream_t)stream, *d);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_flow_reduce(const ehm_flow_reduce_desc* d, void* stream) {
  EHM_CHECK_ARG(d && d->G && d->out && d->R > 0 && d->N > 0 && d->S > 0 && d->ldg > 0);
  EHM_CHECK_ARG(d->mode >= EHM_FLOW_RED_COLS && d->mode <= EHM_FLOW_RED_GATE);
  EHM_CHECK_ARG((const void*)d->out != (const void*)d->G);
  EHM_CHECK_ARG(!d->item || d->ld_item >= d->N);
  if (d->mode == EHM_FLOW_RED_COLS) {
    EHM_CHECK_ARG(d->gather || d->ldg >= d->N);
    hipLaunchKernelGGL(flow_colsum_kernel, dim3((unsigned)ceil_div(d->N, 64)), dim3(1024), 0, (hipStream_t)stream, *d);
  } else {
    const int64_t items = ceil_div(d->R, d->S);
    EHM_CHECK_ARG(!d->gather && d->ldg >= d->N && d->ld_out >= d->N && items <= 65535);
    EHM_CHECK_ARG(d->mode != EHM_FLOW_RED_GATE || (d->U2 && d->item && d->ldu >= d->N));
    hipLaunchKernelGGL(flow_item_reduce_kernel, dim3((unsigned)ceil_div(d->N, 256), (unsigned)items), dim3(256), 0, (hipStream_t)stream, *d);
  }
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_flow_finish_backward(const float* g_log_prob, const float* z, const float* dz_add, float* dz, float* sum_g_log_prob, const float* pose,
                                        const float* g_pose6d, const float* g_global_orient, const float* g_body_pose, float* dpose, int R,
                                        void* stream) {
  EHM_CHECK_ARG(R > 0 && (dz || sum_g_log_prob || dpose));
  EHM_CHECK_ARG(!dz || ((!g_log_prob || z) && (g_log_prob || dz_add)));
  EHM_CHECK_ARG(!sum_g_log_prob || g_log_prob);
  EHM_CHECK_ARG(!dpose || (pose && dpose != pose));
  EHM_CHECK_ARG(dz == nullptr || (dz != z));
  if (dz || dpose) {
    const int64_t threads = (int64_t)R * (dz ? kPoseDim : kJ);
    hipLaunchKernelGGL(flow_finish_bwd_kernel, dim3((unsigned)ceil_div(threads, 256)), dim3(256), 0, (hipStream_t)stream, g_log_prob, z, dz_add, dz,
                       pose, g_pose6d, g_global_orient, g_body_pose, dpose, R);
    EHM_LAUNCH_CHECK();
  }
  if (sum_g_log_prob) {
    hipLaunchKernelGGL(flow_sum_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, g_log_prob, sum_g_log_prob, R);
    EHM_LAUNCH_CHECK();
  }
  return 0;
}
