// Stage 1 (ProHMR-scene) translation on gfx950: the deterministic half of the reference's stage-1 model - context assembly
// (models/prohmr/prohmr_scene.py:111-130), the camera / betas head FCHead (models/prohmr/fc_head.py:46-50) and the full-image camera conversion of
// test_prohmr_scene.py:175-213 (utils/geometry.py:119-131) - in one launch.  The normalizing flow (pose samples, log-prob) is csrc/flow.hip:
// pred_cam does not read it.
//
// One 256-thread block per group of kItems items.  Layer 1 (K x 1024, K = 2560 + the switched leading features): thread t owns hidden units
// t + 256 q (q < 4) of all kItems items, 32 f32 accumulators; the context is read IN PLACE from the two feature matrices and the per-item scalars,
// kKc columns at a time, into LDS as [column][item] (one column = two broadcast ds_read_b128); W1 is read transposed ([K, 1024]: lane-consecutive
// hidden units, coalesced).  Layer 2 (1024 -> 13) runs from LDS, one wave per two items, one wave_sum per output.  Roofline at B = 256: 1.35 GFLOP
// of f32 FMA and 10.5 MB of W1 per block from L2 / Infinity Cache - 32 blocks, a few tens of microseconds against ~9 ms of ResNet-50; the layout
// is chosen for clarity, not for peak.
#include "common.h"
#include "egohmr_hip.h"

namespace {

constexpr int kItems = 8;       // items per block
constexpr int kHidden = 1024;   // FCHead NUM_FEATURES (configs/prohmr.yaml)
constexpr int kOut = 13;        // 10 betas + 3 camera
constexpr int kKc = 256;        // context columns per LDS chunk (= threads per block: one column per thread per chunk)

__global__ __launch_bounds__(256) void stage1_head_kernel(const ehm_stage1_desc d) {
  __shared__ float lead_s[kItems][8];                 // the switched leading features of each item (at most 6)
  __shared__ float4 ctx_s[kKc][kItems / 4];           // a chunk of the context, [column][item]
  __shared__ float h_s[kItems][kHidden];              // relu(W1 ctx + b1)
  const int t = threadIdx.x, b0 = blockIdx.x * kItems;
  const int n_lead = (d.with_cam_center ? 2 : 0) + (d.with_bbox_info ? 3 : 0) + (d.with_focal_length ? 1 : 0);
  const int K = n_lead + d.img_dim + d.scene_dim;

  // ---- leading features, in the reference's order: [cam center | bbox | fx] (each concatenated IN FRONT of the previous context)
  if (t < kItems) {
    const int b = b0 + t;
    int c = 0;
    if (b < d.B) {
      const float fx = d.fx[b], ofx = fx * d.fx_norm;
      if (d.with_cam_center) { lead_s[t][c++] = d.cam_cx[b] / ofx; lead_s[t][c++] = d.cam_cy[b] / ofx; }
      if (d.with_bbox_info) {
        lead_s[t][c++] = d.box_center[2 * b] / ofx; lead_s[t][c++] = d.box_center[2 * b + 1] / ofx; lead_s[t][c++] = d.box_size[b] / ofx;
      }
      if (d.with_focal_length) lead_s[t][c++] = fx;
    }
    for (; c < 8; ++c) lead_s[t][c] = 0.f;
  }

  float acc[kItems][4];
#pragma unroll
  for (int i = 0; i < kItems; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[i][q] = 0.f;

  for (int k0 = 0; k0 < K; k0 += kKc) {
    __syncthreads();                                  // (the lead_s writes, and the previous chunk's readers)
    {
      const int k = k0 + t;                           // this thread's context column of the chunk, for every item
      float v[kItems];
#pragma unroll
      for (int i = 0; i < kItems; ++i) {
        const int b = b0 + i;
        float x = 0.f;
        if (b < d.B && k < K) {
          if (k < n_lead) x = lead_s[i][k];
          else if (k < n_lead + d.img_dim) x = d.img_feats[(size_t)b * d.img_dim + (k - n_lead)];
          else x = d.scene_feats[(size_t)b * d.scene_dim + (k - n_lead - d.img_dim)];
        }
        v[i] = x;
      }
#pragma unroll
      for (int i4 = 0; i4 < kItems / 4; ++i4) ctx_s[t][i4] = make_float4(v[4 * i4], v[4 * i4 + 1], v[4 * i4 + 2], v[4 * i4 + 3]);
    }
    __syncthreads();
    const int kn = min(kKc, K - k0);
    const float* w = d.W1t + (size_t)k0 * kHidden + t;
#pragma unroll 4
    for (int kk = 0; kk < kn; ++kk) {
      float wq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) wq[q] = w[(size_t)kk * kHidden + 256 * q];
#pragma unroll
      for (int i4 = 0; i4 < kItems / 4; ++i4) {
        const float4 c = ctx_s[kk][i4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc[4 * i4 + 0][q] = fmaf(wq[q], c.x, acc[4 * i4 + 0][q]);
          acc[4 * i4 + 1][q] = fmaf(wq[q], c.y, acc[4 * i4 + 1][q]);
          acc[4 * i4 + 2][q] = fmaf(wq[q], c.z, acc[4 * i4 + 2][q]);
          acc[4 * i4 + 3][q] = fmaf(wq[q], c.w, acc[4 * i4 + 3][q]);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int u = t + 256 * q;
    const float bias = d.b1[u];
#pragma unroll
    for (int i = 0; i < kItems; ++i) h_s[i][u] = fmaxf(acc[i][q] + bias, 0.f);
  }
  __syncthreads();

  // ---- layer 2 + outputs: wave w takes items 2w, 2w+1; every lane ends with the wave's sums (wave_sum is wave-uniform)
  const int wave = t >> 6, lane = t & 63;
#pragma unroll
  for (int ii = 0; ii < kItems / 4; ++ii) {
    const int i = wave * (kItems / 4) + ii, b = b0 + i;
    if (b >= d.B) break;                              // (wave-uniform)
    float off[kOut];
#pragma unroll
    for (int o = 0; o < kOut; ++o) {
      float p = 0.f;
      for (int u = lane; u < kHidden; u += 64) p = fmaf(d.W2[(size_t)o * kHidden + u], h_s[i][u], p);
      off[o] = wave_sum(p) + d.b2[o];
    }
    if (lane == 0) {
      if (d.pred_betas)
        for (int j = 0; j < 10; ++j) d.pred_betas[(size_t)b * 10 + j] = off[j] + d.init_betas[j];
      const float s = off[10] + d.init_cam[0], tx = off[11] + d.init_cam[1], ty = off[12] + d.init_cam[2];
      d.pred_cam[(size_t)b * 3 + 0] = s; d.pred_cam[(size_t)b * 3 + 1] = tx; d.pred_cam[(size_t)b * 3 + 2] = ty;
      // convert_pare_to_full_img_cam with focal = fx * fx_norm, img_w = 2 cam_cx, img_h = 2 cam_cy, bbox_height = box_size; s is NOT clamped
      // (s = 0 gives inf, as the reference).  Same operation order as the reference's float32 torch expression.
      const float focal = d.fx[b] * d.fx_norm, bh = d.box_size[b];
      const float r = bh / d.crop_res;
      const float tz = (2.f * focal) / ((r * d.crop_res) * s);
      const float img_w = d.cam_cx[b] * 2.f, img_h = d.cam_cy[b] * 2.f;
      const float cx = (2.f * (d.box_center[2 * b] - img_w / 2.f)) / (s * bh);
      const float cy = (2.f * (d.box_center[2 * b + 1] - img_h / 2.f)) / (s * bh);
      d.pred_cam_full[(size_t)b * 3 + 0] = tx + cx; d.pred_cam_full[(size_t)b * 3 + 1] = ty + cy; d.pred_cam_full[(size_t)b * 3 + 2] = tz;
    }
  }
}

}  // namespace

extern "C" int ehm_stage1_head(const ehm_stage1_desc* d, void* stream) {
  EHM_CHECK_ARG(d && d->B > 0 && d->img_feats && d->scene_feats && d->fx && d->cam_cx && d->cam_cy && d->box_center && d->box_size);
  EHM_CHECK_ARG(d->W1t && d->b1 && d->W2 && d->b2 && d->init_cam && d->init_betas && d->pred_cam && d->pred_cam_full);
  EHM_CHECK_ARG(d->hidden == kHidden && d->img_dim > 0 && d->scene_dim > 0 && d->crop_res > 0.f);
  EHM_CHECK_ARG((int64_t)d->img_dim + d->scene_dim + 6 <= INT32_MAX / kHidden);
  hipLaunchKernelGGL(stage1_head_kernel, dim3((unsigned)ceil_div(d->B, kItems)), dim3(256), 0, (hipStream_t)stream, *d);
  EHM_LAUNCH_CHECK();
  return 0;
}
