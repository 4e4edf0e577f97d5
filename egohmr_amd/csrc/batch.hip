// The reference loader's item on gfx950, the two stages whose work scales with pixels and points (dataloaders/augmentation.py:get_example):
//   image_patch_kernel    generate_image_patch's warp (:121-150), BGR -> RGB, convert_cvimg_to_tensor and the colour / normalise loop (:373-383):
//                         uint8 frames in, the float32 [B,3,P,P] batch['img'] out, one launch
//   scene_augment_kernel  the scene cloud through the crop camera and back (:429-438, scene_verts_3d_processing) and the loader's [::rate] and
//                         float32 cast (egobody_dataset.py:272-273), one pass
// Both are streaming kernels: no LDS, no atomics, every output written once by one thread, so two calls give the same bits.  The per-item
// parameters (a block belongs to one item: blockIdx.y) are wave-uniform scalar loads.  The float64 arithmetic is the reference's, operation by
// operation: the pragma below keeps the compiler from contracting separately rounded products and sums into FMAs; every scalar the host can
// derive (the inverse map, cos, sin, the two translations) comes in as a double computed there (egohmr_amd/batch.py).
#include "common.h"
#include "egohmr_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kPP = EHM_PATCH_PARAMS;
constexpr int kAP = EHM_AUG_PARAMS;

// One source pixel's three bytes as doubles (BGR), or zeros outside the frame (cv2's default constant border) - outside, nothing is loaded.
struct Bgr {
  double v[3];
};
__device__ inline Bgr load_px(const uint8_t* __restrict__ frame, int H, int W, int x, int y, bool flip) {
  Bgr p = {{0.0, 0.0, 0.0}};
  if (x >= 0 && x < W && y >= 0 && y < H) {
    const uint8_t* s = frame + ((int64_t)y * W + (flip ? W - 1 - x : x)) * 3;
    p.v[0] = (double)s[0];
    p.v[1] = (double)s[1];
    p.v[2] = (double)s[2];
  }
  return p;
}

// One thread: four consecutive x of one row of one item, the three planes -> three 16-byte stores.  x is fastest across the lanes, so at
// rot = 0 a wave reads neighbouring source bytes.
__global__ __launch_bounds__(kThreads) void image_patch_kernel(const ehm_image_patch_desc d) {
  const int P = d.P, quads = P >> 2;
  const int q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= quads * P) return;
  const int b = blockIdx.y;
  const int y = q / quads, x4 = (q - y * quads) << 2;
  const double* pr = d.params + (int64_t)b * kPP;
  const double m00 = pr[EHM_PATCH_P_MINV + 0], m01 = pr[EHM_PATCH_P_MINV + 1], m02 = pr[EHM_PATCH_P_MINV + 2];
  const double m10 = pr[EHM_PATCH_P_MINV + 3], m11 = pr[EHM_PATCH_P_MINV + 4], m12 = pr[EHM_PATCH_P_MINV + 5];
  const bool flip = pr[EHM_PATCH_P_FLIP] != 0.0;
  const int f = d.frame_index[b];
  const bool frame_ok = f >= 0 && f < d.F;
  const uint8_t* frame = d.frames + (int64_t)(frame_ok ? f : 0) * d.H * d.W * 3;
  const int H = d.H, W = d.W;
  f32x4 out[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double xd = (double)(x4 + i), yd = (double)y;
    const double sx = (m00 * xd + m01 * yd) + m02;
    const double sy = (m10 * xd + m11 * yd) + m12;
    const double fx0 = floor(sx), fy0 = floor(sy);
    double v[3] = {0.0, 0.0, 0.0};
    // all four neighbours outside (or a non-finite map): the border value, and no conversion of a huge double to int
    if (fx0 >= -1.0 && fx0 < (double)W && fy0 >= -1.0 && fy0 < (double)H) {
      const int x0 = (int)fx0, y0 = (int)fy0;
      const double fx = sx - fx0, fy = sy - fy0;
      const double gx = 1.0 - fx, gy = 1.0 - fy;
      const Bgr pa = load_px(frame, H, W, x0, y0, flip), pb = load_px(frame, H, W, x0 + 1, y0, flip);
      const Bgr pc = load_px(frame, H, W, x0, y0 + 1, flip), pd = load_px(frame, H, W, x0 + 1, y0 + 1, flip);
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = (pa.v[k] * gx + pb.v[k] * fx) * gy + (pc.v[k] * gx + pd.v[k] * fx) * fy;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double vv = v[2 - c];                                   // RGB channel c is BGR channel 2 - c
      if (d.quantize) vv = floor(vv + 0.5);
      float p = (float)vv;
      p = p * (float)pr[EHM_PATCH_P_COLOR + c];
      p = p < 0.0f ? 0.0f : (p > 255.0f ? 255.0f : p);        // np.clip: a NaN stays a NaN
      p = (p - (float)d.mean[c]) / (float)d.std[c];
      out[c][i] = frame_ok ? p : __builtin_nanf("");
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) *(f32x4*)(d.img + (((int64_t)b * 3 + c) * P + y) * P + x4) = out[c];
}

template <typename T>
__global__ __launch_bounds__(kThreads) void scene_augment_kernel(const T* __restrict__ scene, const double* __restrict__ params,
                                                                  float* __restrict__ out, int N, int rows, int stride) {
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= rows) return;
  const int b = blockIdx.y;
  const double* pr = params + (int64_t)b * kAP;
  const bool flip = pr[EHM_AUG_P_FLIP] != 0.0;
  const double cs = pr[EHM_AUG_P_COS], sn = pr[EHM_AUG_P_SIN];
  const T* s = scene + ((int64_t)b * N + (int64_t)r * stride) * 3;
  double q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = ((double)s[k] - pr[EHM_AUG_P_TFULL + k]) + pr[EHM_AUG_P_TCROP + k];
  if (flip) q[0] = -q[0];
  // einsum('ij,kj->ki', rot_mat, v) with rot_mat = [[cs, -sn, 0], [sn, cs, 0], [0, 0, 1]], summed over j in order
  const float r0 = (float)((cs * q[0] + (-sn) * q[1]) + 0.0 * q[2]);
  const float r1 = (float)((sn * q[0] + cs * q[1]) + 0.0 * q[2]);
  const float r2 = (float)((0.0 * q[0] + 0.0 * q[1]) + 1.0 * q[2]);
  const double sg = flip ? -1.0 : 1.0;                        // :434-436: both translations' x change sign under flip
  float* o = out + ((int64_t)b * rows + r) * 3;
  o[0] = (float)(((double)r0 - sg * pr[EHM_AUG_P_TCROP + 0]) + sg * pr[EHM_AUG_P_TFULL + 0]);
  o[1] = (float)(((double)r1 - pr[EHM_AUG_P_TCROP + 1]) + pr[EHM_AUG_P_TFULL + 1]);
  o[2] = (float)(((double)r2 - pr[EHM_AUG_P_TCROP + 2]) + pr[EHM_AUG_P_TFULL + 2]);
}

}  // namespace

extern "C" int ehm_image_patch(const ehm_image_patch_desc* d, void* stream) {
  EHM_CHECK_ARG(d && d->frames && d->frame_index && d->params && d->img);
  EHM_CHECK_ARG(d->B > 0 && d->B <= 65535 && d->F > 0 && d->H > 0 && d->W > 0);
  EHM_CHECK_ARG(d->P > 0 && d->P % 4 == 0 && d->P <= 16384);
  EHM_CHECK_ARG(((uintptr_t)d->img & 15) == 0);
  const int64_t quads = (int64_t)d->P * d->P / 4;
  const dim3 grid((unsigned)ceil_div(quads, kThreads), (unsigned)d->B);
  hipLaunchKernelGGL(image_patch_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, *d);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_scene_augment(const void* scene, int scene_is_f64, const double* params, float* out, int B, int N, int stride, void* stream) {
  EHM_CHECK_ARG(scene && params && out);
  EHM_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && stride >= 1);
  const int rows = (int)ceil_div(N, stride);
  const dim3 grid((unsigned)ceil_div(rows, kThreads), (unsigned)B);
  if (scene_is_f64)
    hipLaunchKernelGGL(scene_augment_kernel<double>, grid, dim3(kThreads), 0, (hipStream_t)stream, (const double*)scene, params, out, N, rows, stride);
  else
    hipLaunchKernelGGL(scene_augment_kernel<float>, grid, dim3(kThreads), 0, (hipStream_t)stream, (const float*)scene, params, out, N, rows, stride);
  EHM_LAUNCH_CHECK();
  return 0;
}
