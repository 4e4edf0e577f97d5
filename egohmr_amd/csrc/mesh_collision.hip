// Mesh collision term for gfx950: occupancy of the posed body by the generalised winding number, penetration depth by the closest point of the
// nearest triangle (the rule: include/egohmr_hip.h, "mesh collision term").  The opt-in alternative to guidance.hip's nearest-vertex proxy, behind the
// same bbox_kernel / select_kernel; everything downstream of d loss / d vertex (skin_bwd_kernel ... finish_kernel) is shared.
//   mesh_collision_kernel   block = 256 selected points of one body (one per thread, state in registers: winding sum, best squared distance, best
//                           face); the F faces pass through LDS in chunks of 512 as 64-byte records gathered from the body's vertices (which stay
//                           in L2: 83 KB at SMPL's size), every record read by all 256 points at one address (an LDS broadcast).  Then, per inside
//                           point, d^2 into the block's sum and 2 beta_k (c - p) into the three vertices of the nearest face (float atomics, as the
//                           vertex proxy's scatter: a few hundred inside points per body at most, nine scalar adds each).
//   mesh_loss_sum_kernel    loss[b] = the blocks' sums in chunk order.
// No global scratch of its own: a block's sum goes into the FIRST index slot of the 256 it has read from select_kernel's list (its own slice, read
// at entry, written after the block's last barrier), so loss has a fixed order without one more buffer; hits are integer atomics (exact in any order).
#include "common.h"
#include "egohmr_hip.h"
#include "internal.h"

namespace {

constexpr int kPB = EHM_MESH_COLLISION_POINT_BLOCK;
constexpr int kFC = EHM_MESH_COLLISION_FACE_CHUNK;
static_assert(kPB % 64 == 0 && kPB <= 1024 && kFC >= 1, "point block: whole waves");
constexpr float kPi = 3.14159265358979323846f;

// what a (point, face) pair needs of a face, independent of the point: v0, the two edges from it, the normal e1 x e2 (not normalised) and the edges'
// Gram matrix.  ok = 0: a face that repeats a vertex index (no area, no side): it is skipped, in the winding sum and in the nearest-face search alike.
struct FaceRec {
  float v0[3], e1[3], e2[3], n[3], e11, e12, e22, ok;
};

__device__ __forceinline__ FaceRec face_rec(const float* __restrict__ vb, const int32_t* __restrict__ faces, int f) {
  const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  FaceRec r;
  float v1[3], v2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    r.v0[c] = vb[(size_t)i0 * 3 + c];
    v1[c] = vb[(size_t)i1 * 3 + c];
    v2[c] = vb[(size_t)i2 * 3 + c];
    r.e1[c] = v1[c] - r.v0[c];
    r.e2[c] = v2[c] - r.v0[c];
  }
  r.n[0] = r.e1[1] * r.e2[2] - r.e1[2] * r.e2[1];
  r.n[1] = r.e1[2] * r.e2[0] - r.e1[0] * r.e2[2];
  r.n[2] = r.e1[0] * r.e2[1] - r.e1[1] * r.e2[0];
  r.e11 = r.e1[0] * r.e1[0] + r.e1[1] * r.e1[1] + r.e1[2] * r.e1[2];
  r.e12 = r.e1[0] * r.e2[0] + r.e1[1] * r.e2[1] + r.e1[2] * r.e2[2];
  r.e22 = r.e2[0] * r.e2[0] + r.e2[1] * r.e2[1] + r.e2[2] * r.e2[2];
  r.ok = (i0 != i1 && i1 != i2 && i0 != i2) ? 1.f : 0.f;
  return r;
}

__device__ __forceinline__ float safe_div(float num, float den) { return den > 0.f ? num / den : 0.f; }

// Closest point of triangle (v0, v0 + e1, v0 + e2) to p, as barycentric weights (1 - v - w, v, w): the seven regions of the textbook test (vertex A,
// vertex B, edge AB, vertex C, edge AC, edge BC, interior), the first that applies.  Written as overrides in REVERSE order, so that every lane of a
// wave runs the same straight-line code (the points of a wave fall into different regions of one face).  a = v0 - p.
__device__ __forceinline__ void closest_bary(const float (&a)[3], const FaceRec& r, float& v, float& w) {
  const float d1 = -(r.e1[0] * a[0] + r.e1[1] * a[1] + r.e1[2] * a[2]);   // ab . ap
  const float d2 = -(r.e2[0] * a[0] + r.e2[1] * a[1] + r.e2[2] * a[2]);   // ac . ap
  const float d3 = d1 - r.e11, d4 = d2 - r.e12;                            // ab . bp, ac . bp   (bp = ap - ab)
  const float d5 = d1 - r.e12, d6 = d2 - r.e22;                            // ab . cp, ac . cp   (cp = ap - ac)
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float inv = safe_div(1.f, va + vb + vc);
  v = vb * inv;                                                            // interior
  w = vc * inv;
  if (va <= 0.f && d4 - d3 >= 0.f && d5 - d6 >= 0.f) { w = safe_div(d4 - d3, (d4 - d3) + (d5 - d6)); v = 1.f - w; }   // edge BC
  if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { v = 0.f; w = safe_div(d2, d2 - d6); }                                    // edge AC
  if (d6 >= 0.f && d5 <= d6) { v = 0.f; w = 1.f; }                                                                    // vertex C
  if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { v = safe_div(d1, d1 - d3); w = 0.f; }                                    // edge AB
  if (d3 >= 0.f && d4 <= d3) { v = 1.f; w = 0.f; }                                                                    // vertex B
  if (d1 <= 0.f && d2 <= 0.f) { v = 0.f; w = 0.f; }                                                                   // vertex A
}

// grid (point chunks of kPB, B).  idx / count: select_kernel's list, or nullptr / nullptr = every point (all_points).  partial: [B][N] words, MAY BE the
// memory of idx (see the head of the file; neither is __restrict__).
__global__ __launch_bounds__(kPB) void mesh_collision_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                             const float* __restrict__ scene, const int* idx, const int* __restrict__ count,
                                                             float* partial, float* __restrict__ gverts, int* __restrict__ hits, int V, int F, int N) {
  __shared__ f32x4 sf[kFC][4];
  __shared__ float sred[kPB];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int cnt = count ? count[b] : N;
  if (chunk * kPB >= cnt) return;                        // block-uniform
  const int k = chunk * kPB + tid;
  const bool active = k < cnt;
  const float* vb = verts + (size_t)b * V * 3;
  float p[3] = {0.f, 0.f, 0.f};
  if (active) {
    const int i = idx ? idx[(size_t)b * N + k] : k;
    const float* q = scene + ((size_t)b * N + i) * 3;
    p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
  }
  float wsum = 0.f, best = 3.4e38f;                      // sum of atan2 (= Omega / 2), nearest squared distance
  int bf = -1;
  for (int f0 = 0; f0 < F; f0 += kFC) {
    const int nf = min(kFC, F - f0);
    __syncthreads();                                     // (the previous chunk has been read by every wave)
    for (int j = tid; j < nf; j += kPB) {
      const FaceRec r = face_rec(vb, faces, f0 + j);
      sf[j][0] = f32x4{r.v0[0], r.v0[1], r.v0[2], r.ok};
      sf[j][1] = f32x4{r.e1[0], r.e1[1], r.e1[2], r.e11};
      sf[j][2] = f32x4{r.e2[0], r.e2[1], r.e2[2], r.e22};
      sf[j][3] = f32x4{r.n[0], r.n[1], r.n[2], r.e12};
    }
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < nf; ++j) {
      const f32x4 s0 = sf[j][0], s1 = sf[j][1], s2 = sf[j][2], s3 = sf[j][3];
      if (s0[3] == 0.f) continue;                        // (uniform: every lane reads the same face)
      FaceRec r;
      r.v0[0] = s0[0]; r.v0[1] = s0[1]; r.v0[2] = s0[2];
      r.e1[0] = s1[0]; r.e1[1] = s1[1]; r.e1[2] = s1[2]; r.e11 = s1[3];
      r.e2[0] = s2[0]; r.e2[1] = s2[1]; r.e2[2] = s2[2]; r.e22 = s2[3];
      r.n[0] = s3[0]; r.n[1] = s3[1]; r.n[2] = s3[2]; r.e12 = s3[3];
      const float a[3] = {r.v0[0] - p[0], r.v0[1] - p[1], r.v0[2] - p[2]};
      const float bb[3] = {a[0] + r.e1[0], a[1] + r.e1[1], a[2] + r.e1[2]};
      const float cc[3] = {a[0] + r.e2[0], a[1] + r.e2[1], a[2] + r.e2[2]};
      // Omega / 2 = atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|);  a . (b x c) = a . (e1 x e2): the terms with a twice vanish
      const float det = a[0] * r.n[0] + a[1] * r.n[1] + a[2] * r.n[2];
      const float la = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
      const float lb = sqrtf(bb[0] * bb[0] + bb[1] * bb[1] + bb[2] * bb[2]);
      const float lc = sqrtf(cc[0] * cc[0] + cc[1] * cc[1] + cc[2] * cc[2]);
      const float ab = a[0] * bb[0] + a[1] * bb[1] + a[2] * bb[2];
      const float bc = bb[0] * cc[0] + bb[1] * cc[1] + bb[2] * cc[2];
      const float ca = cc[0] * a[0] + cc[1] * a[1] + cc[2] * a[2];
      wsum += atan2f(det, la * lb * lc + ab * lc + bc * la + ca * lb);
      float v, w;
      closest_bary(a, r, v, w);
      const float qx = a[0] + v * r.e1[0] + w * r.e2[0], qy = a[1] + v * r.e1[1] + w * r.e2[1], qz = a[2] + v * r.e1[2] + w * r.e2[2];
      const float d2 = qx * qx + qy * qy + qz * qz;
      if (d2 < best) { best = d2; bf = f0 + j; }         // strict <: the lowest face index among equally near ones
    }
  }
  // inside <=> w = sum Omega / 4 pi > 0.5 <=> sum of the atan2 > pi
  const bool inside = active && bf >= 0 && wsum > kPi;
  float contrib = 0.f;
  if (inside) {
    const FaceRec r = face_rec(vb, faces, bf);           // the nearest face again, with the scan's own arithmetic: c - p and the weights
    const float a[3] = {r.v0[0] - p[0], r.v0[1] - p[1], r.v0[2] - p[2]};
    float v, w;
    closest_bary(a, r, v, w);
    const float q[3] = {a[0] + v * r.e1[0] + w * r.e2[0], a[1] + v * r.e1[1] + w * r.e2[1], a[2] + v * r.e1[2] + w * r.e2[2]};
    contrib = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
    if (gverts) {                                        // d (d^2) / d v_k = 2 beta_k (c - p) at fixed beta
      const float beta[3] = {1.f - v - w, v, w};
#pragma unroll
      for (int kk = 0; kk < 3; ++kk) {
        if (beta[kk] == 0.f) continue;
        float* g = gverts + ((size_t)b * V + faces[3 * bf + kk]) * 3;
        const float s = 2.f * beta[kk];
        atomicAdd(g + 0, s * q[0]);
        atomicAdd(g + 1, s * q[1]);
        atomicAdd(g + 2, s * q[2]);
      }
    }
  }
  if (hits) {                                            // one integer add per wave
    const int n = __popcll(__ballot(inside));
    if ((tid & 63) == 0 && n) atomicAdd(hits + b, n);
  }
  // the block's sum: 256 squared depths added in index order, in double (once per block: nothing beside the pair loop), rounded once
  sred[tid] = contrib;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < kPB; ++i) s += (double)sred[i];
    partial[(size_t)b * N + (size_t)chunk * kPB] = (float)s;
  }
}

__global__ void mesh_loss_sum_kernel(const float* __restrict__ partial, const int* __restrict__ count, float* __restrict__ loss, int B, int N) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int cnt = count ? count[b] : N;
  double s = 0.0;
  for (int c = 0; c * kPB < cnt; ++c) s += (double)partial[(size_t)b * N + (size_t)c * kPB];
  loss[b] = (float)s;
}

}  // namespace

int ehm_mesh_collision_launch(const float* verts, const int32_t* faces, const float* scene, const int* idx, const int* count, void* partial,
                              float* loss, float* gverts, int* hits, int B, int V, int F, int N, hipStream_t st) {
  EHM_CHECK_ARG(B > 0 && B <= 65535 && V > 0 && F >= 1 && N > 0 && partial);
  if (gverts) EHM_HIP(hipMemsetAsync(gverts, 0, (size_t)B * V * 3 * sizeof(float), st));
  if (hits) EHM_HIP(hipMemsetAsync(hits, 0, (size_t)B * sizeof(int), st));
  hipLaunchKernelGGL(mesh_collision_kernel, dim3((unsigned)ceil_div(N, kPB), B), dim3(kPB), 0, st, verts, faces, scene, idx, count, (float*)partial,
                     gverts, hits, V, F, N);
  hipLaunchKernelGGL(mesh_loss_sum_kernel, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0, st, (const float*)partial, count, loss, B, N);
  EHM_LAUNCH_CHECK();
  return 0;
}
