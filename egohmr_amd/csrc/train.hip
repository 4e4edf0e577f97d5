// The denoiser's input feature on the training route of EgoHMR.forward and its vector-Jacobian product, for gfx950 (MI355X).
// The reference builds X [B, 24, D] from about ten repeat / cat / mask ops (models/egohmr/egohmr.py:190-191, :220-236, mask_cond :150-169) and lets autograd
// reduce the [B, 24, D] cotangent back over the joints; here it is one launch each way:
//   X[b, j, :] = [ vis[b,j] keep_img[b] img[b] | keep_oth[b] other[b] | x_feat[24 b + j] | temb[b] ],   D = img_dim + n_other + 2 embed_dim
//   keep_img = 1 - drop;  keep_oth = 1 - drop, or 1 with only_mask_img (drop NULL: nothing is dropped)
//   g_img[b] = keep_img[b] sum_j vis[b,j] gX[b,j,img],  g_other[b] = keep_oth[b] sum_j gX[b,j,other],  g_x_feat = gX[.., x_feat],  g_temb[b] = sum_j gX[b,j,temb]
// The masks enter as products with 0.0f / 1.0f, like `cond * mask` in the reference (a NaN under a zero mask stays a NaN, on both sides).
//
// Both kernels are memory bound.  n_other is no multiple of 4 in general (646 or 641), so D is not either, and a row of X starts at any float offset:
//   forward    a block owns one row (b, j) and walks the 16-byte aligned quads of X inside it (the few floats in front of the first and behind the last
//              quad are stored one by one): every store of a quad is one aligned 16-byte store; the source of a quad is read as 16, 2 x 8 or 4 x 4 bytes,
//              whichever its address allows (the same for all lanes of a wave: consecutive lanes hold consecutive quads of one block), and a quad that
//              straddles two blocks of columns is put together float by float;
//   backward   a thread owns four consecutive columns of one output row and adds the 24 joints in index order in a register - no atomics, no partial
//              sums across threads, so a call repeats bit for bit.  The loads follow the same 16 / 8 / 4 byte rule.  An output that is NULL gets no
//              threads: its columns of gX are never read.
#include "common.h"
#include "egohmr_hip.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct CondGeo {
  int B, img, n_other, other_ld, E, D, only_mask_img;
};

__device__ __forceinline__ bool al(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

// four consecutive floats from any float address
__device__ __forceinline__ f32x4 load4_any(const float* __restrict__ p) {
  if (al(p, 16)) return *(const f32x4*)p;
  if (al(p, 8)) {
    const f32x2 lo = *(const f32x2*)p, hi = *(const f32x2*)(p + 2);
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
  }
  return f32x4{p[0], p[1], p[2], p[3]};
}

__device__ __forceinline__ void store4_any(float* __restrict__ p, const f32x4 v) {
  if (al(p, 16)) {
    *(f32x4*)p = v;
  } else if (al(p, 8)) {
    *(f32x2*)p = f32x2{v[0], v[1]};
    *(f32x2*)(p + 2) = f32x2{v[2], v[3]};
  } else {
    p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
  }
}

struct CondSrc {
  const float *img, *other, *x_feat, *temb;     // already at the item's / the row's first float
  float s_img, s_oth;
};

// column c of the row
__device__ __forceinline__ float cond_value(const CondSrc& s, const CondGeo& g, int c) {
  if (c < g.img) return s.img[c] * s.s_img;
  c -= g.img;
  if (c < g.n_other) return s.other[c] * s.s_oth;
  c -= g.n_other;
  return c < g.E ? s.x_feat[c] : s.temb[c - g.E];
}

__global__ __launch_bounds__(256) void cond_assemble_kernel(const float* __restrict__ img, const uint8_t* __restrict__ vis, const uint8_t* __restrict__ drop,
                                                            const float* __restrict__ other, const float* __restrict__ x_feat,
                                                            const float* __restrict__ temb, float* __restrict__ X, CondGeo g) {
  const size_t r = blockIdx.x;                       // row b * 24 + j
  const int b = (int)(r / kJ);
  const bool dropped = drop != nullptr && drop[b] != 0;
  CondSrc s;
  s.img = img + (size_t)b * g.img;
  s.other = other + (size_t)b * g.other_ld;
  s.x_feat = x_feat + r * g.E;
  s.temb = temb + (size_t)b * g.E;
  s.s_img = (vis[r] != 0 ? 1.0f : 0.0f) * (dropped ? 0.0f : 1.0f);
  s.s_oth = dropped && !g.only_mask_img ? 0.0f : 1.0f;
  float* __restrict__ row = X + r * g.D;             // X is 16-byte aligned: the row starts (r D) % 4 floats behind a 16-byte boundary
  const int head = (int)((4 - (r * g.D) % 4) % 4);   // floats in front of the first aligned quad (D >= 4)
  const int nq = (g.D - head) / 4;
  const int e0 = g.img, e1 = e0 + g.n_other, e2 = e1 + g.E;
  for (int q = threadIdx.x; q < nq; q += blockDim.x) {
    const int c = head + 4 * q;
    f32x4 v;
    if (c + 4 <= e0) {
      v = load4_any(s.img + c) * s.s_img;
    } else if (c >= e0 && c + 4 <= e1) {
      v = load4_any(s.other + (c - e0)) * s.s_oth;
    } else if (c >= e1 && c + 4 <= e2) {
      v = load4_any(s.x_feat + (c - e1));
    } else if (c >= e2) {
      v = load4_any(s.temb + (c - e2));
    } else {
      v = f32x4{cond_value(s, g, c), cond_value(s, g, c + 1), cond_value(s, g, c + 2), cond_value(s, g, c + 3)};
    }
    *(f32x4*)(row + c) = v;
  }
  const int tail0 = head + 4 * nq;                   // at most 3 floats in front, at most 3 behind
  if ((int)threadIdx.x < head) row[threadIdx.x] = cond_value(s, g, threadIdx.x);
  else if ((int)threadIdx.x - head < g.D - tail0) row[tail0 + threadIdx.x - head] = cond_value(s, g, tail0 + (int)threadIdx.x - head);
}

// quads of one item: [ g_img | g_other | g_temb | g_x_feat (24 rows) ], each region absent when its output is NULL
struct BwdPlan {
  int q_img, q_oth, q_temb, q_xf, chunks;
};

__global__ __launch_bounds__(256) void cond_assemble_bwd_kernel(const float* __restrict__ gX, const uint8_t* __restrict__ vis, const uint8_t* __restrict__ drop,
                                                                float* __restrict__ g_img, float* __restrict__ g_other, float* __restrict__ g_x_feat,
                                                                float* __restrict__ g_temb, CondGeo g, BwdPlan p) {
  const int b = blockIdx.x / p.chunks;
  int q = (blockIdx.x % p.chunks) * 256 + threadIdx.x;
  const float* __restrict__ item = gX + (size_t)b * kJ * g.D;
  const int eE = g.E / 4;
  if (q >= p.q_img + p.q_oth + p.q_temb) {           // ---- g_x_feat: a copy
    q -= p.q_img + p.q_oth + p.q_temb;
    if (q >= p.q_xf) return;
    const int j = q / eE, c = 4 * (q % eE);
    *(f32x4*)(g_x_feat + ((size_t)b * kJ + j) * g.E + c) = load4_any(item + (size_t)j * g.D + g.img + g.n_other + c);
    return;
  }
  // ---- a sum over the 24 joints of (up to) four columns
  const bool dropped = drop != nullptr && drop[b] != 0;
  int col, n = 4;                                    // first column in a row of gX, live columns
  float keep = 1.0f;
  float* out;
  bool masked = false;
  if (q < p.q_img) {
    col = 4 * q;
    out = g_img + (size_t)b * g.img + col;
    keep = dropped ? 0.0f : 1.0f;
    masked = true;
  } else if (q < p.q_img + p.q_oth) {
    const int c = 4 * (q - p.q_img);
    col = g.img + c;
    n = min(4, g.n_other - c);
    out = g_other + (size_t)b * g.n_other + c;
    keep = dropped && !g.only_mask_img ? 0.0f : 1.0f;
  } else {
    const int c = 4 * (q - p.q_img - p.q_oth);
    col = g.img + g.n_other + g.E + c;
    out = g_temb + (size_t)b * g.E + c;
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < kJ; ++j) {
    const float* src = item + (size_t)j * g.D + col;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (n == 4) {
      v = load4_any(src);
    } else {
      for (int k = 0; k < n; ++k) v[k] = src[k];
    }
    if (masked) v *= vis[(size_t)b * kJ + j] != 0 ? 1.0f : 0.0f;
    acc += v;
  }
  acc *= keep;
  if (n == 4) {
    store4_any(out, acc);
  } else {
    for (int k = 0; k < n; ++k) out[k] = acc[k];
  }
}

int check_geo(int B, int img_dim, int n_other, int other_ld, int embed_dim, CondGeo* g) {
  EHM_CHECK_ARG(B >= 1 && B <= (1 << 24) && img_dim >= 4 && img_dim % 4 == 0 && embed_dim >= 4 && embed_dim % 4 == 0 && n_other >= 1 &&
                other_ld >= n_other && img_dim <= (1 << 20) && n_other <= (1 << 20) && embed_dim <= (1 << 20));
  *g = CondGeo{B, img_dim, n_other, other_ld, embed_dim, img_dim + n_other + 2 * embed_dim, 0};
  return 0;
}

}  // namespace

extern "C" int ehm_cond_assemble(const float* img_feats, const uint8_t* vis, const uint8_t* drop, const float* other, int other_ld, int n_other,
                                 const float* x_feat, const float* temb, int only_mask_img, float* X, int B, int img_dim, int embed_dim, void* stream) {
  CondGeo g;
  const int rc = check_geo(B, img_dim, n_other, other_ld, embed_dim, &g);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(img_feats && vis && other && x_feat && temb && X && ((uintptr_t)X & 15) == 0 && (only_mask_img == 0 || only_mask_img == 1));
  g.only_mask_img = only_mask_img;
  hipLaunchKernelGGL(cond_assemble_kernel, dim3((unsigned)(B * kJ)), dim3(256), 0, (hipStream_t)stream, img_feats, vis, drop, other, x_feat, temb, X, g);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_cond_assemble_backward(const float* gX, const uint8_t* vis, const uint8_t* drop, int n_other, int only_mask_img, float* g_img,
                                          float* g_other, float* g_x_feat, float* g_temb, int B, int img_dim, int embed_dim, void* stream) {
  CondGeo g;
  const int rc = check_geo(B, img_dim, n_other, n_other, embed_dim, &g);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(gX && vis && (only_mask_img == 0 || only_mask_img == 1) && ((uintptr_t)g_x_feat & 15) == 0);
  g.only_mask_img = only_mask_img;
  BwdPlan p;
  p.q_img = g_img ? img_dim / 4 : 0;
  p.q_oth = g_other ? (n_other + 3) / 4 : 0;
  p.q_temb = g_temb ? embed_dim / 4 : 0;
  p.q_xf = g_x_feat ? kJ * (embed_dim / 4) : 0;
  const int64_t total = (int64_t)p.q_img + p.q_oth + p.q_temb + p.q_xf;
  if (total == 0) return 0;
  p.chunks = (int)ceil_div(total, 256);
  EHM_CHECK_ARG((int64_t)B * p.chunks < (1ll << 31));
  hipLaunchKernelGGL(cond_assemble_bwd_kernel, dim3((unsigned)((int64_t)B * p.chunks)), dim3(256), 0, (hipStream_t)stream, gX, vis, drop, g_img, g_other,
                     g_x_feat, g_temb, g, p);
  EHM_LAUNCH_CHECK();
  return 0;
}
