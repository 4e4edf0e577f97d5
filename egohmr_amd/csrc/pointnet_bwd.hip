// Vector-Jacobian product of the scene PointNet (models/respointnet.py:33-97) for gfx950 (MI355X): everything of its backward that is not a GEMM.
// The forward it differentiates (egohmr_amd/encoders.py ResnetPointnet, csrc/linear.hip), per block with x = cat[net, pooled] (block 0: x = net0 = fc_pos(p)):
//   h = fc_0(relu(x)),  net' = fc_1(relu(h)) + shortcut(x),  pooled' = max over the N valid points of a body.
// and, with gnet' = dL/dnet' (absent behind the last block) and gpool' = dL/dpooled':
//   G  = gnet' + one-hot(arg) gpool'                 pointnet_scatter_kernel   (arg = lowest maximising row: pool_argmax_*)
//   dh = (G W1) (.) [relu(h) > 0]                    pointnet_gate_kernel
//   dx = (dh W0) (.) [x > 0] + G S                   pointnet_gate_kernel (with `add`)
//   column sums over all rows and over each body     the same kernels' block partials + group_sums_kernel / total_sums_kernel
//   fc_pos: Wbar = net0bar^T p, bbar = sum net0bar, pbar = net0bar W      pointnet_lift_bwd_kernel
//   weight gradients G^T relu(h), G^T net, dh^T relu(net)                  pointnet_wgrad_kernel (exact-f32 MFMA, split-K over the rows) + wgrad_finish_kernel
// The data-gradient GEMMs run on ehm_conv_nhwc_split (egohmr_amd/pointnet_grad.py).
//
// Matrices are [B * Np, C] with Np a multiple of the 192-row tile of linear.hip and C a multiple of 128; rows >= N of a body are padding: never read
// as candidates or summands, written as exact zeros.  A block owns one 192-row slab x 128 columns: 32 lanes x 16 bytes across, 8 row lanes down;
// a lane adds its 24 rows in row order, the 8 row lanes are added in index order through LDS, the slabs of a body and then the bodies in index order
// (float64) by the two small finish kernels.  No atomics: two calls on the same inputs give the same bits.
#include <limits.h>

#include "common.h"
#include "egohmr_hip.h"
#include "gcn_dev.h"

namespace {

constexpr int SLAB = 192;          // rows per block = LBM of linear.hip (a body's rows are a whole number of slabs)
constexpr int CW = 128;            // columns per block
constexpr int RL = 8;              // row lanes per block

typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

struct Geo { int N, Np, C; };

// four consecutive values (c % 4 == 0) of row `row` of a float32 or an X2 matrix
template <bool X2>
__device__ __forceinline__ f32x4 load4(const void* base, size_t row, int c, int C) {
  if constexpr (X2) {
    const half_t* p = (const half_t*)base + split_off<32>(row, c, C);
    const half4 hi = *(const half4*)p, lo = *(const half4*)(p + 32);
    return f32x4{(float)hi[0] + (float)lo[0], (float)hi[1] + (float)lo[1], (float)hi[2] + (float)lo[2], (float)hi[3] + (float)lo[3]};
  } else {
    return *(const f32x4*)((const float*)base + row * (size_t)C + c);
  }
}

// is (v, r) a better maximum than (bv, br)?  NaN beats every number (torch.max propagates it); among equals the lower row wins
__device__ __forceinline__ bool better(float v, int r, float bv, int br) {
  if (v != v) return bv == bv || r < br;
  if (bv != bv) return false;
  return v > bv || (v == bv && r < br);
}

// the block's position: slab -> (first global row, first row inside its body), my columns, my row lane
struct Pos { size_t row0; int i0, b, c, rl; };
__device__ __forceinline__ Pos block_pos(int Np) {
  Pos p;
  p.row0 = (size_t)blockIdx.x * SLAB;
  p.b = (int)(p.row0 / (size_t)Np);
  p.i0 = (int)(p.row0 - (size_t)p.b * Np);
  p.c = blockIdx.y * CW + 4 * (threadIdx.x & 31);
  p.rl = threadIdx.x >> 5;
  return p;
}

// acc of the 8 row lanes, added in index order -> part[slab][C]
__device__ __forceinline__ void reduce_row_lanes(const f32x4 acc, float* __restrict__ part, int C) {
  __shared__ __attribute__((aligned(16))) float red[RL][CW];
  *(f32x4*)&red[threadIdx.x >> 5][4 * (threadIdx.x & 31)] = acc;
  __syncthreads();
  if (threadIdx.x < CW) {
    float s = red[0][threadIdx.x];
#pragma unroll
    for (int r = 1; r < RL; ++r) s += red[r][threadIdx.x];
    part[(size_t)blockIdx.x * C + blockIdx.y * CW + threadIdx.x] = s;
  }
}

template <bool X2>
__global__ __launch_bounds__(256) void pool_argmax_slab_kernel(const void* __restrict__ net, float* __restrict__ pv, int* __restrict__ pr, Geo g) {
  __shared__ float sv[RL][CW];
  __shared__ int sr[RL][CW];
  const Pos p = block_pos(g.Np);
  float bv[4];
  int br[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { bv[q] = -INFINITY; br[q] = INT_MAX; }
  for (int i = p.rl; i < SLAB && p.i0 + i < g.N; i += RL) {
    const f32x4 x = load4<X2>(net, p.row0 + i, p.c, g.C);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (better(x[q], p.i0 + i, bv[q], br[q])) { bv[q] = x[q]; br[q] = p.i0 + i; }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    sv[p.rl][4 * (threadIdx.x & 31) + q] = bv[q];
    sr[p.rl][4 * (threadIdx.x & 31) + q] = br[q];
  }
  __syncthreads();
  if (threadIdx.x < CW) {
    float v = sv[0][threadIdx.x];
    int r = sr[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < RL; ++k)
      if (better(sv[k][threadIdx.x], sr[k][threadIdx.x], v, r)) { v = sv[k][threadIdx.x]; r = sr[k][threadIdx.x]; }
    const size_t o = (size_t)blockIdx.x * g.C + blockIdx.y * CW + threadIdx.x;
    pv[o] = v;
    pr[o] = r;
  }
}

__global__ __launch_bounds__(256) void pool_argmax_finish_kernel(const float* __restrict__ pv, const int* __restrict__ pr, int* __restrict__ arg, int spg,
                                                                  int C, long long total) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long long b = t / C;
  const int c = (int)(t - b * C);
  float v = -INFINITY;
  int r = INT_MAX;
  for (int s = 0; s < spg; ++s) {
    const size_t o = ((size_t)b * spg + s) * C + c;
    const int rs = pr[o];
    if (rs != INT_MAX && better(pv[o], rs, v, r)) { v = pv[o]; r = rs; }
  }
  arg[t] = r;
}

__global__ __launch_bounds__(256) void pointnet_scatter_kernel(const float* __restrict__ gnet, const float* __restrict__ gpool, const int* __restrict__ arg,
                                                                float* __restrict__ G, float* __restrict__ part, Geo g) {
  const Pos p = block_pos(g.Np);
  const f32x4 gp = *(const f32x4*)(gpool + (size_t)p.b * g.C + p.c);
  const i32x4 ar = *(const i32x4*)(arg + (size_t)p.b * g.C + p.c);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int i = p.rl; i < SLAB; i += RL) {
    const int gi = p.i0 + i;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (gi < g.N) {
      if (gnet) v = *(const f32x4*)(gnet + (p.row0 + i) * (size_t)g.C + p.c);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] += ar[q] == gi ? gp[q] : 0.f;
      acc += v;
    }
    *(f32x4*)(G + (p.row0 + i) * (size_t)g.C + p.c) = v;
  }
  if (part) reduce_row_lanes(acc, part, g.C);
}

template <bool X2>
__global__ __launch_bounds__(256) void pointnet_gate_kernel(const float* T, const void* __restrict__ act, const float* __restrict__ add,
                                                             const float* __restrict__ t_scale, const float* __restrict__ add_scale, float* out,
                                                             float* __restrict__ part, Geo g) {
  const Pos p = block_pos(g.Np);
  const float ts = t_scale ? *t_scale : 1.f, as = add_scale ? *add_scale : 1.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int i = p.rl; i < SLAB; i += RL) {
    const size_t row = p.row0 + i;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (p.i0 + i < g.N) {
      const f32x4 t = *(const f32x4*)(T + row * (size_t)g.C + p.c);
      const f32x4 a = load4<X2>(act, row, p.c, g.C);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = a[q] > 0.f ? t[q] * ts : 0.f;
      if (add) {
        const f32x4 d = *(const f32x4*)(add + row * (size_t)g.C + p.c);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] += d[q] * as;
      }
      acc += v;
    }
    *(f32x4*)(out + row * (size_t)g.C + p.c) = v;          // (out may be T: every element is read and written by the same lane)
  }
  if (part) reduce_row_lanes(acc, part, g.C);
}

// net0 = fc_pos(p) with the forward loader's own arithmetic (linear.hip gen_a: fmaf(w_z, z, fmaf(w_y, y, fmaf(w_x, x, b)))), so [net0 > 0] is the forward's gate
__global__ __launch_bounds__(256) void pointnet_net0_kernel(const float* __restrict__ pts, const float* __restrict__ Wpos, const float* __restrict__ bpos,
                                                             float* __restrict__ net0, float* __restrict__ rnet0, Geo g) {
  const Pos p = block_pos(g.Np);
  float w[4][3], bb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int k = 0; k < 3; ++k) w[q][k] = Wpos[(size_t)(p.c + q) * 3 + k];
    bb[q] = bpos[p.c + q];
  }
  for (int i = p.rl; i < SLAB; i += RL) {
    const size_t row = p.row0 + i;
    const int gi = p.i0 + i;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (gi < g.N) {
      const float* q3 = pts + ((size_t)p.b * g.N + gi) * 3;
      const float x = q3[0], y = q3[1], z = q3[2];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = fmaf(w[q][2], z, fmaf(w[q][1], y, fmaf(w[q][0], x, bb[q])));
    }
    if (net0) *(f32x4*)(net0 + row * (size_t)g.C + p.c) = v;
    if (rnet0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = fmaxf(v[q], 0.f);
      *(f32x4*)(rnet0 + row * (size_t)g.C + p.c) = v;
    }
  }
}

// X [M, C], points -> part[slab][C][4] = sum over the slab's valid rows of X[m,c] (x, y, z, 1) and, when gp is given, gp[b,i,:] = X[m,:] Wpos.
// One wave per row: a lane owns 4 columns of every 256-column chunk; the rows of a wave go in row order, the 4 waves are added in index order.
__global__ __launch_bounds__(256) void pointnet_lift_bwd_kernel(const float* __restrict__ X, const float* __restrict__ pts, const float* __restrict__ Wpos,
                                                                 float* __restrict__ gp, float* __restrict__ part, Geo g) {
  __shared__ float sp[SLAB][3];
  __shared__ float sg[SLAB][3];
  __shared__ __attribute__((aligned(16))) float red[4][64][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row0 = (size_t)blockIdx.x * SLAB;
  const int b = (int)(row0 / (size_t)g.Np), i0 = (int)(row0 - (size_t)b * g.Np);
  int nvalid = g.N - i0;
  nvalid = nvalid < 0 ? 0 : (nvalid > SLAB ? SLAB : nvalid);
  for (int e = tid; e < SLAB * 3; e += 256) {
    const int i = e / 3, k = e - 3 * i;
    sp[i][k] = i < nvalid ? pts[((size_t)b * g.N + i0 + i) * 3 + k] : 0.f;
    sg[i][k] = 0.f;
  }
  __syncthreads();
  for (int c0 = 0; c0 < g.C; c0 += 256) {
    const int c = c0 + 4 * lane;
    const bool live = c < g.C;
    float w[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int k = 0; k < 3; ++k) w[q][k] = (gp && live) ? Wpos[(size_t)(c + q) * 3 + k] : 0.f;
    float acc[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[q][k] = 0.f;
    for (int i = wave; i < nvalid; i += 4) {
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (live) x = *(const f32x4*)(X + (row0 + i) * (size_t)g.C + c);
      const float px = sp[i][0], py = sp[i][1], pz = sp[i][2];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[q][0] = fmaf(x[q], px, acc[q][0]);
        acc[q][1] = fmaf(x[q], py, acc[q][1]);
        acc[q][2] = fmaf(x[q], pz, acc[q][2]);
        acc[q][3] += x[q];
      }
      if (gp) {                                            // (block-uniform)
        float t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          t[k] = fmaf(x[3], w[3][k], fmaf(x[2], w[2][k], fmaf(x[1], w[1][k], x[0] * w[0][k])));
          t[k] = wave_sum(t[k]);
        }
        if (lane == 0) {                                   // row i belongs to this wave alone: chunk after chunk in program order
#pragma unroll
          for (int k = 0; k < 3; ++k) sg[i][k] += t[k];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) *(f32x4*)&red[wave][lane][4 * q] = f32x4{acc[q][0], acc[q][1], acc[q][2], acc[q][3]};
    __syncthreads();
    {
      const int col = tid, cc = c0 + col;                  // thread t: column c0 + t, its four sums
      if (cc < g.C) {
        f32x4 s = *(const f32x4*)&red[0][col >> 2][4 * (col & 3)];
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) s += *(const f32x4*)&red[wv][col >> 2][4 * (col & 3)];
        *(f32x4*)(part + ((size_t)blockIdx.x * g.C + cc) * 4) = s;
      }
    }
    __syncthreads();
  }
  if (gp)
    for (int e = tid; e < nvalid * 3; e += 256) {
      const int i = e / 3, k = e - 3 * i;
      gp[((size_t)b * g.N + i0 + i) * 3 + k] = sg[i][k];
    }
}

// out[g, a] = sum over the valid rows m of P[m, g] act(Q[m, a]): a weight gradient, the contraction over the rows, straight from the row-major operands.
// v_mfma_f32_32x32x2_f32 takes A[i][k] from lane (i = l & 31, k = l >> 5) and B[k][j] from lane (j = l & 31, k = l >> 5): with k = the row, both fragments are
// 128-byte runs of a row of P and of Q - no transpose, no packing, exact float32 products.  A block owns a 128 x 128 tile of `out` for one run of slabs (split-K over
// the rows); its 4 waves own 64 x 64 each = 2 x 2 accumulators, 16 rows of loads in flight.  The runs' partial tiles are added in index order by wgrad_finish_kernel.
struct WgArgs {
  const float* P; const void* Q; float* part;
  int N, Np, Cg, Ca, relu, slabs, spb;
};

template <bool X2>
__global__ __launch_bounds__(256) void pointnet_wgrad_kernel(WgArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
  const int g0 = blockIdx.y * 128 + 64 * (wave >> 1) + l31, a0 = blockIdx.z * 128 + 64 * (wave & 1) + l31;    // my columns of P and of Q (+ 32 for the second block)
  f32x16 acc[2][2];
#pragma unroll
  for (int gb = 0; gb < 2; ++gb)
#pragma unroll
    for (int ab = 0; ab < 2; ++ab)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[gb][ab][r] = 0.f;
  const int slab_begin = blockIdx.x * p.spb;
  const int slab_end = slab_begin + p.spb < p.slabs ? slab_begin + p.spb : p.slabs;
  for (int slab = slab_begin; slab < slab_end; ++slab) {
    const size_t row0 = (size_t)slab * SLAB;
    int nv = p.N - (int)(row0 % (size_t)p.Np);                     // valid rows of this slab (a slab lies inside one body)
    nv = nv < 0 ? 0 : (nv > SLAB ? SLAB : nv);
    for (int mm = 0; mm < nv; mm += 16) {
      float pg[8][2], qa[8][2];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int rl = mm + 2 * u + h;                               // < SLAB: in bounds even where it is past nv
        const size_t row = row0 + rl;
        const bool ok = rl < nv;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float pv = p.P[row * (size_t)p.Cg + g0 + 32 * e];
          float qv;
          if constexpr (X2) qv = split_load<32>((const half_t*)p.Q, row, a0 + 32 * e, p.Ca);
          else qv = ((const float*)p.Q)[row * (size_t)p.Ca + a0 + 32 * e];
          if (p.relu) qv = fmaxf(qv, 0.f);
          pg[u][e] = ok ? pv : 0.f;                                  // padding rows: whatever they hold (NaN included) never enters
          qa[u][e] = ok ? qv : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int gb = 0; gb < 2; ++gb)
#pragma unroll
          for (int ab = 0; ab < 2; ++ab) acc[gb][ab] = __builtin_amdgcn_mfma_f32_32x32x2f32(pg[u][gb], qa[u][ab], acc[gb][ab], 0, 0, 0);
    }
  }
  // accumulator layout: column = l & 31, row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)
  float* o = p.part + (size_t)blockIdx.x * p.Cg * p.Ca;
#pragma unroll
  for (int gb = 0; gb < 2; ++gb)
#pragma unroll
    for (int ab = 0; ab < 2; ++ab)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int g = g0 - l31 + 32 * gb + (r & 3) + 8 * (r >> 2) + 4 * h;
        o[(size_t)g * p.Ca + a0 + 32 * ab] = acc[gb][ab][r];
      }
}

// sum of n floats `stride` apart in index order (float64); the loads go out 16 at a time
__device__ __forceinline__ double strided_sum(const float* __restrict__ p, size_t stride, int n) {
  double s = 0.0;
  int k = 0;
  for (; k + 16 <= n; k += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = p[(size_t)(k + u) * stride];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += (double)v[u];
  }
  for (; k < n; ++k) s += (double)p[(size_t)k * stride];
  return s;
}

// part [B * spg][W] -> grp [B][W]: the slabs of a body in index order
__global__ __launch_bounds__(256) void group_sums_kernel(const float* __restrict__ part, float* __restrict__ grp, int spg, int W, long long total) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long long b = t / W;
  grp[t] = (float)strided_sum(part + (size_t)b * spg * W + (t - b * W), (size_t)W, spg);
}

// grp [B][W] -> the bodies in index order.  lift == 0: out0 [W].  lift == 1 (W = 4 C, entries (x, y, z, 1) per column): out0 = gW [C][3], out1 = gb [C]
__global__ __launch_bounds__(256) void total_sums_kernel(const float* __restrict__ grp, float* __restrict__ out0, float* __restrict__ out1, int B, int W, int lift) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= W) return;
  const float s = (float)strided_sum(grp + t, (size_t)W, B);
  if (!lift) out0[t] = s;
  else if ((t & 3) < 3) { if (out0) out0[(t >> 2) * 3 + (t & 3)] = s; }
  else if (out1) out1[t >> 2] = s;
}

// part [nsplit][Cg][Ca] -> out [Cg][ld_out]: the runs in index order
__global__ __launch_bounds__(256) void wgrad_finish_kernel(const float* __restrict__ part, float* __restrict__ out, int ld_out, int Cg, int Ca, int nsplit) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Cg * Ca) return;
  out[(size_t)(t / Ca) * ld_out + t % Ca] = (float)strided_sum(part + t, (size_t)Cg * Ca, nsplit);
}

int check_geo(int B, int N, int Np, int C) {
  EHM_CHECK_ARG(B > 0 && N > 0 && Np >= N && Np % SLAB == 0 && C > 0 && C % CW == 0);
  EHM_CHECK_ARG((int64_t)B * (Np / SLAB) < (1ll << 31) && C / CW < 65536);
  return 0;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int64_t ws_floats(int B, int Np, int C) { return ((int64_t)B * (Np / SLAB) + B) * C * 4; }

dim3 slab_grid(int B, int Np, int C) { return dim3((unsigned)((int64_t)B * (Np / SLAB)), (unsigned)(C / CW)); }

// block partials [B * spg][W] in `ws` -> per-body sums (to `grp_out`, or behind the partials when only the total is wanted) and the total
void finish_sums(float* ws, int B, int spg, int W, float* grp_out, float* out0, float* out1, int lift, hipStream_t st) {
  float* grp = grp_out ? grp_out : ws + (size_t)B * spg * W;
  const long long total = (long long)B * W;
  hipLaunchKernelGGL(group_sums_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, st, ws, grp, spg, W, total);
  if (out0 || out1) hipLaunchKernelGGL(total_sums_kernel, dim3((unsigned)ceil_div(W, 256)), dim3(256), 0, st, grp, out0, out1, B, W, lift);
}

// split-K plan of the weight-gradient kernel: at most 256 runs of whole slabs, a function of the shape alone (the same bits on every device)
void wgrad_plan(int B, int Np, int* slabs, int* spb, int* nsplit) {
  *slabs = B * (Np / SLAB);
  *spb = (int)ceil_div(*slabs, 256);
  *nsplit = (int)ceil_div(*slabs, *spb);
}

}  // namespace

extern "C" int ehm_pointnet_bwd_workspace_bytes(int B, int N_padded, int C, int64_t* bytes) {
  EHM_CHECK_ARG(bytes != nullptr);
  const int rc = check_geo(B, 1, N_padded, C);
  if (rc != 0) return rc;
  *bytes = ws_floats(B, N_padded, C) * (int64_t)sizeof(float);
  return 0;
}

#define EHM_POINTNET_WS(B, Np, C) \
  EHM_CHECK_ARG(workspace && al16(workspace) && workspace_bytes >= ws_floats(B, Np, C) * (int64_t)sizeof(float))

extern "C" int ehm_pointnet_pool_argmax(const void* net, int x2, int32_t* arg, int B, int N, int N_padded, int C, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
  const int rc = check_geo(B, N, N_padded, C);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(net && arg && al16(net) && (x2 == 0 || x2 == 1));
  EHM_POINTNET_WS(B, N_padded, C);
  const Geo g{N, N_padded, C};
  const int spg = N_padded / SLAB;
  float* pv = (float*)workspace;
  int* pr = (int*)(pv + (size_t)B * spg * C);
  if (x2) hipLaunchKernelGGL(pool_argmax_slab_kernel<true>, slab_grid(B, N_padded, C), dim3(256), 0, (hipStream_t)stream, net, pv, pr, g);
  else hipLaunchKernelGGL(pool_argmax_slab_kernel<false>, slab_grid(B, N_padded, C), dim3(256), 0, (hipStream_t)stream, net, pv, pr, g);
  const long long total = (long long)B * C;
  hipLaunchKernelGGL(pool_argmax_finish_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, pv, pr, arg, spg, C, total);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_pointnet_bwd_scatter(const float* gnet, const float* gpool, const int32_t* arg, float* G, float* gsum, float* gsum_group, int B, int N,
                                        int N_padded, int C, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = check_geo(B, N, N_padded, C);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(gpool && arg && G && al16(gnet) && al16(gpool) && al16(arg) && al16(G) && (const void*)gnet != (const void*)G);
  const bool sums = gsum || gsum_group;
  if (sums) EHM_POINTNET_WS(B, N_padded, C);
  const Geo g{N, N_padded, C};
  hipLaunchKernelGGL(pointnet_scatter_kernel, slab_grid(B, N_padded, C), dim3(256), 0, (hipStream_t)stream, gnet, gpool, arg, G,
                     sums ? (float*)workspace : nullptr, g);
  if (sums) finish_sums((float*)workspace, B, N_padded / SLAB, C, gsum_group, gsum, nullptr, 0, (hipStream_t)stream);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_pointnet_bwd_gate(const float* T, const void* act, int act_x2, const float* add, const float* t_scale, const float* add_scale,
                                     float* out, float* sum, float* sum_group, int B, int N, int N_padded, int C, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  const int rc = check_geo(B, N, N_padded, C);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(T && act && out && al16(T) && al16(act) && al16(add) && al16(out) && (act_x2 == 0 || act_x2 == 1));
  EHM_CHECK_ARG((const void*)act != (const void*)out && (const void*)add != (const void*)out && (add || !add_scale));
  const bool sums = sum || sum_group;
  if (sums) EHM_POINTNET_WS(B, N_padded, C);
  const Geo g{N, N_padded, C};
  float* part = sums ? (float*)workspace : nullptr;
  if (act_x2) hipLaunchKernelGGL(pointnet_gate_kernel<true>, slab_grid(B, N_padded, C), dim3(256), 0, (hipStream_t)stream, T, act, add, t_scale, add_scale, out, part, g);
  else hipLaunchKernelGGL(pointnet_gate_kernel<false>, slab_grid(B, N_padded, C), dim3(256), 0, (hipStream_t)stream, T, act, add, t_scale, add_scale, out, part, g);
  if (sums) finish_sums(part, B, N_padded / SLAB, C, sum_group, sum, nullptr, 0, (hipStream_t)stream);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_pointnet_bwd_net0(const float* pts, const float* Wpos, const float* bpos, float* net0, float* relu_net0, int B, int N, int N_padded,
                                     int C, void* stream) {
  const int rc = check_geo(B, N, N_padded, C);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(pts && Wpos && bpos && (net0 || relu_net0) && al16(net0) && al16(relu_net0));
  const Geo g{N, N_padded, C};
  hipLaunchKernelGGL(pointnet_net0_kernel, slab_grid(B, N_padded, C), dim3(256), 0, (hipStream_t)stream, pts, Wpos, bpos, net0, relu_net0, g);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_pointnet_bwd_lift(const float* X, const float* pts, const float* Wpos, float* gW, float* gb, float* gp, int B, int N, int N_padded,
                                     int C, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = check_geo(B, N, N_padded, C);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(X && pts && al16(X) && (gW || gb || gp) && (!gp || Wpos));
  EHM_POINTNET_WS(B, N_padded, C);
  const Geo g{N, N_padded, C};
  const int spg = N_padded / SLAB;
  hipLaunchKernelGGL(pointnet_lift_bwd_kernel, dim3((unsigned)((int64_t)B * spg)), dim3(256), 0, (hipStream_t)stream, X, pts, Wpos, gp,
                     (float*)workspace, g);
  if (gW || gb) finish_sums((float*)workspace, B, spg, 4 * C, nullptr, gW, gb, 1, (hipStream_t)stream);
  EHM_LAUNCH_CHECK();
  return 0;
}

extern "C" int ehm_pointnet_bwd_wgrad_workspace_bytes(int B, int N_padded, int Cg, int Ca, int64_t* bytes) {
  EHM_CHECK_ARG(bytes != nullptr);
  int rc = check_geo(B, 1, N_padded, Cg);
  if (rc == 0) rc = check_geo(B, 1, N_padded, Ca);
  if (rc != 0) return rc;
  int slabs, spb, nsplit;
  wgrad_plan(B, N_padded, &slabs, &spb, &nsplit);
  *bytes = (int64_t)nsplit * Cg * Ca * (int64_t)sizeof(float);
  return 0;
}

extern "C" int ehm_pointnet_bwd_wgrad(const float* P, const void* Q, int q_x2, int q_relu, float* out, int ld_out, int B, int N, int N_padded, int Cg,
                                      int Ca, void* workspace, int64_t workspace_bytes, void* stream) {
  int rc = check_geo(B, N, N_padded, Cg);
  if (rc == 0) rc = check_geo(B, N, N_padded, Ca);
  if (rc != 0) return rc;
  EHM_CHECK_ARG(P && Q && out && ld_out >= Ca && (q_x2 == 0 || q_x2 == 1) && (q_relu == 0 || q_relu == 1) && (int64_t)Cg * Ca < (1ll << 31));
  WgArgs a;
  int nsplit;
  wgrad_plan(B, N_padded, &a.slabs, &a.spb, &nsplit);
  EHM_CHECK_ARG(workspace && al16(workspace) && workspace_bytes >= (int64_t)nsplit * Cg * Ca * (int64_t)sizeof(float));
  a.P = P; a.Q = Q; a.part = (float*)workspace;
  a.N = N; a.Np = N_padded; a.Cg = Cg; a.Ca = Ca; a.relu = q_relu;
  const dim3 grid((unsigned)nsplit, (unsigned)(Cg / 128), (unsigned)(Ca / 128));
  if (q_x2) hipLaunchKernelGGL(pointnet_wgrad_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(pointnet_wgrad_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(wgrad_finish_kernel, dim3((unsigned)ceil_div((int64_t)Cg * Ca, 256)), dim3(256), 0, (hipStream_t)stream, a.part, out, ld_out, Cg, Ca, nsplit);
  EHM_LAUNCH_CHECK();
  return 0;
}
