// The stage-1 and stage-2 scene clouds on gfx950: the offline preprocessing of the reference (preprocess_scene_s1.py:94-118, whole scene;
// preprocess_scene_s2_for_test.py:176-208, the cube around the stage-1 translation) followed by its loaders' transform
// (dataloaders/egobody_dataset.py:205-225, :273), per item, from scene meshes resident on the device.
//
// select(pred, target) = "the vertices where pred holds, in mesh order, every k-th of them (open3d's uniform_down_sample keeps 0, k, 2k, ...),
// the first `target`", k = int(n / target), is an ordered compaction.  It runs in up to five launches, with no atomics on the ordering path:
//   scene_ymin_kernel     (cube only) per tile and item: min y over the xz-selected vertices (+inf when none)
//   scene_reduce_kernel   (cube only) per item: ymin over its tiles, thresh = ymin + cube_size (+inf: the xz crop is empty)
//   scene_count_kernel    per tile and item: how many vertices pass the full predicate (wave64 ballot + popcount)
//   scene_scan_kernel     per item (one wave): exclusive scan of the tile counts in place; n_selected, k = n / target and the status word
//   scene_scatter_kernel  per tile and item: predicate again, rank = tile offset + per-(chunk, wave) offset in LDS + mbcnt of the ballot;
//                         ranks r with r % k == 0 and r / k < target are rows r / k, of which every stride-th is written, as T_out v in f32
// A block is one tile (2048 vertices: 8 chunks of 256) x one group of up to 8 items of the SAME mesh: each vertex is loaded once per pass for
// the whole group.  The predicates reproduce numpy's float64 arithmetic bit for bit: separately rounded operations in the reference's order
// (the pragma below keeps the compiler from contracting them into FMAs); every scalar the host can derive (cos, sin, centre, bounds) comes in
// as a double computed there exactly as the reference writes it.
#include "common.h"
#include "egohmr_hip.h"

#pragma clang fp contract(off)

namespace {

// separately rounded float64 operations.  (The header's __dadd_rn / __dmul_rn are plain `+` / `*` compiled under the default fast contraction:
// inlined here, their fmul / fadd carry the `contract` flag and the backend fuses them into v_fma_f64.  Written in this file, under the pragma
// above, they do not.)
__device__ inline double dadd(double a, double b) { return a + b; }
__device__ inline double dsub(double a, double b) { return a - b; }
__device__ inline double dmul(double a, double b) { return a * b; }

constexpr int kThreads = 256;
constexpr int kChunks = 8;
constexpr int kTile = kThreads * kChunks;     // vertices per tile
constexpr int kG = EHM_SCENE_GROUP;           // items per group
constexpr int kP = EHM_SCENE_PARAMS;          // doubles per item
constexpr int kWaves = kThreads / 64;

struct Ws {
  double* tile_ymin;   // [B, max_tiles]
  int32_t* tile_cnt;   // [B, max_tiles]: counts, then (scan) exclusive offsets
  double* thresh;      // [B]: ymin + cube_size (cube)
  int32_t* k;          // [B]
};

__host__ __device__ inline int64_t max_tiles_of(int64_t max_verts) { return (max_verts + kTile - 1) / kTile; }
__host__ __device__ inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

__host__ __device__ inline int64_t ws_bytes(int B, int64_t max_verts) {
  const int64_t mt = max_tiles_of(max_verts);
  return align256((int64_t)B * mt * 8) + align256((int64_t)B * mt * 4) + align256((int64_t)B * 8) + align256((int64_t)B * 4);
}

__host__ __device__ inline Ws ws_of(const ehm_scene_desc& d) {
  const int64_t mt = max_tiles_of(d.max_mesh_verts);
  char* p = (char*)d.workspace;
  Ws w;
  w.tile_ymin = (double*)p; p += align256((int64_t)d.B * mt * 8);
  w.tile_cnt = (int32_t*)p; p += align256((int64_t)d.B * mt * 4);
  w.thresh = (double*)p; p += align256((int64_t)d.B * 8);
  w.k = (int32_t*)p;
  return w;
}

// the group's items (the first n are valid), its mesh's first vertex and vertex count; false: nothing for this block to do
__device__ inline bool group_of(const ehm_scene_desc& d, int grp, int items[kG], int& n, int64_t& base, int64_t& nv) {
  const int32_t* g = d.groups + (int64_t)grp * (1 + kG);
  const int m = g[0];
  if (m < 0 || m >= d.num_meshes) return false;
  base = d.mesh_offsets[m];
  nv = d.mesh_offsets[m + 1] - base;
  if (nv <= 0 || nv > d.max_mesh_verts || base < 0 || base + nv > d.total_verts) return false;
  n = 0;
#pragma unroll
  for (int i = 0; i < kG; ++i) {
    const int it = g[1 + i];
    items[i] = it;
    if (it >= 0 && it < d.B && n == i) n = i + 1;
  }
  return n > 0;
}

// one affine row: ((m0 x + m1 y) + m2 z) + m3, each operation rounded (open3d's transform of [p, 1], w = 1)
__device__ inline double row4(const double* m, double x, double y, double z) {
  return dadd(dadd(dadd(dmul(m[0], x), dmul(m[1], y)), dmul(m[2], z)), m[3]);
}

// preprocess_scene_s1.py:102-109: the chain of mesh.transform calls, then z > 0
__device__ inline bool pred_whole(const double* p, int K, double x, double y, double z) {
  for (int c = 0; c < K; ++c) {
    const double* m = p + EHM_SCENE_P_CHAIN + 12 * c;
    const double nx = row4(m, x, y, z), ny = row4(m + 4, x, y, z), nz = row4(m + 8, x, y, z);
    x = nx; y = ny; z = nz;
  }
  return z > 0.0;
}

// preprocess_scene_s2_for_test.py:185-196: rotation about y through the centre, inclusive xz bounds
__device__ inline bool pred_xz(const double* p, double x, double z) {
  const double c = p[EHM_SCENE_P_COS], s = p[EHM_SCENE_P_SIN], cx = p[EHM_SCENE_P_CX], cz = p[EHM_SCENE_P_CZ];
  const double dx = dsub(x, cx), dz = dsub(z, cz);
  const double xr = dadd(dsub(dmul(dx, c), dmul(dz, s)), cx);
  const double zr = dadd(dadd(dmul(dx, s), dmul(dz, c)), cz);
  return xr >= p[EHM_SCENE_P_XMIN] && xr <= p[EHM_SCENE_P_XMAX] && zr >= p[EHM_SCENE_P_ZMIN] && zr <= p[EHM_SCENE_P_ZMAX];
}

struct Verts {
  double x[kChunks], y[kChunks], z[kChunks];
  unsigned valid;   // bit j: chunk j's vertex exists
};

__device__ inline Verts load_tile(const ehm_scene_desc& d, int64_t base, int64_t nv, int64_t tile) {
  Verts v;
  v.valid = 0;
  const double* X = d.verts;
  const double* Y = d.verts + d.total_verts;
  const double* Z = d.verts + 2 * d.total_verts;
#pragma unroll
  for (int j = 0; j < kChunks; ++j) {
    const int64_t i = tile * kTile + j * kThreads + threadIdx.x;
    if (i < nv) {
      v.x[j] = X[base + i]; v.y[j] = Y[base + i]; v.z[j] = Z[base + i];
      v.valid |= 1u << j;
    } else {
      v.x[j] = v.y[j] = v.z[j] = 0.0;
    }
  }
  return v;
}

// the group's per-item parameters into LDS (+ thresh and k from the workspace when asked)
__device__ inline void load_params(const ehm_scene_desc& d, const int items[kG], int n, double (*p_s)[kP]) {
  for (int e = threadIdx.x; e < kG * kP; e += kThreads) {
    const int g = e / kP;
    if (g < n) p_s[g][e % kP] = d.params[(int64_t)items[g] * kP + e % kP];
  }
}

// the full predicate of item g for the tile's vertices: bit j = chunk j's vertex is selected
__device__ inline unsigned full_bits(const ehm_scene_desc& d, const double* p, double thresh, const Verts& v) {
  unsigned bits = 0;
#pragma unroll
  for (int j = 0; j < kChunks; ++j) {
    bool sel;
    if (d.mode == EHM_SCENE_WHOLE) sel = pred_whole(p, d.chain_len, v.x[j], v.y[j], v.z[j]);
    else sel = pred_xz(p, v.x[j], v.z[j]) && v.y[j] <= thresh;   // :197
    if (sel && (v.valid >> j & 1u)) bits |= 1u << j;
  }
  return bits;
}

__device__ inline double wave_min_d(double m) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmin(m, __shfl_xor(m, o, 64));
  return m;
}

__global__ __launch_bounds__(kThreads) void scene_ymin_kernel(const ehm_scene_desc d) {
  __shared__ double p_s[kG][kP];
  __shared__ double red_s[kG][kWaves];
  int items[kG], n;
  int64_t base, nv;
  const int64_t tile = blockIdx.x;
  if (!group_of(d, blockIdx.y, items, n, base, nv) || tile * kTile >= nv) return;
  load_params(d, items, n, p_s);
  const Verts v = load_tile(d, base, nv, tile);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int g = 0; g < n; ++g) {
    double m = __builtin_huge_val();
#pragma unroll
    for (int j = 0; j < kChunks; ++j)
      if ((v.valid >> j & 1u) && pred_xz(p_s[g], v.x[j], v.z[j])) m = fmin(m, v.y[j]);
    m = wave_min_d(m);
    if (lane == 0) red_s[g][wave] = m;
  }
  __syncthreads();
  if ((int)threadIdx.x < n) {
    const int g = threadIdx.x;
    double m = red_s[g][0];
    for (int w = 1; w < kWaves; ++w) m = fmin(m, red_s[g][w]);
    ws_of(d).tile_ymin[(int64_t)items[g] * max_tiles_of(d.max_mesh_verts) + tile] = m;
  }
}

// one wave per item: items w and w + 4 of the group
__global__ __launch_bounds__(kThreads) void scene_reduce_kernel(const ehm_scene_desc d) {
  int items[kG], n;
  int64_t base, nv;
  if (!group_of(d, blockIdx.x, items, n, base, nv)) return;
  const Ws w = ws_of(d);
  const int64_t mt = max_tiles_of(d.max_mesh_verts), nt = max_tiles_of(nv);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int g = wave; g < n; g += kWaves) {
    const double* t = w.tile_ymin + (int64_t)items[g] * mt;
    double m = __builtin_huge_val();
    for (int64_t i = lane; i < nt; i += 64) m = fmin(m, t[i]);
    m = wave_min_d(m);
    if (lane == 0) w.thresh[items[g]] = dadd(m, d.params[(int64_t)items[g] * kP + EHM_SCENE_P_CUBE]);   // np.min(..) + cube_size
  }
}

__global__ __launch_bounds__(kThreads) void scene_count_kernel(const ehm_scene_desc d) {
  __shared__ double p_s[kG][kP];
  __shared__ double th_s[kG];
  __shared__ int cnt_s[kG][kWaves];
  int items[kG], n;
  int64_t base, nv;
  const int64_t tile = blockIdx.x;
  if (!group_of(d, blockIdx.y, items, n, base, nv) || tile * kTile >= nv) return;
  const Ws w = ws_of(d);
  load_params(d, items, n, p_s);
  if ((int)threadIdx.x < n) th_s[threadIdx.x] = d.mode == EHM_SCENE_CUBE ? w.thresh[items[threadIdx.x]] : 0.0;
  const Verts v = load_tile(d, base, nv, tile);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int g = 0; g < n; ++g) {
    const unsigned bits = full_bits(d, p_s[g], th_s[g], v);
    int c = 0;
#pragma unroll
    for (int j = 0; j < kChunks; ++j) c += __popcll(__ballot(bits >> j & 1u));
    if (lane == 0) cnt_s[g][wave] = c;
  }
  __syncthreads();
  if ((int)threadIdx.x < n) {
    const int g = threadIdx.x;
    int c = 0;
    for (int q = 0; q < kWaves; ++q) c += cnt_s[g][q];
    w.tile_cnt[(int64_t)items[g] * max_tiles_of(d.max_mesh_verts) + tile] = c;
  }
}

// one wave per item: each lane scans a contiguous run of tiles, the lanes' sums are scanned across the wave
__global__ __launch_bounds__(kThreads) void scene_scan_kernel(const ehm_scene_desc d) {
  int items[kG], n;
  int64_t base, nv;
  if (!group_of(d, blockIdx.x, items, n, base, nv)) return;
  const Ws w = ws_of(d);
  const int64_t mt = max_tiles_of(d.max_mesh_verts), nt = max_tiles_of(nv);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t per = (nt + 63) / 64, lo = min((int64_t)lane * per, nt), hi = min(lo + per, nt);
  for (int g = wave; g < n; g += kWaves) {
    const int it = items[g];
    int32_t* t = w.tile_cnt + (int64_t)it * mt;
    int s = 0;
    for (int64_t i = lo; i < hi; ++i) s += t[i];
    int incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    int run = incl - s;
    for (int64_t i = lo; i < hi; ++i) {
      const int c = t[i];
      t[i] = run;
      run += c;
    }
    const int total = __shfl(incl, 63, 64);
    if (lane == 0) {
      const int k = total / d.target;
      int st = k == 0 ? EHM_SCENE_TOO_FEW : EHM_SCENE_OK;
      if (d.mode == EHM_SCENE_CUBE && __builtin_isinf(w.thresh[it])) st = EHM_SCENE_EMPTY_CROP;   // np.min of an empty crop raises
      w.k[it] = st == EHM_SCENE_OK ? k : 0;
      d.n_selected[it] = total;
      d.status[it] = st;
    }
  }
}

__global__ __launch_bounds__(kThreads) void scene_scatter_kernel(const ehm_scene_desc d) {
  __shared__ double p_s[kG][kP];
  __shared__ double th_s[kG];
  __shared__ int k_s[kG];
  __shared__ int pre_s[kG][kChunks][kWaves];
  int items[kG], n;
  int64_t base, nv;
  const int64_t tile = blockIdx.x;
  if (!group_of(d, blockIdx.y, items, n, base, nv) || tile * kTile >= nv) return;
  const Ws w = ws_of(d);
  const int64_t mt = max_tiles_of(d.max_mesh_verts);
  load_params(d, items, n, p_s);
  if ((int)threadIdx.x < n) {
    th_s[threadIdx.x] = d.mode == EHM_SCENE_CUBE ? w.thresh[items[threadIdx.x]] : 0.0;
    k_s[threadIdx.x] = w.k[items[threadIdx.x]];
  }
  const Verts v = load_tile(d, base, nv, tile);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned bits[kG];
#pragma unroll
  for (int g = 0; g < kG; ++g) {
    bits[g] = 0;
    if (g < n && k_s[g] > 0) {
      bits[g] = full_bits(d, p_s[g], th_s[g], v);
#pragma unroll
      for (int j = 0; j < kChunks; ++j) {
        const int c = __popcll(__ballot(bits[g] >> j & 1u));
        if (lane == 0) pre_s[g][j][wave] = c;
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < n && k_s[threadIdx.x] > 0) {     // exclusive prefix in (chunk, wave) order = mesh order inside the tile
    const int g = threadIdx.x;
    int run = w.tile_cnt[(int64_t)items[g] * mt + tile];
    for (int j = 0; j < kChunks; ++j)
      for (int q = 0; q < kWaves; ++q) {
        const int c = pre_s[g][j][q];
        pre_s[g][j][q] = run;
        run += c;
      }
  }
  __syncthreads();
  const int rows = (d.target + d.stride - 1) / d.stride;
#pragma unroll
  for (int g = 0; g < kG; ++g) {
    if (g >= n || k_s[g] <= 0) continue;
    const int k = k_s[g], it = items[g];
    const double* T = p_s[g] + EHM_SCENE_P_OUT;
#pragma unroll
    for (int j = 0; j < kChunks; ++j) {
      const unsigned long long m = __ballot(bits[g] >> j & 1u);
      if (!(bits[g] >> j & 1u)) continue;
      const int r = pre_s[g][j][wave] + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      if (r % k != 0) continue;
      const int row = r / k;
      if (row >= d.target || row % d.stride != 0) continue;
      const int64_t o = (int64_t)it * rows + row / d.stride;
      const double x = v.x[j], y = v.y[j], z = v.z[j];
      d.points[o * 3 + 0] = (float)row4(T, x, y, z);
      d.points[o * 3 + 1] = (float)row4(T + 4, x, y, z);
      d.points[o * 3 + 2] = (float)row4(T + 8, x, y, z);
      if (d.index) d.index[o] = tile * kTile + j * kThreads + threadIdx.x;
    }
  }
}

int check_desc(const ehm_scene_desc* d) {
  EHM_CHECK_ARG(d && d->verts && d->mesh_offsets && d->groups && d->params && d->points && d->n_selected && d->status);
  EHM_CHECK_ARG(d->mode == EHM_SCENE_WHOLE || d->mode == EHM_SCENE_CUBE);
  EHM_CHECK_ARG(d->mode == EHM_SCENE_CUBE || (d->chain_len >= 1 && d->chain_len <= EHM_SCENE_MAX_CHAIN));
  EHM_CHECK_ARG(d->B > 0 && d->num_groups > 0 && d->num_groups <= 65535 && d->num_meshes > 0 && d->target > 0 && d->stride > 0);
  EHM_CHECK_ARG(d->max_mesh_verts > 0 && d->max_mesh_verts <= INT32_MAX - kTile && d->total_verts >= d->max_mesh_verts);
  return 0;
}

}  // namespace

extern "C" int ehm_scene_workspace_bytes(const ehm_scene_desc* d, int64_t* bytes) {
  EHM_CHECK_ARG(bytes);
  if (int rc = check_desc(d)) return rc;
  *bytes = ws_bytes(d->B, d->max_mesh_verts);
  return 0;
}

extern "C" int ehm_scene_select(const ehm_scene_desc* d, void* stream) {
  if (int rc = check_desc(d)) return rc;
  EHM_CHECK_ARG(d->workspace && d->workspace_bytes >= ws_bytes(d->B, d->max_mesh_verts));
  hipStream_t st = (hipStream_t)stream;
  const dim3 tiles((unsigned)max_tiles_of(d->max_mesh_verts), (unsigned)d->num_groups), groups((unsigned)d->num_groups), blk(kThreads);
  if (d->mode == EHM_SCENE_CUBE) {
    hipLaunchKernelGGL(scene_ymin_kernel, tiles, blk, 0, st, *d);
    EHM_LAUNCH_CHECK();
    hipLaunchKernelGGL(scene_reduce_kernel, groups, blk, 0, st, *d);
    EHM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(scene_count_kernel, tiles, blk, 0, st, *d);
  EHM_LAUNCH_CHECK();
  hipLaunchKernelGGL(scene_scan_kernel, groups, blk, 0, st, *d);
  EHM_LAUNCH_CHECK();
  hipLaunchKernelGGL(scene_scatter_kernel, tiles, blk, 0, st, *d);
  EHM_LAUNCH_CHECK();
  return 0;
}
