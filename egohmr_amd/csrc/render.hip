// A software mesh rasteriser on gfx950 for the reference's overlays (utils/renderer.py:15-47, drawn there by pyrender): the rule of
// include/egohmr_hip.h (ehm_render), in six launches on the caller's stream:
//   vertex_kernel        per (item, vertex): projection, the "usable" flag, the smooth normal by the vertex -> face CSR gather
//   face_kernel          per (item, face): the drop tests, the 64-byte record (projected vertices, 1/z, area, edge vectors), and the count of the
//                        face in every 64 x 16 pixel tile its bounding box touches
//   scan_kernel          per item: the tiles' list offsets, the needed capacity, the overflow decision, the list of tiles that have a face
//   fill_kernel          per (item, face): the face's index into its tiles' lists
//   tile_kernel<true>    per (item, tile with a face): the background tile into LDS, the list streamed through LDS in chunks of 128 records, four pixels
//                        per lane with (z, face index) in registers (a wave owns a 16 x 16 region and skips a face by its box, wave-uniformly,
//                        before any edge function), shading of the winners, every output written once
//   tile_kernel<false>   per (item, tile without a face): the background copy, depth 0, face index -1
// With clip_near a face that straddles the near plane gets a second kind of record (the plane coefficients of the header's homogeneous rule, D, its
// binning box) in the same 64 bytes: face_kernel writes it from the raw vertices, fill_kernel and the LDS staging take its box from it, and
// tile_kernel<true, CLIP = true> evaluates a second coverage / depth body for it - the kind belongs to the face, so that branch is wave-uniform like
// the others.  Without clip_near the CLIP = false instance runs, which has no second body.
// The only atomics are integer ones on the tile counters: they decide the ORDER of a list, and the winner of a pixel is the minimum of
// (z, face index), which no order changes.  Every float operation is rounded on its own (the pragma below), so the arithmetic is the header's
// formula operation by operation and does not depend on where the compiler would have fused.
// Both tile launches have one block per tile of the image, because how many tiles have a face is known on the device only; a block with nothing to
// do leaves after two loads.  The tiles with a face go first and by their work list, so that the blocks that rasterise are dispatched together.  On the
// benchmark's mesh that did not pay by itself (one tile per body holds 2479 faces, and the launch is as long as that tile: docs/EXPERIMENTS.md R25.2).
#include "common.h"
#include "egohmr_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTW = 64, kTH = 16;        // tile: one wave owns 16 x 16 pixels of it, a lane four pixels of one column
constexpr int kRows = kTH / 4;           // pixels per lane
constexpr int kChunk = 128;              // records per LDS chunk (8 KiB)
constexpr int kRowBytes = kTW * 3;

// record: q0 = (u0, v0, u1, v1), q1 = (u2, v2, 1/z0, 1/z1), q2 = (1/z2, area, a0x, a0y), q3 = (a1x, a1y, a2x, a2y); a_k = p_{k+1} - p_k.
// area == 0 marks a dropped face.
// record of a crossing face (clip_near): q0 = (c0x, c0y, c0z, c1x), q1 = (c1y, c1z, c2x, c2y), q2 = (c2z, D, umin, umax), q3 = (vmin, vmax, 0, tag) with
// c_k = g_{k+1} x g_{k+2} the plane coefficients of E_k and (umin .. vmax) the binning box; D == 0 marks a dropped face in the same slot as area.
// The tag is a NaN's bit pattern: the other kind holds a2y = v0 - v2 there, a difference of two finite numbers, which is never a NaN.  A record is
// read by whole waves (one face at a time), so its kind is wave-uniform.
constexpr unsigned kCrossTag = 0x7fc0c11bu;
struct Layout {
  int64_t proj, vnorm, rec, count, cursor, offset, work, nwork, list, total;
  int ntx, nty;
  int64_t nt;
};

inline Layout layout_of(const ehm_render_desc& d) {
  Layout L;
  L.ntx = (int)ceil_div(d.W, kTW);
  L.nty = (int)ceil_div(d.H, kTH);
  L.nt = (int64_t)L.ntx * L.nty;
  int64_t at = 0;
  auto take = [&](int64_t bytes) {
    const int64_t p = at;
    at += round_up(bytes, 256);
    return p;
  };
  L.proj = take((int64_t)d.B * d.V * 16);
  L.vnorm = take(d.smooth ? (int64_t)d.B * d.V * 12 : 0);
  L.rec = take((int64_t)d.B * d.F * 64);
  L.count = take((int64_t)d.B * L.nt * 4);     // count and cursor are cleared by one memset: keep them adjacent
  L.cursor = take((int64_t)d.B * L.nt * 4);
  L.offset = take((int64_t)d.B * L.nt * 4);
  L.work = take((int64_t)d.B * L.nt * 4);      // per item: the tiles with a face, ascending
  L.nwork = take((int64_t)d.B * 4);
  L.list = take((int64_t)d.B * d.bin_capacity * 4);
  L.total = at;
  return L;
}

struct Params {
  ehm_render_desc d;
  float4* proj;
  float* vnorm;
  f32x4* rec;
  int* count;
  int* cursor;
  int* offset;
  int* work;
  int* nwork;
  int* list;
  int ntx, nty;
  int aligned16;
};

__device__ inline bool finite3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }

__device__ inline void cross_of(const float* __restrict__ verts, int i0, int i1, int i2, float n[3]) {
  const float* p0 = verts + (int64_t)i0 * 3;
  const float* p1 = verts + (int64_t)i1 * 3;
  const float* p2 = verts + (int64_t)i2 * 3;
  const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
  const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
  n[0] = ay * bz - az * by;
  n[1] = az * bx - ax * bz;
  n[2] = ax * by - ay * bx;
}

__global__ __launch_bounds__(kThreads) void vertex_kernel(const Params p) {
  const ehm_render_desc& d = p.d;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= d.V) return;
  const int b = blockIdx.y;
  const float* verts = d.vertices + (int64_t)b * d.V * 3;
  const float x = verts[(int64_t)i * 3], y = verts[(int64_t)i * 3 + 1], z = verts[(int64_t)i * 3 + 2];
  float u = 0.0f, v = 0.0f;
  bool ok = finite3(x, y, z) && z > d.z_near;
  if (ok) {
    u = d.fx[b] * x / z + d.cx[b];
    v = d.fy[b] * y / z + d.cy[b];
    ok = isfinite(u) && isfinite(v);
  }
  p.proj[(int64_t)b * d.V + i] = make_float4(u, v, z, ok ? 1.0f : 0.0f);
  if (!d.smooth) return;
  float n[3] = {0.0f, 0.0f, 0.0f};
  const int hi3 = 3 * d.F;
  int j0 = d.vf_offsets[i], j1 = d.vf_offsets[i + 1];
  j0 = j0 < 0 ? 0 : j0;
  j1 = j1 > hi3 ? hi3 : j1;
  for (int j = j0; j < j1; ++j) {
    const int f = d.vf_faces[j];
    if (f < 0 || f >= d.F) continue;
    const int i0 = d.faces[(int64_t)f * 3], i1 = d.faces[(int64_t)f * 3 + 1], i2 = d.faces[(int64_t)f * 3 + 2];
    if ((unsigned)i0 >= (unsigned)d.V || (unsigned)i1 >= (unsigned)d.V || (unsigned)i2 >= (unsigned)d.V) continue;
    float c[3];
    cross_of(verts, i0, i1, i2, c);
    if (!finite3(c[0], c[1], c[2])) continue;
    n[0] += c[0];
    n[1] += c[1];
    n[2] += c[2];
  }
  float* o = p.vnorm + ((int64_t)b * d.V + i) * 3;
  o[0] = n[0];
  o[1] = n[1];
  o[2] = n[2];
}

// The tiles a face's bounding box touches: the samples (j + 0.5, i + 0.5) inside the box, padded by a pixel (the edge functions decide, the box
// only has to be conservative), clamped to the image IN FLOAT before any conversion to int.  false: no sample of the image is inside.
__device__ inline bool tile_range(float umin, float umax, float vmin, float vmax, int W, int H, int* tx0, int* tx1, int* ty0, int* ty1) {
  const float x0 = fmaxf(floorf(umin - 0.5f), 0.0f), x1 = fminf(ceilf(umax - 0.5f), (float)(W - 1));
  const float y0 = fmaxf(floorf(vmin - 0.5f), 0.0f), y1 = fminf(ceilf(vmax - 0.5f), (float)(H - 1));
  if (!(x0 <= x1 && y0 <= y1)) return false;
  *tx0 = (int)x0 / kTW;
  *tx1 = (int)x1 / kTW;
  *ty0 = (int)y0 / kTH;
  *ty1 = (int)y1 / kTH;
  return true;
}

__device__ inline bool is_crossing(const f32x4 q3) { return __float_as_uint(q3[3]) == kCrossTag; }

// (umin, umax, vmin, vmax) of a record: of its three projected vertices, or what face_kernel stored for a crossing face.
__device__ inline f32x4 box_of(const f32x4 q0, const f32x4 q1, const f32x4 q2, const f32x4 q3) {
  if (is_crossing(q3)) return f32x4{q2[2], q2[3], q3[0], q3[1]};
  return f32x4{fminf(fminf(q0[0], q0[2]), q1[0]), fmaxf(fmaxf(q0[0], q0[2]), q1[0]), fminf(fminf(q0[1], q0[3]), q1[1]), fmaxf(fmaxf(q0[1], q0[3]), q1[1])};
}

// The record of a crossing face (the header's near-plane rule), from its raw vertices: proj holds nothing for a vertex behind the plane.  The caller
// has checked the indices.  false: the face is not crossing, or is dropped.
__device__ inline bool crossing_record(const ehm_render_desc& d, int b, int i0, int i1, int i2, f32x4* q0, f32x4* q1, f32x4* q2, f32x4* q3) {
  const float* verts = d.vertices + (int64_t)b * d.V * 3;
  const int idx[3] = {i0, i1, i2};
  float x[3], y[3], z[3];
  int front = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    x[k] = verts[(int64_t)idx[k] * 3];
    y[k] = verts[(int64_t)idx[k] * 3 + 1];
    z[k] = verts[(int64_t)idx[k] * 3 + 2];
    if (!finite3(x[k], y[k], z[k])) return false;
    front += z[k] > d.z_near;
  }
  if (front == 0 || front == 3) return false;
  const float fx = d.fx[b], fy = d.fy[b], cx = d.cx[b], cy = d.cy[b];
  float gx[3], gy[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    gx[k] = fx * x[k];
    gy[k] = fy * y[k];
  }
  float c[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = (k + 1) % 3, j = (k + 2) % 3;
    c[k][0] = gy[i] * z[j] - z[i] * gy[j];
    c[k][1] = z[i] * gx[j] - gx[i] * z[j];
    c[k][2] = gx[i] * gy[j] - gy[i] * gx[j];
  }
  const float D = (gx[0] * c[0][0] + gy[0] * c[0][1]) + z[0] * c[0][2];
  if (!isfinite(D) || D == 0.0f || (d.cull_backface && D > 0.0f)) return false;
  // the box: the front vertices and the two points where an edge meets the plane
  float umin = __builtin_inff(), umax = -__builtin_inff(), vmin = umin, vmax = umax;
  bool finite = true;
  auto add = [&](float u, float v) {
    finite = finite && isfinite(u) && isfinite(v);
    umin = fminf(umin, u);
    umax = fmaxf(umax, u);
    vmin = fminf(vmin, v);
    vmax = fmaxf(vmax, v);
  };
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int j = (k + 1) % 3;
    if (z[k] > d.z_near) add(fx * x[k] / z[k] + cx, fy * y[k] / z[k] + cy);
    if ((z[k] > d.z_near) != (z[j] > d.z_near)) {
      const float t = (d.z_near - z[k]) / (z[j] - z[k]);
      add(fx * (x[k] + t * (x[j] - x[k])) / d.z_near + cx, fy * (y[k] + t * (y[j] - y[k])) / d.z_near + cy);
    }
  }
  if (!finite) {
    umin = 0.0f;
    umax = (float)d.W;
    vmin = 0.0f;
    vmax = (float)d.H;
  }
  *q0 = f32x4{c[0][0], c[0][1], c[0][2], c[1][0]};
  *q1 = f32x4{c[1][1], c[1][2], c[2][0], c[2][1]};
  *q2 = f32x4{c[2][2], D, umin, umax};
  *q3 = f32x4{vmin, vmax, 0.0f, __uint_as_float(kCrossTag)};
  return true;
}

__global__ __launch_bounds__(kThreads) void face_kernel(const Params p) {
  const ehm_render_desc& d = p.d;
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= d.F) return;
  const int b = blockIdx.y;
  f32x4 q0 = {0.0f, 0.0f, 0.0f, 0.0f}, q1 = q0, q2 = q0, q3 = q0;
  const int i0 = d.faces[(int64_t)f * 3], i1 = d.faces[(int64_t)f * 3 + 1], i2 = d.faces[(int64_t)f * 3 + 2];
  bool keep = (unsigned)i0 < (unsigned)d.V && (unsigned)i1 < (unsigned)d.V && (unsigned)i2 < (unsigned)d.V;
  int tx0 = 0, tx1 = -1, ty0 = 0, ty1 = -1;
  if (keep) {
    const float4 a = p.proj[(int64_t)b * d.V + i0], bb = p.proj[(int64_t)b * d.V + i1], c = p.proj[(int64_t)b * d.V + i2];
    keep = a.w != 0.0f && bb.w != 0.0f && c.w != 0.0f;
    if (keep) {
      const float a0x = bb.x - a.x, a0y = bb.y - a.y, a1x = c.x - bb.x, a1y = c.y - bb.y, a2x = a.x - c.x, a2y = a.y - c.y;
      const float area = a0x * (c.y - a.y) - a0y * (c.x - a.x);
      keep = isfinite(area) && area != 0.0f && !(d.cull_backface && area > 0.0f);
      if (keep) {
        q0 = f32x4{a.x, a.y, bb.x, bb.y};
        q1 = f32x4{c.x, c.y, 1.0f / a.z, 1.0f / bb.z};
        q2 = f32x4{1.0f / c.z, area, a0x, a0y};
        q3 = f32x4{a1x, a1y, a2x, a2y};
      }
    } else if (d.clip_near) {
      keep = crossing_record(d, b, i0, i1, i2, &q0, &q1, &q2, &q3);
    }
    if (keep) {
      const f32x4 bx = box_of(q0, q1, q2, q3);
      keep = tile_range(bx[0], bx[1], bx[2], bx[3], d.W, d.H, &tx0, &tx1, &ty0, &ty1);
      if (!keep) q2[1] = 0.0f;
    }
  }
  f32x4* r = p.rec + ((int64_t)b * d.F + f) * 4;
  r[0] = q0;
  r[1] = q1;
  r[2] = q2;
  r[3] = q3;
  if (!keep) return;
  int* cnt = p.count + (int64_t)b * p.ntx * p.nty;
  for (int ty = ty0; ty <= ty1; ++ty)
    for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(cnt + (int64_t)ty * p.ntx + tx, 1);
}

// One block per item: exclusive prefix of the tile counts (each thread a contiguous run of tiles, the 256 run sums scanned by thread 0), and the
// item's tiles that have a face, in ascending order: the work list of tile_kernel<true>.
__global__ __launch_bounds__(kThreads) void scan_kernel(const Params p) {
  __shared__ long long part[kThreads];
  __shared__ int busy[kThreads];
  __shared__ long long total;
  const int b = blockIdx.x, t = threadIdx.x;
  const int64_t nt = (int64_t)p.ntx * p.nty;
  const int* cnt = p.count + (int64_t)b * nt;
  int* off = p.offset + (int64_t)b * nt;
  const int64_t seg = (nt + kThreads - 1) / kThreads;
  const int64_t lo = t * seg < nt ? t * seg : nt, hi = lo + seg < nt ? lo + seg : nt;
  long long s = 0;
  int nz = 0;
  for (int64_t i = lo; i < hi; ++i) {
    s += cnt[i];
    nz += cnt[i] > 0;
  }
  part[t] = s;
  busy[t] = nz;
  __syncthreads();
  if (t == 0) {
    long long run = 0;
    int nrun = 0;
    for (int k = 0; k < kThreads; ++k) {
      const long long v = part[k];
      part[k] = run;
      run += v;
      const int w = busy[k];
      busy[k] = nrun;
      nrun += w;
    }
    p.nwork[b] = run > p.d.bin_capacity ? 0 : nrun;
    p.d.needed_capacity[b] = run > 0x7fffffffll ? 0x7fffffff : (int)run;
    total = run;
  }
  __syncthreads();
  if (total > p.d.bin_capacity) return;     // overflow: no list is filled or read, the offsets are not needed
  long long run = part[t];
  int* work = p.work + (int64_t)b * nt + busy[t];
  for (int64_t i = lo; i < hi; ++i) {
    off[i] = (int)run;
    run += cnt[i];
    if (cnt[i] > 0) *work++ = (int)i;
  }
}

__global__ __launch_bounds__(kThreads) void fill_kernel(const Params p) {
  const ehm_render_desc& d = p.d;
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= d.F) return;
  const int b = blockIdx.y;
  if (d.needed_capacity[b] > d.bin_capacity) return;
  const f32x4* r = p.rec + ((int64_t)b * d.F + f) * 4;
  const f32x4 q0 = r[0], q1 = r[1], q2 = r[2];
  if (q2[1] == 0.0f) return;
  const f32x4 bx = box_of(q0, q1, q2, d.clip_near ? r[3] : f32x4{0.0f, 0.0f, 0.0f, 0.0f});
  int tx0, tx1, ty0, ty1;
  if (!tile_range(bx[0], bx[1], bx[2], bx[3], d.W, d.H, &tx0, &tx1, &ty0, &ty1)) return;
  const int64_t nt = (int64_t)p.ntx * p.nty;
  const int* cnt = p.count + (int64_t)b * nt;
  int* cur = p.cursor + (int64_t)b * nt;
  const int* off = p.offset + (int64_t)b * nt;
  int* list = p.list + (int64_t)b * d.bin_capacity;
  for (int ty = ty0; ty <= ty1; ++ty)
    for (int tx = tx0; tx <= tx1; ++tx) {
      const int64_t t = (int64_t)ty * p.ntx + tx;
      const int pos = atomicAdd(cur + t, 1);
      const int64_t at = (int64_t)off[t] + pos;
      if (pos < cnt[t] && at < d.bin_capacity) list[at] = f;      // (always true: the same faces were counted; the bound is kept anyway)
    }
}

// The three edge functions of one record at the sample (px, py), as the header writes them.
__device__ inline void edges_at(const f32x4 q0, const f32x4 q1, const f32x4 q2, const f32x4 q3, float px, float py, float e[3]) {
  e[0] = q2[2] * (py - q0[1]) - q2[3] * (px - q0[0]);
  e[1] = q3[0] * (py - q0[3]) - q3[1] * (px - q0[2]);
  e[2] = q3[2] * (py - q1[1]) - q3[3] * (px - q1[0]);
}

// bg_color's byte for byte offset o of a row (a select, not an index: a runtime index into the kernel's argument would move it to scratch)
__device__ inline uint8_t bg_at(const ehm_render_desc& d, int o) {
  const int k = o % 3;
  return k == 0 ? d.bg_color[0] : (k == 1 ? d.bg_color[1] : d.bg_color[2]);
}

struct Bytes16 {
  uint8_t v[16];
};

// The winner's colour: the header's normal and colour rule at one pixel.
// `cross`: f is a crossing face, whose weights are beta_k = E_k / S and already sum to one.
__device__ inline void shade(const Params& p, int b, int f, bool cross, float px, float py, uint8_t out[3]) {
  const ehm_render_desc& d = p.d;
  const f32x4* r = p.rec + ((int64_t)b * d.F + f) * 4;
  const f32x4 q0 = r[0], q1 = r[1], q2 = r[2], q3 = r[3];
  float w0, w1, w2;
  if (cross) {
    const float rx = px - d.cx[b], ry = py - d.cy[b];
    const float E0 = (q0[0] * rx + q0[1] * ry) + q0[2], E1 = (q0[3] * rx + q1[0] * ry) + q1[1], E2 = (q1[2] * rx + q1[3] * ry) + q2[0];
    const float S = (E0 + E1) + E2;
    w0 = E0 / S;
    w1 = E1 / S;
    w2 = E2 / S;
  } else {
    float e[3];
    edges_at(q0, q1, q2, q3, px, py, e);
    const float sum = (e[0] + e[1]) + e[2];
    w0 = e[1] / sum * q1[2];      // b_k / z_k
    w1 = e[2] / sum * q1[3];
    w2 = e[0] / sum * q2[0];
  }
  const int i0 = d.faces[(int64_t)f * 3], i1 = d.faces[(int64_t)f * 3 + 1], i2 = d.faces[(int64_t)f * 3 + 2];
  float n[3];
  if (d.smooth) {
    const float* n0 = p.vnorm + ((int64_t)b * d.V + i0) * 3;
    const float* n1 = p.vnorm + ((int64_t)b * d.V + i1) * 3;
    const float* n2 = p.vnorm + ((int64_t)b * d.V + i2) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = (w0 * n0[k] + w1 * n1[k]) + w2 * n2[k];
  } else {
    cross_of(d.vertices + (int64_t)b * d.V * 3, i0, i1, i2, n);
  }
  const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  float ndl = 0.0f;
  if (len > 0.0f && isfinite(len)) ndl = ((n[0] * d.light_dir[0] + n[1] * d.light_dir[1]) + n[2] * d.light_dir[2]) / len;
  ndl = d.two_sided ? fabsf(ndl) : fmaxf(ndl, 0.0f);
  const float light = d.ambient + d.diffuse * ndl;
  const float wsum = (w0 + w1) + w2;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float base = d.base_color[k];
    if (d.vertex_colors) {
      base = (w0 * d.vertex_colors[(int64_t)i0 * 3 + k] + w1 * d.vertex_colors[(int64_t)i1 * 3 + k]) + w2 * d.vertex_colors[(int64_t)i2 * 3 + k];
      if (!cross) base = base / wsum;
    }
    float c = base * light;
    c = fminf(fmaxf(c, 0.0f), 1.0f);             // (a NaN becomes 0)
    out[k] = (uint8_t)floorf(255.0f * c + 0.5f);
  }
}

// What a lane of tile_kernel needs to evaluate a record: its column's sample, its row inside a block of four, the tile's and the region's origin.
struct Lane {
  float px, rxc, cyb, ry0, z_near;
  int y0, ly;
};

// One record of a face wholly in front against the lane's four pixels: the header's edge functions and depth.
__device__ __forceinline__ void front_face(const f32x4 q0, const f32x4 q1, const f32x4 q2, const f32x4 q3, int f, const Lane& L, float (&bz)[kRows],
                                           int (&bi)[kRows]) {
  const float area = q2[1];
  const float vmin = fminf(fminf(q0[1], q0[3]), q1[1]), vmax = fmaxf(fmaxf(q0[1], q0[3]), q1[1]);
  const float t0 = q2[3] * (L.px - q0[0]), t1 = q3[1] * (L.px - q0[2]), t2 = q3[3] * (L.px - q1[0]);
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const float by0 = L.ry0 + (float)(4 * k);
    if (vmax < by0 || vmin > by0 + 4.0f) continue;
    const float py = (float)(L.y0 + L.ly + 4 * k) + 0.5f;
    const float e0 = q2[2] * (py - q0[1]) - t0, e1 = q3[0] * (py - q0[3]) - t1, e2 = q3[2] * (py - q1[1]) - t2;
    const bool in = area > 0.0f ? (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) : (e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f);
    if (!in) continue;
    const float sum = (e0 + e1) + e2;
    if (sum == 0.0f) continue;
    const float z = sum / ((e1 * q1[2] + e2 * q1[3]) + e0 * q2[0]);      // 1 / (b0/z0 + b1/z1 + b2/z2) with b = e / sum, in one division
    if (z < bz[k] || (z == bz[k] && f < bi[k])) {
      bz[k] = z;
      bi[k] = f;
    }
  }
}

// One record of a crossing face: E_k = (c_kx rx + c_ky ry) + c_kz, covered where each has the sign of D, z = D / S beyond the near plane.
__device__ __forceinline__ void crossing_face(const f32x4 q0, const f32x4 q1, const f32x4 q2, const f32x4 q3, int f, const Lane& L, float (&bz)[kRows],
                                              int (&bi)[kRows]) {
  const float D = q2[1];
  const float t0 = q0[0] * L.rxc, t1 = q0[3] * L.rxc, t2 = q1[2] * L.rxc;
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const float by0 = L.ry0 + (float)(4 * k);
    if (q3[1] < by0 || q3[0] > by0 + 4.0f) continue;
    const float ry = ((float)(L.y0 + L.ly + 4 * k) + 0.5f) - L.cyb;
    const float e0 = (t0 + q0[1] * ry) + q0[2], e1 = (t1 + q1[0] * ry) + q1[1], e2 = (t2 + q1[3] * ry) + q2[0];
    const bool in = D > 0.0f ? (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) : (e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f);
    if (!in) continue;
    const float sum = (e0 + e1) + e2;
    if (sum == 0.0f) continue;
    const float z = D / sum;
    if (!(z > L.z_near)) continue;
    if (z < bz[k] || (z == bz[k] && f < bi[k])) {
      bz[k] = z;
      bi[k] = f;
    }
  }
}

// The survivors of one group of 64 records (mask, wave-uniform) one after the other with all lanes, the next survivor's record read from LDS while
// the current one is evaluated.  For a chunk without a crossing face: every chunk of a mesh in front of the plane.
__device__ __forceinline__ void walk(const f32x4 (*recs)[4], const int* ids, int h, unsigned long long mask, const Lane& L, float (&bz)[kRows],
                                     int (&bi)[kRows]) {
  int i = h + __builtin_ctzll(mask);
  mask &= mask - 1;
  f32x4 q0 = recs[i][0], q1 = recs[i][1], q2 = recs[i][2], q3 = recs[i][3];
  int f = ids[i];
  while (true) {
    const bool more = mask != 0;
    if (more) {
      i = h + __builtin_ctzll(mask);
      mask &= mask - 1;
    }
    const f32x4 n0 = recs[i][0], n1 = recs[i][1], n2 = recs[i][2], n3 = recs[i][3];
    const int nf = ids[i];
    if (q2[1] != 0.0f) front_face(q0, q1, q2, q3, f, L, bz, bi);
    if (!more) break;
    q0 = n0;
    q1 = n1;
    q2 = n2;
    q3 = n3;
    f = nf;
  }
}

// The same for a chunk that holds a crossing face: the kind is bit 0 of the id, wave-uniform as the face is.  Such chunks are few (the faces that
// straddle the plane and the tiles their boxes touch), so this loop does without the read-ahead: its registers then stay under the other loop's.
__device__ __forceinline__ void walk_mixed(const f32x4 (*recs)[4], const int* ids, int h, unsigned long long mask, const Lane& L, float (&bz)[kRows],
                                           int (&bi)[kRows]) {
  while (mask != 0) {
    const int i = h + __builtin_ctzll(mask);
    mask &= mask - 1;
    const f32x4 q0 = recs[i][0], q1 = recs[i][1], q2 = recs[i][2], q3 = recs[i][3];
    const int f = ids[i];
    if (q2[1] == 0.0f) continue;
    if (__builtin_amdgcn_readfirstlane(f & 1))
      crossing_face(q0, q1, q2, q3, f, L, bz, bi);
    else
      front_face(q0, q1, q2, q3, f, L, bz, bi);
  }
}

// WORK: block j of item b renders the j-th tile of the item's work list (the tiles with a face; a block beyond the list leaves at once, so the
// blocks that rasterise are dispatched together and fill the chip).  !WORK: block `tile` of item b writes the background of a tile without a face
// (all tiles of an item whose lists overflowed) and leaves a tile with one to the other launch.  Between them every pixel is written once.
// CLIP: the list may hold crossing faces.  Without it the kernel is the one-kind kernel (81 VGPRs, 5 waves per SIMD).  With it a chunk that holds
// a crossing face takes walk_mixed and every other chunk the same read-ahead loop: 95 VGPRs, still 5 waves, no scratch (a second body inside the
// read-ahead loop took 102 VGPRs and 4 waves, and cost a mesh without a crossing face 12 %: docs/EXPERIMENTS.md R30.3).
template <bool WORK, bool CLIP>
__global__ __launch_bounds__(kThreads) void tile_kernel(const Params p) {
  __shared__ f32x4 recs[kChunk][4];
  __shared__ int ids[kChunk];
  __shared__ f32x4 box[kChunk];                      // (umin, umax, vmin, vmax) of the record
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTH * kRowBytes];
  const ehm_render_desc& d = p.d;
  const int b = blockIdx.y, t = threadIdx.x;
  const int64_t nt = (int64_t)p.ntx * p.nty;
  const bool over = d.needed_capacity[b] > d.bin_capacity;
  if (WORK && (over || (int)blockIdx.x >= p.nwork[b])) return;
  int id = WORK ? p.work[b * nt + blockIdx.x] : (int)blockIdx.x;
  if (WORK && (unsigned)id >= (unsigned)nt) return;          // (never: the list holds tile indices)
  const int n = over ? 0 : p.count[b * nt + id];
  if (WORK != (n > 0)) return;
  const int tyi = id / p.ntx, txi = id - tyi * p.ntx;
  const int x0 = txi * kTW, y0 = tyi * kTH;
  const int cols = d.W - x0 < kTW ? d.W - x0 : kTW, rows = d.H - y0 < kTH ? d.H - y0 : kTH;
  const int rowbytes = cols * 3;
  const int* list = p.list + (int64_t)b * d.bin_capacity + (n > 0 ? p.offset[b * nt + id] : 0);

  // ---- the background tile: straight to the output when the tile has no face, into LDS otherwise
  const uint8_t* frame = nullptr;
  if (d.frames) {
    const int fi = d.frame_index[b];
    if (fi >= 0 && fi < d.Fr) frame = d.frames + (int64_t)fi * d.H * d.W * 3;
  }
  uint8_t* color = d.color ? d.color + (int64_t)b * d.H * d.W * 3 : nullptr;
  if (color) {
    if (p.aligned16) {
      const int r = t / (kRowBytes / 16), c = t - r * (kRowBytes / 16);
      if (r < rows && c * 16 < rowbytes) {                  // rowbytes % 16 == 0 here: a 16-byte piece is inside the row or outside it
        const int64_t g = ((int64_t)(y0 + r) * d.W + x0) * 3 + c * 16;
        Bytes16 v;
        if (frame) {
          *(uint4*)&v = *(const uint4*)(frame + g);
        } else {
#pragma unroll
          for (int k = 0; k < 16; ++k) v.v[k] = bg_at(d, c * 16 + k);
        }
        if (n > 0)
          *(uint4*)(tile + r * kRowBytes + c * 16) = *(uint4*)&v;
        else
          *(uint4*)(color + g) = *(uint4*)&v;
      }
    } else {
      for (int i = t; i < rows * rowbytes; i += kThreads) {
        const int r = i / rowbytes, o = i - r * rowbytes;
        const int64_t g = ((int64_t)(y0 + r) * d.W + x0) * 3 + o;
        const uint8_t v = frame ? frame[g] : bg_at(d, o);
        if (n > 0)
          tile[r * kRowBytes + o] = v;
        else
          color[g] = v;
      }
    }
  }

  // ---- the list, in chunks through LDS.  Wave w owns the 16 columns 16 w .. 16 w + 15 of the tile, a lane column lx of them and the rows
  // ly + 4 k: for one k the wave covers a 16 x 4 block, so a face is skipped per wave (its box against the 16 x 16 region) and per k (against the
  // block) before any lane evaluates an edge function - the boxes are wave-uniform, the branches too.
  const int wv = t >> 6, lx = wv * 16 + (t & 15), ly = (t >> 4) & 3;
  const float px = (float)(x0 + lx) + 0.5f;
  const float rx0 = (float)(x0 + wv * 16), rx1 = rx0 + 16.0f, ry0 = (float)y0;      // the region's samples lie inside (rx0, rx1) x (ry0, ry0 + 16)
  // (a crossing face's rule is relative to the principal point)
  const Lane lane = {px, CLIP ? px - d.cx[b] : 0.0f, CLIP ? d.cy[b] : 0.0f, ry0, d.z_near, y0, ly};
  float bz[kRows];
  int bi[kRows];                                       // 2 * face index + kind, as ids[] holds it
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    bz[k] = __builtin_inff();
    bi[k] = -1;
  }
  for (int c0 = 0; c0 < n; c0 += kChunk) {
    const int m = n - c0 < kChunk ? n - c0 : kChunk;
    __syncthreads();
    bool crossing = false;
    if (t < m) {
      int f = list[c0 + t];
      const bool valid = (unsigned)f < (unsigned)d.F;     // (always: the lists hold what fill_kernel wrote; an index outside would read outside)
      f = valid ? f : 0;
      const f32x4* r = p.rec + ((int64_t)b * d.F + f) * 4;
      const f32x4 q0 = r[0], q1 = r[1];
      f32x4 q2 = r[2];
      if (!valid) q2[1] = 0.0f;
      recs[t][0] = q0;
      recs[t][1] = q1;
      recs[t][2] = q2;
      const f32x4 q3 = r[3];
      recs[t][3] = q3;
      crossing = CLIP && is_crossing(q3);
      ids[t] = 2 * f + (crossing ? 1 : 0);               // the kind rides in bit 0: the order of the face indices is kept (F <= 2^24)
      box[t] = box_of(q0, q1, q2, CLIP ? q3 : f32x4{0.0f, 0.0f, 0.0f, 0.0f});
    }
    // a chunk without a crossing face (every chunk of a mesh in front of the plane) takes the loop that has no second body
    bool mixed = false;
    if (CLIP)
      mixed = __syncthreads_or(crossing) != 0;
    else
      __syncthreads();
    // 64 faces at a time, one per lane, against the wave's region; the survivors (a wave-uniform mask) one after the other with all lanes, the
    // next survivor's record read from LDS while the current one is evaluated
    for (int h = 0; h < m; h += 64) {
      const int mine = h + (t & 63);
      bool hit = false;
      if (mine < m) {
        const f32x4 bx = box[mine];
        hit = !(bx[1] < rx0 || bx[0] > rx1 || bx[3] < ry0 || bx[2] > ry0 + 16.0f);
      }
      unsigned long long mask = __ballot(hit);
      if (mask == 0) continue;
      if (CLIP && mixed)
        walk_mixed(recs, ids, h, mask, lane, bz, bi);
      else
        walk(recs, ids, h, mask, lane, bz, bi);
    }
  }

  // ---- the winners: depth, index, colour
  const int x = x0 + lx;
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int y = y0 + ly + 4 * k;
    if (x >= d.W || y >= d.H) continue;
    const int64_t g = ((int64_t)b * d.H + y) * d.W + x;
    if (d.depth) d.depth[g] = bi[k] >= 0 ? bz[k] : 0.0f;
    if (d.face_index) d.face_index[g] = bi[k] >> 1;      // (-1 stays -1)
    if (color && bi[k] >= 0) {
      uint8_t c[3];
      shade(p, b, bi[k] >> 1, CLIP && (bi[k] & 1), px, (float)y + 0.5f, c);
      uint8_t* o = tile + (ly + 4 * k) * kRowBytes + lx * 3;
      o[0] = c[0];
      o[1] = c[1];
      o[2] = c[2];
    }
  }
  if (!color || n == 0) return;
  __syncthreads();
  if (p.aligned16) {
    const int r = t / (kRowBytes / 16), c = t - r * (kRowBytes / 16);
    if (r < rows && c * 16 < rowbytes) *(uint4*)(color + ((int64_t)(y0 + r) * d.W + x0) * 3 + c * 16) = *(const uint4*)(tile + r * kRowBytes + c * 16);
  } else {
    for (int i = t; i < rows * rowbytes; i += kThreads) {
      const int r = i / rowbytes, o = i - r * rowbytes;
      color[((int64_t)(y0 + r) * d.W + x0) * 3 + o] = tile[r * kRowBytes + o];
    }
  }
}

int check_desc(const ehm_render_desc* d) {
  EHM_CHECK_ARG(d && d->vertices && d->faces && d->fx && d->fy && d->cx && d->cy);
  EHM_CHECK_ARG(d->H > 0 && d->W > 0 && d->H <= 32768 && d->W <= 32768);
  EHM_CHECK_ARG(d->B > 0 && d->B <= 65535 && d->V > 0 && d->V <= (1 << 24) && d->F > 0 && d->F <= (1 << 24));
  EHM_CHECK_ARG(!d->frames || (d->frame_index && d->Fr > 0));
  EHM_CHECK_ARG(d->color || d->depth || d->face_index);
  EHM_CHECK_ARG(!d->smooth || (d->vf_offsets && d->vf_faces));
  EHM_CHECK_ARG(d->bin_capacity >= 1 && d->bin_capacity <= (1 << 30));
  EHM_CHECK_ARG(d->clip_near == 0 || d->clip_near == 1);
  return 0;
}

}  // namespace

extern "C" int ehm_render_workspace_bytes(const ehm_render_desc* d, int64_t* bytes) {
  EHM_CHECK_ARG(bytes);
  if (int rc = check_desc(d)) return rc;
  *bytes = layout_of(*d).total;
  return 0;
}

extern "C" int ehm_render(const ehm_render_desc* d, void* stream) {
  if (int rc = check_desc(d)) return rc;
  const Layout L = layout_of(*d);
  EHM_CHECK_ARG(d->needed_capacity && d->workspace && ((uintptr_t)d->workspace & 15) == 0 && d->workspace_bytes >= L.total);
  EHM_CHECK_ARG(L.nt <= 0x7fffffff);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)d->workspace;
  Params p;
  p.d = *d;
  p.proj = (float4*)(ws + L.proj);
  p.vnorm = (float*)(ws + L.vnorm);
  p.rec = (f32x4*)(ws + L.rec);
  p.count = (int*)(ws + L.count);
  p.cursor = (int*)(ws + L.cursor);
  p.offset = (int*)(ws + L.offset);
  p.work = (int*)(ws + L.work);
  p.nwork = (int*)(ws + L.nwork);
  p.list = (int*)(ws + L.list);
  p.ntx = L.ntx;
  p.nty = L.nty;
  p.aligned16 = d->W % 16 == 0 && ((uintptr_t)d->color & 15) == 0 && ((uintptr_t)d->frames & 15) == 0;
  EHM_HIP(hipMemsetAsync(ws + L.count, 0, (size_t)(L.offset - L.count), s));
  const dim3 block(kThreads);
  hipLaunchKernelGGL(vertex_kernel, dim3((unsigned)ceil_div(d->V, kThreads), (unsigned)d->B), block, 0, s, p);
  EHM_LAUNCH_CHECK();
  hipLaunchKernelGGL(face_kernel, dim3((unsigned)ceil_div(d->F, kThreads), (unsigned)d->B), block, 0, s, p);
  EHM_LAUNCH_CHECK();
  hipLaunchKernelGGL(scan_kernel, dim3((unsigned)d->B), block, 0, s, p);
  EHM_LAUNCH_CHECK();
  hipLaunchKernelGGL(fill_kernel, dim3((unsigned)ceil_div(d->F, kThreads), (unsigned)d->B), block, 0, s, p);
  EHM_LAUNCH_CHECK();
  if (d->clip_near)
    hipLaunchKernelGGL((tile_kernel<true, true>), dim3((unsigned)L.nt, (unsigned)d->B), block, 0, s, p);
  else
    hipLaunchKernelGGL((tile_kernel<true, false>), dim3((unsigned)L.nt, (unsigned)d->B), block, 0, s, p);
  EHM_LAUNCH_CHECK();
  hipLaunchKernelGGL((tile_kernel<false, false>), dim3((unsigned)L.nt, (unsigned)d->B), block, 0, s, p);
  EHM_LAUNCH_CHECK();
  return 0;
}
