// Shared helpers for the gfx950 kernels behind include/egohmr_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define EHM_EINVAL (-22)
#define EHM_ENOMEM (-12)
#define EHM_EIO (-5)
#define EHM_ERANGE (-34)

extern "C" const char* ehm_last_error(void);
void ehm_set_error(const char* fmt, ...);

#define EHM_CHECK_ARG(cond)                                              \
  do {                                                                   \
    if (!(cond)) {                                                       \
      ehm_set_error("%s:%d bad argument: %s", __func__, __LINE__, #cond); \
      return EHM_EINVAL;                                                 \
    }                                                                    \
  } while (0)

#define EHM_HIP(call)                                                                        \
  do {                                                                                       \
    hipError_t e__ = (call);                                                                 \
    if (e__ != hipSuccess) {                                                                 \
      ehm_set_error("%s:%d %s -> %s", __func__, __LINE__, #call, hipGetErrorString(e__));     \
      return e__ == hipErrorOutOfMemory ? EHM_ENOMEM : EHM_EIO;                              \
    }                                                                                        \
  } while (0)

#define EHM_LAUNCH_CHECK() EHM_HIP(hipGetLastError())

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kJ = 24;        // SMPL joints = graph nodes
constexpr int kPoseDim = 144;  // 24 x 6

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t round_up(int64_t a, int64_t b) { return ceil_div(a, b) * b; }

// ---- data-parallel BatchNorm (csrc/gcn_train.hip, csrc/bn2d_train.hip): every rank's row count, handed to a merge kernel by value
constexpr int kMaxRanks = 64;
struct RankRows {
  double r[kMaxRanks];
  double total;
};
// rows [world] on the host -> RankRows: every rank has rows, all of them together at least two
static inline int rank_rows_of(const int64_t* rows, int world, RankRows* rr) {
  EHM_CHECK_ARG(rows && world >= 1 && world <= kMaxRanks);
  int64_t total = 0;
  for (int k = 0; k < world; ++k) {
    EHM_CHECK_ARG(rows[k] >= 1 && rows[k] < (1ll << 40));
    rr->r[k] = (double)rows[k];
    total += rows[k];
  }
  EHM_CHECK_ARG(total >= 2);
  rr->total = (double)total;
  return 0;
}
// one channel's n float64 partial sums p[k * stride], added in index order: the fixed order every BatchNorm reduction of the two files ends in
static __device__ __forceinline__ double ordered_sum(const double* __restrict__ p, size_t stride, int n) {
  double s = 0.0;
  for (int k = 0; k < n; ++k) s += p[k * stride];
  return s;
}
// Chan et al.'s merge of the ranks' (mean, M2 = sum of squares centred on the rank's own mean) of one channel, in rank order; g: that channel's mean of
// rank 0, rank k's at g[k * stride], its M2 at g[k * stride + m2].  The mean is taken relative to rank 0's and M2's correction on the merged mean, so
// ranks whose means lie many sigma apart cancel nothing, and ONE rank gives back its own (mean, M2) bit for bit (mu_0 + 0, M2_0 + R_0 0).
static __device__ __forceinline__ void merge_moments(const double* __restrict__ g, size_t stride, size_t m2, const RankRows& rr, int world, double* mu,
                                                     double* M2) {
  const double mu0 = g[0];
  double d = 0.0;
  for (int k = 1; k < world; ++k) d += rr.r[k] * (g[(size_t)k * stride] - mu0);
  const double m = mu0 + d / rr.total;
  double s = 0.0, c = 0.0;
  for (int k = 0; k < world; ++k) {
    const double dk = g[(size_t)k * stride] - m;
    s += g[(size_t)k * stride + m2];
    c += rr.r[k] * (dk * dk);
  }
  *mu = m;
  *M2 = s + c;
}
// Where a channel's (mean, M2) over rr.total rows come from, for the one kernel per file that writes a BatchNorm's statistics out.  gathered == NULL: a
// call's own two passes, mean [N] and `count` partial sums of centred squares part[k * N].  Else every rank's pair [world][2][N], merged.
struct BnMoments {
  const double *part, *mean;
  int count;
  const double* gathered;
  int world;
  RankRows rr;
};
static inline BnMoments own_moments(const double* part, const double* mean, int count, double R) {
  BnMoments m = {part, mean, count, nullptr, 0, {}};
  m.rr.total = R;
  return m;
}
static __device__ __forceinline__ void moments_of(const BnMoments& s, int n, int N, double* mu, double* M2) {
  if (s.gathered) {
    merge_moments(s.gathered + n, (size_t)2 * N, (size_t)N, s.rr, s.world, mu, M2);
  } else {
    *mu = s.mean[n];
    *M2 = ordered_sum(s.part + n, (size_t)N, s.count);
  }
}

// ---- float32 chains that must round like the reference's separate torch ops: one correctly rounded operation each, never contracted.
// HIP's __fmul_rn / __fadd_rn / __fsub_rn are the plain operators, which hipcc's default -ffp-contract=fast-honor-pragmas fuses across
// statements: __fadd_rn(__fmul_rn(a, b), c) compiles to ONE v_fma_f32.  A product formed here carries no contract flag, so no sum can absorb it.
static __device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
static __device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
static __device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

// ---- cross-lane helpers on the DPP path (hipcc lowers __shfl_xor to ds_bpermute_b32, an LDS-crossbar instruction) ----
template <int CTRL>
static __device__ __forceinline__ float dpp_move(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
static __device__ __forceinline__ unsigned int dpp_xor1_u32(unsigned int v) {          // value of lane ^ 1 (quad_perm [1,0,3,2])
  return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
}
static __device__ __forceinline__ float row16_sum(float v) {   // every lane ends with the sum over its 16-lane row
  v += dpp_move<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_move<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_move<0x141>(v);   // row_half_mirror
  v += dpp_move<0x140>(v);   // row_mirror
  return v;
}
static __device__ __forceinline__ float wave_sum(float v) {    // wave-uniform sum over the 64 lanes
  const int b = __builtin_bit_cast(int, row16_sum(v));   // readlane is an integer builtin: move the bits, not the value
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16)) +
         __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
}

// Buffer descriptor over [p, p + 2 GiB) for raw_buffer_load/store: SGPR descriptor + 32-bit lane offset + scalar offset, i.e. no
// VALU address arithmetic.  readfirstlane pins the (wave-uniform) base into SGPRs; without it hipcc wraps every access in a
// waterfall loop.
// (num_records = 2 GiB - 1: the default; ehm_buffer_rsrc_4g covers [p, p + 4 GiB) for the one caller whose lane offsets span a whole tensor)
static __device__ __forceinline__ __amdgpu_buffer_rsrc_t ehm_buffer_rsrc_4g(const void* p) {
  const unsigned long long a = (unsigned long long)p;
  const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)a);
  const unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, (int)0xffffffffu, 0x00020000);
}
static __device__ __forceinline__ __amdgpu_buffer_rsrc_t ehm_buffer_rsrc(const void* p) {
  const unsigned long long a = (unsigned long long)p;
  const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)a);
  const unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, 0x7fffffff, 0x00020000);
}
