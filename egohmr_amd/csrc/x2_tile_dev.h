// The split-f16 ("X2": hi + lo f16 pairs, gcn_dev.h) tile engine's shared device pieces: what the K loops of gcn_tile.hip (hidden graph convs),
// linear.hip (scene PointNet) and conv.hip (ResNet-50 trunk) have in common.  The .hip files keep what is theirs: operand addressing (dma_a / dma_b),
// tile scheduling and epilogues.
// Everything here is inlined, and moving a piece here left every kernel's generated code as it was (tools/isa_diff.py compares two revisions kernel
// by kernel; docs/EXPERIMENTS.md R7.1).  That is why some pieces are macros: the kernels sit at the edge of their register budget (they keep SGPRs in
// VGPR lanes), and index arithmetic or LDS loads that arrive through a function - inlined or not - reach the optimiser in another order and come out
// with another register allocation.  MFMA sequences and schedule pins do not have that problem and are functions.
//
// LDS image of an operand stage: rows of X2_RK floats = 128 bytes = one K tile (X2: 32 hi halves | 32 lo halves; plain f16: 64 k), filled by
// 16-byte buffer_load ... lds DMA.  The physical 16-byte chunk c of row r holds the logical chunk c ^ ((r >> 1) & 7): the XOR is applied to the SOURCE
// address by the DMA lane (x2_dma_lane), so every ds_read_b128 fragment read is bank-conflict free.
#pragma once
#include <type_traits>

#include "common.h"
#include "gcn_dev.h"

#define AS1 __attribute__((address_space(1)))
#define AS3 __attribute__((address_space(3)))

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4a __attribute__((ext_vector_type(4)));   // accumulator of the 16 x 16 x 32 MFMA
typedef std::integral_constant<int, 0> I0;                   // compile-time operand half / K tile parity, passed as a value
typedef std::integral_constant<int, 1> I1;

constexpr int X2_RK = 32;                                    // floats per operand row and K tile = 128 bytes
// __builtin_amdgcn_sched_group_barrier masks
constexpr int SG_MFMA = 0x008, SG_DS_READ = 0x100, SG_VMEM = 0x010;

// MODE.FP16_OVFL = 1 for the life of the wave (hwreg MODE = 1, bit 23): every f32 -> f16 conversion of the epilogue clamps to +-65504 instead of
// producing inf - the same results on finite values as the explicit clamps it replaces (4 of the ~8 vector-ALU instructions per output value: v_med3
// + its canonicalising v_max, twice; in the GCN tile engine 144 v_med3_f32 + their canonicalising v_max_f32 per wave and tile, in an epilogue
// during which the block's matrix pipes idle).
static __device__ __forceinline__ void x2_fp16_ovfl_on() { __builtin_amdgcn_s_setreg(1 | (23 << 6), 1); }
// ... and back to 0.  A kernel whose activations may hold a NaN or an infinity keeps the bit CLEAR while its matrix cores run and sets it around the
// epilogue's conversions alone: with the bit set an MFMA does not propagate a non-finite f16 operand (measured on an MI355X: a NaN half left finite,
// wrong sums - docs/EXPERIMENTS.md, round 32), while the conversions keep a NaN and an infinity of their f32 input as they are.
static __device__ __forceinline__ void x2_fp16_ovfl_off() { __builtin_amdgcn_s_setreg(1 | (23 << 6), 0); }

// The hi / lo split of a value (MODE.FP16_OVFL: the conversions saturate at +-65504, never inf); hi and lo may be elements of a half8, hence a macro.
#define X2_SPLIT(v, hi, lo) ((hi) = (half_t)(v), (lo) = (half_t)((v) - (float)(hi)))
// ... of 8 values v[] in front of two b128 stores (LO = false, the hi-only tiers: lo is left alone)
#define X2_SPLIT8(LO, v, hi, lo)                                   \
  _Pragma("unroll") for (int c_ = 0; c_ < 8; ++c_) {               \
    if constexpr (LO) X2_SPLIT((v)[c_], (hi)[c_], (lo)[c_]);       \
    else (hi)[c_] = (half_t)(v)[c_];                               \
  }

// ---- lane identity.  The kernels RE-DERIVE it at the head of every tile from an opaque copy of the thread id, so that none of it has to stay in a
// register across the epilogue (with it live the chained GCN kernel spilled ~120 VGPRs); the opaque copy keeps hipcc from hoisting it out of the tile loop.
static __device__ __forceinline__ void x2_lane_wave(int tid, int& lane, int& wave) {
  int t = tid;
  asm volatile("" : "+v"(t));
  lane = t & 63;
  wave = __builtin_amdgcn_readfirstlane(t >> 6);
}
// DMA: one wave instruction = 8 rows x 128 B.  My row of instruction i is r0 + 8 * (waves) * i (a multiple of 32 further: the swizzle key stays), my
// 16-byte chunk sits at float offset swz of the SOURCE row; swz < 16 <=> the chunk holds hi halves (logical chunks 0-3 of an X2 K tile).
static __device__ __forceinline__ void x2_dma_lane(int lane, int wave, int& r0, int& swz) {
  r0 = 8 * wave + (lane >> 3);
  swz = ((lane & 7) ^ ((r0 >> 1) & 7)) << 2;
}
static __device__ __forceinline__ bool x2_hi_lane(int swz) { return swz < 16; }

// ---- fragment offsets (floats from the start of a stage; the B region starts at baseB), derived per wave from the lane's rows
// 32 x 32 x 16: lane (mi = l & 31, g = l >> 5) holds row mi, k = 8 g .. + 7 of a 16-wide k-step s = one 16-byte chunk: logical chunk 4 hl + 2 s + g of an
// X2 tile [hi k0-31 | lo k0-31] (NHL = 2: hl = 0 hi, 1 lo), 2 s + g of an f16 tile (k0-63, NHL = 1).  rA / rB = the lane's row of A / B block 0; blocks
// 32 rows further leave the swizzle key alone.  int oA[KS][NHL][NO], oB[KS][NHL]; NO = 2 (the GCN's permuted rows, blocks 8 rows apart): oA[..][1] is
// the offset for the odd blocks, whose key has bit 2 flipped.
#define X2_FRAG_OFFSETS32(oA, oB, KS, NHL, NO, baseB, rA, rB, g)                                                \
  {                                                                                                              \
    const int rA_ = (rA), rB_ = (rB);                                                                            \
    const int keyA_ = (rA_ >> 1) & 7, keyB_ = (rB_ >> 1) & 7;                                                    \
    _Pragma("unroll") for (int s_ = 0; s_ < (KS); ++s_)                                                          \
      _Pragma("unroll") for (int hl_ = 0; hl_ < (NHL); ++hl_) {                                                  \
        const int c_ = ((NHL) == 2 ? 4 * hl_ : 0) + 2 * s_ + (g);                                                \
        _Pragma("unroll") for (int o_ = 0; o_ < (NO); ++o_) (oA)[s_][hl_][o_] = rA_ * X2_RK + (((c_ ^ keyA_) ^ (4 * o_)) << 2); \
        (oB)[s_][hl_] = (baseB) + rB_ * X2_RK + ((c_ ^ keyB_) << 2);                                             \
      }                                                                                                          \
  }
// 16 x 16 x 32 (a K tile = ONE k-step): lane (i = l & 15, kg = l >> 4) holds row i of a 16-row tile and the logical chunk kg (hi halves, [0]) / 4 + kg
// (lo halves, [1]) of the tile's 128-byte rows.  rowA0 / rowB0 = the wave's first A / B row (multiples of 16: row tiles 16 t further leave the key alone).
// int oA16[2], oB16[2].
#define X2_FRAG_OFFSETS16(oA16, oB16, baseB, rowA0, rowB0, lane)                                \
  {                                                                                             \
    const int i16_ = (lane) & 15, kg_ = (lane) >> 4, key_ = (i16_ >> 1) & 7;                    \
    _Pragma("unroll") for (int hl_ = 0; hl_ < 2; ++hl_) {                                       \
      (oA16)[hl_] = ((rowA0) + i16_) * X2_RK + (((4 * hl_ + kg_) ^ key_) << 2);                 \
      (oB16)[hl_] = (baseB) + ((rowB0) + i16_) * X2_RK + (((4 * hl_ + kg_) ^ key_) << 2);       \
    }                                                                                           \
  }

// ---- 16 x 16 x 32 micro-kernel.  Operand halves A[rh] (row tiles 3 rh .. + 2 of 16 rows) and B[ch] (NU column tiles of 16), 6 x 2 NU accumulators.
// N fragment pairs (hi into h[t], lo into l[t]) of the stage S, pair t from row `row` (an expression of the loop variable t): one ds_read_b128 each; an
// optional statement per pair behind its loads
#define X2_LD16(t, N, h, l, S, o_hi, o_lo, row, ...)              \
  _Pragma("unroll") for (int t = 0; t < (N); ++t) {               \
    (h)[t] = *(const half8*)((S) + (o_hi) + (row) * X2_RK);       \
    (l)[t] = *(const half8*)((S) + (o_lo) + (row) * X2_RK);       \
    __VA_ARGS__;                                                  \
  }
// ... the hi fragments alone (the two-term product reads no activation lo half)
#define X2_LD16_HI(t, N, h, S, o_hi, row)                         \
  _Pragma("unroll") for (int t = 0; t < (N); ++t) (h)[t] = *(const half8*)((S) + (o_hi) + (row) * X2_RK);
// one phase (row half RH, column half CH) = 3 TERMS NU MFMAs: small cross terms first, leading term last, 3 NU independent accumulators per term.
// TERMS = 3: al*bh + ah*bl + ah*bh.  TERMS = 2: ah*bl + ah*bh = a_hi * (b_hi + b_lo) - the A operand taken as its hi half, B in full (Al is not read).
template <int RH, int CH, int NU, int TERMS = 3>
static __device__ __forceinline__ void x2_mm16(f32x4a (&c16)[6][2 * NU], const half8 (&Ah)[2][3], const half8 (&Al)[2][3], const half8 (&Bh)[2][NU],
                                                const half8 (&Bl)[2][NU]) {
  static_assert(TERMS == 2 || TERMS == 3, "two or three terms per product");
  if constexpr (TERMS == 3) {
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int u = 0; u < NU; ++u) c16[3 * RH + t][NU * CH + u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al[RH][t], Bh[CH][u], c16[3 * RH + t][NU * CH + u], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int u = 0; u < NU; ++u) c16[3 * RH + t][NU * CH + u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[RH][t], Bl[CH][u], c16[3 * RH + t][NU * CH + u], 0, 0, 0);
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int u = 0; u < NU; ++u) c16[3 * RH + t][NU * CH + u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[RH][t], Bh[CH][u], c16[3 * RH + t][NU * CH + u], 0, 0, 0);
}
// The schedule of a phase of NMFMA MFMAs: LDS reads behind every second MFMA, DMA instructions in the gaps between them (GCN chain kernel, same box:
// 918 -> 903 us per launch against "reads one per MFMA from the start, DMAs behind them"; no pinning at all measured like the latter)
template <int NMFMA>
static __device__ __forceinline__ void x2_pin16(int reads, int dmas) {
#pragma unroll
  for (int i = 0; i < NMFMA; ++i) {
    __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
    if ((i & 1) == 0 && (i >> 1) < reads) __builtin_amdgcn_sched_group_barrier(SG_DS_READ, 1, 0);
    else if ((i & 1) == 1 && (i >> 1) < dmas) __builtin_amdgcn_sched_group_barrier(SG_VMEM, 1, 0);
  }
}

// ---- 32 x 32 x 16 micro-kernel (plain f16 and the hi-only tiers; a K tile = 2 (X2) or 4 (f16) k-steps on register double-buffered fragment sets).
// One k-step's fragments: three 32-row A blocks, NB 32-column B blocks; the lo halves only in SPLIT mode.
template <int NB, bool SPLIT>
struct X2Frags {
  half8 ah[3], al[SPLIT ? 3 : 1], bh[NB], bl[SPLIT ? NB : 1];
};
// acc[t][u] += A block t . B block u, the three terms of one accumulator back to back: small cross terms first, leading term last.  (The GCN keeps its
// own: its two branches' accumulators alternate term by term, and as one [3][2] array its plain-f16 kernels came out differently.)
template <int NB, bool SPLIT>
static __device__ __forceinline__ void x2_mfmas(f32x16 (&acc)[3][NB], const X2Frags<NB, SPLIT>& f) {
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if constexpr (SPLIT) {
        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[t], f.bh[u], acc[t][u], 0, 0, 0);
        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[t], f.bl[u], acc[t][u], 0, 0, 0);
      }
      acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[t], f.bh[u], acc[t][u], 0, 0, 0);
    }
}
// MFMA, read, MFMA, read, ... (NR reads), then the remaining NM - NR MFMAs
template <int NR, int NM>
static __device__ __forceinline__ void x2_pin_reads() {
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
    __builtin_amdgcn_sched_group_barrier(SG_DS_READ, 1, 0);
  }
  __builtin_amdgcn_sched_group_barrier(SG_MFMA, NM - NR, 0);
}

// ---- XCD-aware tile order of a persistent grid of G blocks (linear, conv): block b sits on XCD b % 8; the n_tiles column tiles of one row tile go to
// neighbouring blocks of ONE XCD in the same iteration `it`, so the row tile's activations come from HBM once.  false: the grid is past its tiles.
static __device__ __forceinline__ bool x2_xcd_order(int G, int n_tiles) { return (G % 8 == 0) && ((G / 8) % n_tiles == 0); }
static __device__ __forceinline__ bool x2_xcd_tile_of(bool xcd_order, int it, int b, int G, int n_tiles, int m_tiles, int& m, int& n) {
  if (xcd_order) {
    const int x = b & 7, j = b >> 3, per = (G >> 3) / n_tiles;
    m = (it * per + j / n_tiles) * 8 + x;
    n = j % n_tiles;
  } else {
    const long long t = (long long)it * G + b;
    m = (int)(t / n_tiles);
    n = (int)(t % n_tiles);
  }
  return m < m_tiles;
}
