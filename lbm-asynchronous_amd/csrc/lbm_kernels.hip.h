// lbm_kernels.hip.h -- CDNA4 (gfx950) device code of the D2Q9-BGK engine.
//
// One fused kernel replaces the reference's five sweeps per timestep
// (accelerate_flow, propagate, rebound, collision, av_velocity;
// /root/reference/SerialCode/d2q9-bgk.c:207-458):
//   pull-stream 9 populations from the neighbours (periodic in x; in y either periodic or fed by
//   halo rows stored around the slab), bounce back on blocked cells, BGK-relax fluid cells, sum
//   |u| of the relaxed cells into one partial per workgroup, and apply the NEXT step's
//   accelerate_flow to the lid row before storing (so no separate pass over that row is needed).
// step_vec4 / step_scalar advance one timestep per pass over memory, step2_stream two, stepk_stream / stepk_pk
// two to four (stepk_pk with the collision on pairs of cells: packed fp32 instructions), step_tile several from LDS.
//
// Layout: structure of arrays interleaved by row -- value (k, y, x) lives at
// base + y*row_pitch + k*plane_stride + x with plane_stride = pitch and row_pitch = 9*pitch, i.e.
// the 9 planes of one row lie next to each other (36*nx bytes), rows follow each other, and four
// halo rows sit below row 0 and above row rows-1.  Every access is a contiguous, 16-byte-aligned
// run along x of ONE speed (fully coalesced), and a workgroup's 9+9 streams fall into a ~1 MB
// window instead of 18 windows 256 MiB apart: measured 10-13 % faster than 9 whole-grid planes on
// MI355X (profiles/r01_tuning.md).
//
// Each value is read exactly once and written exactly once per step: the algorithmic traffic is
// 72 B per lattice update, and there is no reuse to stage in LDS or to feed MFMA.  The one-step
// kernel is bound by HBM bandwidth: each lane owns 4 consecutive cells and moves every plane with
// one 16-byte access; the +-1 column shifts of the six x-moving populations are assembled from
// the lane's own aligned vector plus one neighbour dword.
//
// Speed numbering (SerialCode/d2q9-bgk.c:9-15):   6 2 5
//                                                  3 0 1
//                                                  7 4 8
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <tuple>
#include <type_traits>

#include "lbm_exact_sum.h"
#include "lbm_stats_row.h"
#include "lbm_residual_row.h"
#include "lbm_profile_row.h"
#include "lbm_coarse_row.h"
#include "lbm_enstrophy_row.h"
#include "lbm_stress_row.h"
#include "lbm_psi_row.h"
#include "lbm_exact_round.h"
#include "lbm_residual_until.h"
#include "lbm_tracer_step.h"

namespace lbm {

constexpr int kBlock = 256;  // 4 waves of 64
constexpr int kQ = 9;
constexpr int kNoRow = -1000000;  // "no such row in this slab"
// what a context records while it runs, at most one at a time: the host's Recorder::kind and resident_band's REC
constexpr int kRecNone = 0, kRecFrames = 1, kRecProbes = 2, kRecMean = 3, kRecFields = 4;
// (the obstacle forces, lbm_set_forces / lbm_batch_set_forces, the lattice statistics, lbm_set_stats /
// lbm_batch_set_stats, the velocity residuals, lbm_set_residual / lbm_batch_set_residual, and the line profiles,
// lbm_set_profiles / lbm_batch_set_profiles, are recorder kinds of the host alone: force_gather, stats_gather,
// residual_gather, profile_rows, profile_columns and their batch twins run behind the step kernels; so does the
// vorticity's vorticity_gather, lbm_set_enstrophy / lbm_batch_set_enstrophy, and the stream function's scan, psi_band_totals,
// psi_band_bases, psi_scan and psi_extrema, lbm_set_psi / lbm_batch_set_psi, and the coarse frames' coarse_gather,
// lbm_set_coarse_frames / lbm_batch_set_coarse_frames)

// 1/3 rounded to fp32, and the two constant divisors of the equilibrium, folded in fp32
// exactly as the reference's "2.f * c_sq" and "2.f * c_sq * c_sq" (SerialCode/d2q9-bgk.c:308,367-370)
constexpr float kCsq = 1.f / 3.f;
constexpr float kTwoCsq = 2.f * kCsq;
constexpr float kTwoCsqSq = 2.f * kCsq * kCsq;
constexpr float kW0 = 4.f / 9.f;
constexpr float kW1 = 1.f / 9.f;
constexpr float kW2 = 1.f / 36.f;

// Where a lattice lies and how its rows are addressed: the leading fields of every kernel's arguments, filled in one
// place on the host (lattice_args).  Value (k, row, x) is at k * plane_stride + row * row_pitch + x, mask byte (row, x) at
// row * pitch + x.  A kernel that reads a stored lattice takes it as src; one that modifies a lattice in place
// (accelerate_row*, init_equilibrium, aos_to_soa) takes it as dst.  48 bytes without padding: the structs derived from
// it keep their own first field at offset 48 (asserted below each), so no kernel argument moves.
struct LatticeArgs {
  const float* src;           // plane 0, row 0 of the source lattice
  float* dst;                 // plane 0, row 0 of the destination lattice
  const unsigned char* mask;  // rows x pitch, 1 = blocked
  long plane_stride;          // floats between planes
  long row_pitch;             // floats between lattice rows of one plane
  int pitch;                  // bytes between rows of the uint8 mask
  int nx;                     // cells per row
};
static_assert(sizeof(LatticeArgs) == 48, "no padding: derived arguments start at 48");

// the nine populations of cell (row, x) of the source lattice
__device__ __forceinline__ void gather_cell(const LatticeArgs& a, int row, int x, float (&f)[kQ]) {
  const long c = (long)row * a.row_pitch + x;
#pragma unroll
  for (int k = 0; k < kQ; k++) f[k] = a.src[k * a.plane_stride + c];
}
__device__ __forceinline__ bool cell_blocked(const LatticeArgs& a, int row, int x) {
  return a.mask[(long)row * a.pitch + x] != 0;
}

struct StepArgs : LatticeArgs {
  int rows;                   // rows owned by this slab
  int row_first;              // first slab row this launch advances
  int row_stride;             // distance between the rows this launch advances (1 = contiguous)
  int n_rows;                 // number of rows this launch advances
  int accel_row;              // slab row that receives next step's acceleration, or kNoRow
  float omega;
  float a1, a2;               // density*accel/9, density*accel/36 (SerialCode/d2q9-bgk.c:219-220)
  float* partials;            // one fp32 partial sum of |u| per workgroup of this launch
  int reverse;                // 1: workgroup b handles tile (n_tiles-1-b): rows are swept top-down
  int wrap;                   // 1: the slab is the whole grid, rows wrap periodically;
                              // 0: rows -1 and `rows` are halo rows stored around the slab
};

// ---------------------------------------------------------------------------------------------
// per-cell arithmetic
// ---------------------------------------------------------------------------------------------

// EXACT: the reference's expression trees, IEEE division and sqrt, no contraction
// (the library is compiled with -ffp-contract=off).  SerialCode/d2q9-bgk.c:325-401, 426-450.
__device__ __forceinline__ void moments_exact(const float (&f)[kQ], float& rho, float& ux, float& uy) {
  float d = f[0];
#pragma unroll
  for (int k = 1; k < kQ; k++) d += f[k];
  rho = d;
  ux = (f[1] + f[5] + f[8] - (f[3] + f[6] + f[7])) / d;
  uy = (f[2] + f[5] + f[6] - (f[4] + f[7] + f[8])) / d;
}

// ---- exact division by the three constant divisors ------------------------------------------
// x / C with C constant is the bulk of the reference's 27 divides per cell.  With R = RN(1/C):
//     q = x*R;  r = fma(-C, q, x);  q' = fma(r, R, q)
// q' equals the correctly rounded x / C -- verified EXHAUSTIVELY on the CPU for every fp32 x with
// 1e-30 < |x| < 1e30 and each of the three constants (tools/verify_const_div.c; the only
// mismatches lie where the residual r underflows or x*R overflows); x = 0 gives 0.
// Below 1e-30 the fast quotient may be a few ulps off, but it cannot change the result: every
// quotient is only ever ADDED to a value that is exactly 1 at that point --
//   eq_k = w*rho * (((1 + u_k/c^2) + u_k^2/(2c^4)) - |u|^2/(2c^2)):
//   |u_k^2| < 1e-30 means |u_k| < 1e-15, so |u_k/c^2| < 2^-25 and 1 + u_k/c^2 == 1, then
//   1 + (anything below 2^-25) == 1;  |u|^2 < 1e-30 means every |u_k| < 2e-15, so the minuend is 1
//   and 1 - (anything below 2^-25) == 1
// -- and a wrong-by-ulps number below 5e-30 is absorbed exactly like the right one (also checked
// exhaustively: the fast quotient of every |x| <= 1e-30 is finite and below 2^-90).
// Only huge dividends need care: a cell whose |u|^2 is not below 5e28 (or is NaN) takes the IEEE
// divides.  So the result is bit-identical to the reference's "x / c_sq" for ALL inputs at
// 3 instructions per divide instead of ~11 plus a quarter-rate v_rcp_f32.
__device__ __forceinline__ float div_const_fast(float x, float C, float R) {
  const float q = x * R;
  const float r = __fmaf_rn(-C, q, x);
  return __fmaf_rn(r, R, q);
}

struct EqTerms {
  float q1;  // u / c_sq
  float q2;  // (u*u) / (2 c_sq^2)
};
template <bool GUARDED_FAST>
__device__ __forceinline__ EqTerms eq_terms(float u) {
  constexpr float kInvCsq = 1.0f / kCsq;            // RN(1/C), folded by the compiler in fp32
  constexpr float kInvTwoCsqSq = 1.0f / kTwoCsqSq;
  EqTerms e;
  const float sq = u * u;
  if constexpr (GUARDED_FAST) {
    e.q1 = div_const_fast(u, kCsq, kInvCsq);
    e.q2 = div_const_fast(sq, kTwoCsqSq, kInvTwoCsqSq);
  } else {
    e.q1 = u / kCsq;
    e.q2 = sq / kTwoCsqSq;
  }
  return e;
}

__device__ __forceinline__ float equilibrium_from_terms(float w_rho, float q1, float q2, float usq_term) {
  return w_rho * (1.f + q1 + q2 - usq_term);
}

template <bool GUARDED_FAST>
__device__ __forceinline__ void collide_exact_body(const float (&t)[kQ], float omega, float rho, float ux,
                                                   float uy, float (&r)[kQ]) {
  constexpr float kInvTwoCsq = 1.0f / kTwoCsq;
  const float u_sq = ux * ux + uy * uy;
  const float usq_term = GUARDED_FAST ? div_const_fast(u_sq, kTwoCsq, kInvTwoCsq) : u_sq / kTwoCsq;
  const float w1r = kW1 * rho, w2r = kW2 * rho;
  // u[3] = -u[1], u[4] = -u[2], u[7] = -u[5], u[8] = -u[6] (exact negations), so the quotients of
  // the four opposite directions are the negated / identical quotients of the first four
  const EqTerms ex = eq_terms<GUARDED_FAST>(ux);
  const EqTerms ey = eq_terms<GUARDED_FAST>(uy);
  const EqTerms es = eq_terms<GUARDED_FAST>(ux + uy);
  const EqTerms ed = eq_terms<GUARDED_FAST>(-ux + uy);
  float eq[kQ];
  eq[0] = kW0 * rho * (1.f - usq_term);
  eq[1] = equilibrium_from_terms(w1r, ex.q1, ex.q2, usq_term);
  eq[2] = equilibrium_from_terms(w1r, ey.q1, ey.q2, usq_term);
  eq[3] = equilibrium_from_terms(w1r, -ex.q1, ex.q2, usq_term);
  eq[4] = equilibrium_from_terms(w1r, -ey.q1, ey.q2, usq_term);
  eq[5] = equilibrium_from_terms(w2r, es.q1, es.q2, usq_term);
  eq[6] = equilibrium_from_terms(w2r, ed.q1, ed.q2, usq_term);
  eq[7] = equilibrium_from_terms(w2r, -es.q1, es.q2, usq_term);
  eq[8] = equilibrium_from_terms(w2r, -ed.q1, ed.q2, usq_term);
#pragma unroll
  for (int k = 0; k < kQ; k++) r[k] = t[k] + omega * (eq[k] - t[k]);
}

// want_speed (wave-uniform): also return |u| of the relaxed cell for the av_velocity sum; the warm-up rows
// of a two-step band relax cells whose |u| belongs to another band's sum
template <bool EXACT>
__device__ __forceinline__ void collide(const float (&t)[kQ], float omega, float (&r)[kQ], float& speed,
                                        bool want_speed = true);

// ---- the two divides by the density, sharing one reciprocal -----------------------------------
// hipcc expands the IEEE fp32 divide a / b (AMDGPU LowerFDIV32) into
//     r0 = v_rcp_f32(b);  e = fma(-b, r0, 1);  r = fma(e, r0, r0);            (refined reciprocal)
//     q = a*r;  e = fma(-b, q, a);  q = fma(e, r, q);  e = fma(-b, q, a);  q = fma(e, r, q)
// wrapped in v_div_scale / v_div_fmas / v_div_fixup, which only act when an operand or the
// quotient is near the ends of the exponent range (denominator denormal or above 2^126,
// |a| below 2^-103, |a/b| above 2^96 or denormal) or is 0 / inf / NaN.  u_x and u_y divide by the
// same density, so the first line is done once and the second per numerator: the very same
// instructions, hence the same bits, 28 instead of 48 issue slots per cell.  Outside the plain
// range: a density outside [2^-60, 2^60] sends the cell to the IEEE divides; a numerator of 0 gives 0
// either way; a non-zero numerator below 2^-103 gives a quotient below 2^-43 that may differ in
// its last bits -- before the collision such a u is absorbed like the tiny quotients above
// (|u/c^2| < 2^-25), after it it only enters the diagnostic sum of |u| at the 1e-13 level; a
// quotient above 2^96 trips the |u|^2 guard.
__device__ __forceinline__ bool density_in_plain_range(float rho) {
  return (__float_as_uint(rho) - 0x21800000u) < (0x5D800000u - 0x21800000u);  // 2^-60 <= rho < 2^60
}
__device__ __forceinline__ float refined_rcp(float b) {
  const float r0 = __builtin_amdgcn_rcpf(b);
  const float e = __fmaf_rn(-b, r0, 1.f);
  return __fmaf_rn(e, r0, r0);
}
__device__ __forceinline__ float div_with_rcp(float a, float b, float r) {
  float q = a * r;
  float e = __fmaf_rn(-b, q, a);
  q = __fmaf_rn(e, r, q);
  e = __fmaf_rn(-b, q, a);
  return __fmaf_rn(e, r, q);
}
// density and velocity with the bits of moments_exact, the two divides sharing one refined reciprocal
__device__ __forceinline__ void moments_shared(const float (&f)[kQ], float& rho, float& ux, float& uy) {
  float d = f[0];
#pragma unroll
  for (int k = 1; k < kQ; k++) d += f[k];
  rho = d;
  const float X = f[1] + f[5] + f[8] - (f[3] + f[6] + f[7]);
  const float Y = f[2] + f[5] + f[6] - (f[4] + f[7] + f[8]);
  if (density_in_plain_range(d)) {
    const float r = refined_rcp(d);
    ux = div_with_rcp(X, d, r);
    uy = div_with_rcp(Y, d, r);
  } else {
    ux = X / d;
    uy = Y / d;
  }
}

// SPEED: where |u| for the av_velocity sum comes from
//   0  the relaxed populations, IEEE sqrt -- the reference's own arithmetic (SerialCode/d2q9-bgk.c:426-450):
//      per-cell |u| bit-identical to the reference's
//   1  the pre-collision moments (BGK conserves density and momentum, so they equal the relaxed cell's up to
//      rounding, ~1e-7 relative), native v_sqrt_f32 (1 ulp): saves the second moment pass, ~50 VALU
//      instructions per cell.  The lattice is untouched by this choice; av_vels moves by < 1e-6 relative,
//      far inside the summation-order noise it already carries (the reference adds sequentially in fp32).
#ifndef LBM_STREAM_SPEED
#define LBM_STREAM_SPEED 1
#endif
template <int SPEED = 0>
__device__ __forceinline__ void collide_exact(const float (&t)[kQ], float omega, float (&r)[kQ],
                                              float& speed, bool want_speed) {
  float rho, ux, uy;
  moments_shared(t, rho, ux, uy);
  // |u|^2 below 5e28 bounds every dividend of the fast constant divides (squares of ux, uy,
  // ux+-uy are at most 2|u|^2 < 1e29); NaN compares false and takes the IEEE path
  const float u_sq = ux * ux + uy * uy;
  const bool ok = u_sq < 5.0e28f;
  if (ok) collide_exact_body<true>(t, omega, rho, ux, uy, r);
  else    collide_exact_body<false>(t, omega, rho, ux, uy, r);
  speed = 0.f;
  if (want_speed) {
    if constexpr (SPEED == 0) {
      // av_velocity() looks at the relaxed populations (SerialCode/d2q9-bgk.c:169, 426-450)
      float rho2, ux2, uy2;
      moments_shared(r, rho2, ux2, uy2);
      speed = sqrtf((ux2 * ux2) + (uy2 * uy2));  // IEEE: __fsqrt_rn is the native approximation
    } else {
      speed = __builtin_amdgcn_sqrtf(u_sq);
    }
  }
}
template <>
__device__ __forceinline__ void collide<true>(const float (&t)[kQ], float omega, float (&r)[kQ],
                                              float& speed, bool want_speed) {
  collide_exact<0>(t, omega, r, speed, want_speed);
}

// FAST: one reciprocal, multiplies by 3, 4.5, 1.5 and explicit FMAs.  BGK conserves density and
// momentum, so |u| of the relaxed cell is taken from the pre-collision moments.
template <>
__device__ __forceinline__ void collide<false>(const float (&t)[kQ], float omega, float (&r)[kQ],
                                               float& speed, bool /*want_speed*/) {
  const float rho = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7])) + t[8];
  const float inv = 1.f / rho;
  const float ux = ((t[1] + t[5] + t[8]) - (t[3] + t[6] + t[7])) * inv;
  const float uy = ((t[2] + t[5] + t[6]) - (t[4] + t[7] + t[8])) * inv;
  const float u_sq = __fmaf_rn(ux, ux, uy * uy);
  const float base = __fmaf_rn(-1.5f, u_sq, 1.f);
  const float w0r = omega * kW0 * rho, w1r = omega * kW1 * rho, w2r = omega * kW2 * rho;
  const float keep = 1.f - omega;
  auto relax = [&](float tk, float wr, float u) {
    const float poly = __fmaf_rn(u, __fmaf_rn(4.5f, u, 3.f), base);
    return __fmaf_rn(wr, poly, keep * tk);
  };
  r[0] = __fmaf_rn(w0r, base, keep * t[0]);
  r[1] = relax(t[1], w1r, ux);
  r[2] = relax(t[2], w1r, uy);
  r[3] = relax(t[3], w1r, -ux);
  r[4] = relax(t[4], w1r, -uy);
  r[5] = relax(t[5], w2r, ux + uy);
  r[6] = relax(t[6], w2r, uy - ux);
  r[7] = relax(t[7], w2r, -ux - uy);
  r[8] = relax(t[8], w2r, ux - uy);
  speed = __builtin_amdgcn_sqrtf(u_sq);  // v_sqrt_f32, 1 ulp
}

// accelerate_flow() on one cell (SerialCode/d2q9-bgk.c:229-242)
__device__ __forceinline__ void accelerate(float (&f)[kQ], float a1, float a2) {
  if ((f[3] - a1) > 0.f && (f[6] - a2) > 0.f && (f[7] - a2) > 0.f) {
    f[1] += a1;  f[5] += a2;  f[8] += a2;
    f[3] -= a1;  f[6] -= a2;  f[7] -= a2;
  }
}

// rebound(): mirrored copy, speed 0 kept (SerialCode/d2q9-bgk.c:291-298)
__device__ __forceinline__ void bounce(const float (&t)[kQ], float (&r)[kQ]) {
  r[0] = t[0];
  r[1] = t[3];  r[2] = t[4];  r[3] = t[1];  r[4] = t[2];
  r[5] = t[7];  r[6] = t[8];  r[7] = t[5];  r[8] = t[6];
}

// ---------------------------------------------------------------------------------------------
// workgroup reduction: wave64 shuffles, then one LDS hop across the 4 waves
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

template <int BLOCK = kBlock>
__device__ __forceinline__ float block_sum(float v) {
  __shared__ float wave_part[BLOCK / 64];
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_part[wave] = v;
  __syncthreads();
  float total = 0.f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) total += wave_part[w];
  }
  return total;  // valid in thread 0
}

// ---------------------------------------------------------------------------------------------
// fused step, 4 cells per lane (nx % 4 == 0, pitch % 4 == 0)
//
// MATH : 0 exact (reference arithmetic), 1 fast (reciprocal + FMA), 2 copy-through (tuning only)
// NEIGH: how the +-1 column neighbours of the six x-moving populations are obtained
//        0 = one strided dword load per plane (simple, but each touches as many cache lines as
//            the 16-byte load beside it),
//        1 = from the adjacent lane's aligned vector by a wave64 cross-lane move
//            (__shfl_up/down -> ds_bpermute_b32, no LDS storage); only the first / last lane of a
//            wave and the row ends load a dword,
//        2 = the same with DPP wave_shr:1 / wave_shl:1 (one VALU move, no LDS crossbar).
// NTS  : nontemporal stores.
// ---------------------------------------------------------------------------------------------
template <int NEIGH>
__device__ __forceinline__ float lane_from_west(float v) {  // lane i <- lane i-1
  if constexpr (NEIGH == 2)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
  else
    return __shfl_up(v, 1, 64);
}
template <int NEIGH>
__device__ __forceinline__ float lane_from_east(float v) {  // lane i <- lane i+1
  if constexpr (NEIGH == 2)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
  else
    return __shfl_down(v, 1, 64);
}

template <bool NTS>
__device__ __forceinline__ void store4(float* p, float a, float b, float c, float d) {
  if constexpr (NTS) {
    typedef float v4 __attribute__((ext_vector_type(4)));
    v4 v = {a, b, c, d};
    __builtin_nontemporal_store(v, reinterpret_cast<v4*>(p));
  } else {
    *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
  }
}

template <int MATH, int NEIGH, bool NTS, int BLOCK = kBlock, bool SYNC = false>
__global__ __launch_bounds__(BLOCK) void step_vec4(const StepArgs a) {
  const int quads_x = a.nx >> 2;
  const long n_quads = (long)quads_x * a.n_rows;
  // alternate the sweep direction from step to step: the rows written last by the previous step
  // (still in L2 / Infinity Cache) are then the first ones read
  const long tile = a.reverse ? (long)(gridDim.x - 1 - blockIdx.x) : (long)blockIdx.x;
  const long q = tile * BLOCK + threadIdx.x;
  const bool active = q < n_quads;
  const long ps = a.plane_stride;
  float my_sum = 0.f;
  float r[4][kQ];
  int row = 0, x0 = 0;

  if (active) {
    const int rsel = (int)(q / quads_x);
    x0 = (int)(q - (long)rsel * quads_x) << 2;
    row = a.row_first + rsel * a.row_stride;

    // neighbour columns with periodic wrap (SerialCode/d2q9-bgk.c:258,260)
    const int xw = (x0 == 0) ? a.nx - 1 : x0 - 1;
    const int xe = (x0 + 4 == a.nx) ? 0 : x0 + 4;

    const float* c_row = a.src + (long)row * a.row_pitch;  // plane 0, this row
    // row below (speeds 2,5,6 arrive from it) and above (4,7,8), :257,259.  In a multi-slab run the
    // slab is surrounded by halo rows (-1 and `rows`) that hold the neighbours' boundary rows.
    const int rs = (row == 0 && a.wrap) ? a.rows - 1 : row - 1;
    const int rn = (row == a.rows - 1 && a.wrap) ? 0 : row + 1;
    const float* sb = a.src + (long)rs * a.row_pitch;
    const float* nb = a.src + (long)rn * a.row_pitch;
    const float *s2 = sb + 2 * ps, *s5 = sb + 5 * ps, *s6 = sb + 6 * ps;
    const float *n4 = nb + 4 * ps, *n7 = nb + 7 * ps, *n8 = nb + 8 * ps;

    // 9 aligned 16-byte loads
    const float4 v0 = *reinterpret_cast<const float4*>(c_row + x0);
    const float4 v1 = *reinterpret_cast<const float4*>(c_row + 1 * ps + x0);
    const float4 v3 = *reinterpret_cast<const float4*>(c_row + 3 * ps + x0);
    const float4 v2 = *reinterpret_cast<const float4*>(s2 + x0);
    const float4 v5 = *reinterpret_cast<const float4*>(s5 + x0);
    const float4 v6 = *reinterpret_cast<const float4*>(s6 + x0);
    const float4 v4 = *reinterpret_cast<const float4*>(n4 + x0);
    const float4 v7 = *reinterpret_cast<const float4*>(n7 + x0);
    const float4 v8 = *reinterpret_cast<const float4*>(n8 + x0);
    // the cell just west of the quad (for speeds 1,5,8) and just east of it (3,6,7)
    float e1, e3, e5, e6, e7, e8;
    if constexpr (NEIGH == 0) {
      e1 = c_row[1 * ps + xw];  // speed 1 travels east: comes from the west cell
      e3 = c_row[3 * ps + xe];
      e5 = s5[xw];
      e6 = s6[xe];
      e7 = n7[xe];
      e8 = n8[xw];
    } else {
      const int lane = threadIdx.x & 63;
      e1 = lane_from_west<NEIGH>(v1.w);
      e5 = lane_from_west<NEIGH>(v5.w);
      e8 = lane_from_west<NEIGH>(v8.w);
      e3 = lane_from_east<NEIGH>(v3.x);
      e6 = lane_from_east<NEIGH>(v6.x);
      e7 = lane_from_east<NEIGH>(v7.x);
      // the wave's first / last lane and the row ends have no such lane: one dword each
      if (lane == 0 || x0 == 0) {
        e1 = c_row[1 * ps + xw];  e5 = s5[xw];  e8 = n8[xw];
      }
      if (lane == 63 || x0 + 4 == a.nx || q + 1 == n_quads) {
        e3 = c_row[3 * ps + xe];  e6 = s6[xe];  e7 = n7[xe];
      }
    }
    const uchar4 m = *reinterpret_cast<const uchar4*>(a.mask + (long)row * a.pitch + x0);

    // streamed populations of the 4 cells: t[j][k]
    float t[4][kQ] = {
        {v0.x, e1,   v2.x, v3.y, v4.x, e5,   v6.y, v7.y, e8},
        {v0.y, v1.x, v2.y, v3.z, v4.y, v5.x, v6.z, v7.z, v8.x},
        {v0.z, v1.y, v2.z, v3.w, v4.z, v5.y, v6.w, v7.w, v8.y},
        {v0.w, v1.z, v2.w, e3,   v4.w, v5.z, e6,   e7,   v8.z}};
    const unsigned char blocked[4] = {m.x, m.y, m.z, m.w};
    const bool lid = (row == a.accel_row);

#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (blocked[j]) {
        bounce(t[j], r[j]);
      } else {
        float speed = 0.f;
        if constexpr (MATH == 0) collide<true>(t[j], a.omega, r[j], speed);
        else if constexpr (MATH == 1) collide<false>(t[j], a.omega, r[j], speed);
        else {
#pragma unroll
          for (int k = 0; k < kQ; k++) r[j][k] = t[j][k];
        }
        my_sum += speed;
        if (lid) accelerate(r[j], a.a1, a.a2);
      }
    }
  }

  // optionally let the whole workgroup reach its stores together (one contiguous burst per plane)
  if constexpr (SYNC) __syncthreads();

  if (active) {
    float* d_row = a.dst + (long)row * a.row_pitch + x0;
#pragma unroll
    for (int k = 0; k < kQ; k++) store4<NTS>(d_row + k * ps, r[0][k], r[1][k], r[2][k], r[3][k]);

  }

  const float total = block_sum<BLOCK>(my_sum);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------------------------
// TWO timesteps per pass over memory (temporal blocking); periodic in x, in y either periodic (single
// slab) or fed by the two halo rows stored below and above a slab (wrap = 0).
//
// The one-step kernel above sits at the float4-copy ceiling of the chip (72 B per update cannot
// move faster).  The only way past that roofline is to move fewer bytes: this kernel advances the
// lattice by two steps while reading it once and writing it once (36 B per update).
//
// One WAVE (64 lanes, no LDS, no barrier) owns a vertical strip of 62 quads (248 cells; lanes 0
// and 63 are halo quads that only feed their neighbours) and sweeps a band of rows upwards.
// Per row iteration it
//   1. pulls row r of the source lattice and relaxes it            -> step t   results N (registers)
//   2. relaxes row r-1 a second time from a sliding window of step-t results kept in registers:
//        speeds 2,5,6 of row r-2, speeds 0,1,3 of row r-1, speeds 4,7,8 of row r (= N);
//      the +-1 column neighbours come from the adjacent lanes (DPP wave_shr:1 / wave_shl:1)
//                                                                   -> step t+1 results, stored
//   3. rotates the window.
// Every step-t value is consumed exactly once, so the window is 36 floats per lane and nothing
// is staged in LDS.  Redundant work: 2 of 64 lanes and 2 warm-up rows per band.
// Per-cell arithmetic is the same code as the one-step kernel: results stay bit-identical.
//
// accelerate_flow: step t+1's acceleration is applied to the step-t results of the lid row
// (always); step t+2's to the stored results when accel_after != 0 (not on the last step of a run).
// ---------------------------------------------------------------------------------------------
struct Step2Args : LatticeArgs {
  int rows;        // rows owned by the slab
  int wrap;        // 1: rows wrap periodically (single slab); 0: two halo rows surround the slab
  int band_rows;   // output rows per wave (band height)
  int row_first;   // band b of this launch starts at row_first + b*band_pitch ...
  int band_pitch;  // (= band_rows for a contiguous region)
  int row_end;     // ... and ends before row_end
  int n_strips;    // waves across x
  int accel_row;
  int accel_after;
  float omega, a1, a2;
  float* partials1;  // per wave: sum |u| after step t   (own cells only)
  float* partials2;  // per wave: sum |u| after step t+1
};

constexpr int kStripQuads = 62;  // output lanes per wave (lanes 1..62; each owns C cells)

template <int MATH, int SPEED = 0>
__device__ __forceinline__ void relax_cell(const float (&t)[kQ], bool blocked, bool lid, float omega, float a1,
                                           float a2, float (&r)[kQ], float& speed, bool want_speed = true) {
  speed = 0.f;
  if (blocked) {
    bounce(t, r);
  } else {
    if constexpr (MATH == 0) collide_exact<SPEED>(t, omega, r, speed, want_speed);
    else collide<false>(t, omega, r, speed, want_speed);
    if (lid) accelerate(r, a1, a2);
  }
}

// the 9 aligned vectors and the mask bytes one lane pulls for one row; C cells per lane
template <int C>
struct RowPull {
  typedef float vec __attribute__((ext_vector_type(C)));
  vec v[kQ];
  unsigned m;  // C mask bytes
};

template <int C>
__device__ __forceinline__ RowPull<C> pull_row(const Step2Args& a, int r, int x0) {
  typedef typename RowPull<C>::vec vec;
  const long ps = a.plane_stride;
  const int rs = (r == 0 && a.wrap) ? a.rows - 1 : r - 1;
  const int rn = (r == a.rows - 1 && a.wrap) ? 0 : r + 1;
  const float* c_row = a.src + (long)r * a.row_pitch + x0;
  const float* sb = a.src + (long)rs * a.row_pitch + x0;
  const float* nb = a.src + (long)rn * a.row_pitch + x0;
  RowPull<C> p;
  p.v[0] = *reinterpret_cast<const vec*>(c_row);
  p.v[1] = *reinterpret_cast<const vec*>(c_row + 1 * ps);
  p.v[3] = *reinterpret_cast<const vec*>(c_row + 3 * ps);
  p.v[2] = *reinterpret_cast<const vec*>(sb + 2 * ps);
  p.v[5] = *reinterpret_cast<const vec*>(sb + 5 * ps);
  p.v[6] = *reinterpret_cast<const vec*>(sb + 6 * ps);
  p.v[4] = *reinterpret_cast<const vec*>(nb + 4 * ps);
  p.v[7] = *reinterpret_cast<const vec*>(nb + 7 * ps);
  p.v[8] = *reinterpret_cast<const vec*>(nb + 8 * ps);
  const unsigned char* mp = a.mask + (long)r * a.pitch + x0;
  if constexpr (C == 4) p.m = *reinterpret_cast<const unsigned*>(mp);
  else if constexpr (C == 2) p.m = *reinterpret_cast<const unsigned short*>(mp);
  else p.m = *mp;
  return p;
}

// periodic single slab: fold the row index; multi-slab: rows -2..rows+1 exist as halo rows
__device__ __forceinline__ int wrap_row(int r, int rows, int wrap) {
  if (wrap) {
    if (r < 0) r += rows;
    if (r >= rows) r -= rows;
  }
  return r;
}

// C = cells per lane (4: 16-byte accesses, 138 VGPRs, 3 waves/SIMD; 2: 8-byte accesses, about half
// the registers, twice the waves -- better for slabs too small to fill the chip with 4-cell lanes)
template <int MATH, bool NTS, int C>
__global__ __launch_bounds__(64) void step2_stream(const Step2Args a) {
  typedef typename RowPull<C>::vec vec;
  const int lane = threadIdx.x;
  const int strip = blockIdx.x % a.n_strips;
  const int units_x = a.nx / C;
  const int y0 = a.row_first + (int)(blockIdx.x / a.n_strips) * a.band_pitch;
  const int band_n = min(a.band_rows, a.row_end - y0);

  // this lane's group of C cells (may lie outside the grid: halo lanes and the tail of the last
  // strip wrap around)
  const int ux_raw = strip * kStripQuads + lane - 1;
  int ux = ux_raw % units_x;
  if (ux < 0) ux += units_x;
  const int x0 = ux * C;
  const bool out_lane = (lane >= 1) && (lane <= kStripQuads) && (ux_raw < units_x);
  const long ps = a.plane_stride;

  // sliding window of step-t results (registers)
  float w256[3][C];  // speeds 2,5,6 of row r-2
  float w013[3][C];  // speeds 0,1,3 of row r-1
  float n256[3][C];  // speeds 2,5,6 of row r-1 (become w256 after the rotation)
  unsigned m_prev = 0;
  float sum1 = 0.f, sum2 = 0.f;

  for (int i = 0; i < band_n + 2; i++) {
    // ---- step t on row r ------------------------------------------------------------------
    const int r = wrap_row(y0 - 1 + i, a.rows, a.wrap);
    const RowPull<C> p = pull_row<C>(a, r, x0);
    // +-1 column neighbours of the pulled vectors come from the adjacent lanes.  Lane 0 has no
    // west lane and lane 63 no east lane: their outermost cells get zeros and produce garbage,
    // which nothing consumes (those lanes are halo groups; only their inner edge feeds a neighbour).
    const float e1 = lane_from_west<2>(p.v[1][C - 1]), e5 = lane_from_west<2>(p.v[5][C - 1]),
                e8 = lane_from_west<2>(p.v[8][C - 1]);
    const float e3 = lane_from_east<2>(p.v[3][0]), e6 = lane_from_east<2>(p.v[6][0]),
                e7 = lane_from_east<2>(p.v[7][0]);

    float t[C][kQ];
#pragma unroll
    for (int j = 0; j < C; j++) {
      const int jw = (j == 0) ? 0 : j - 1, je = (j == C - 1) ? C - 1 : j + 1;
      t[j][0] = p.v[0][j];
      t[j][1] = (j == 0) ? e1 : p.v[1][jw];
      t[j][2] = p.v[2][j];
      t[j][3] = (j == C - 1) ? e3 : p.v[3][je];
      t[j][4] = p.v[4][j];
      t[j][5] = (j == 0) ? e5 : p.v[5][jw];
      t[j][6] = (j == C - 1) ? e6 : p.v[6][je];
      t[j][7] = (j == C - 1) ? e7 : p.v[7][je];
      t[j][8] = (j == 0) ? e8 : p.v[8][jw];
    }
    const bool lid = (r == a.accel_row);
    const bool own_row = (i >= 1) && (i <= band_n);  // rows y0 .. y0+band_n-1 belong to this band
    float N[C][kQ];
#pragma unroll
    for (int j = 0; j < C; j++) {
      float speed;
      relax_cell<MATH, LBM_STREAM_SPEED>(t[j], ((p.m >> (8 * j)) & 0xffu) != 0, lid, a.omega, a.a1, a.a2, N[j], speed, own_row);
      if (own_row && out_lane) sum1 += speed;
    }

    // ---- step t+1 on row r-1 (needs step-t rows r-2, r-1, r) -------------------------------
    if (i >= 2) {
      const int ro = wrap_row(r - 1, a.rows, a.wrap);
      // neighbours in x from the adjacent lanes: west cell = lane-1's last cell, east = lane+1's first
      const float w1 = lane_from_west<2>(w013[1][C - 1]);
      const float w5 = lane_from_west<2>(w256[1][C - 1]);
      const float w8 = lane_from_west<2>(N[C - 1][8]);
      const float x3 = lane_from_east<2>(w013[2][0]);
      const float x6 = lane_from_east<2>(w256[2][0]);
      const float x7 = lane_from_east<2>(N[0][7]);
      float u[C][kQ];
#pragma unroll
      for (int j = 0; j < C; j++) {
        const int jw = (j == 0) ? 0 : j - 1, je = (j == C - 1) ? C - 1 : j + 1;
        u[j][0] = w013[0][j];
        u[j][1] = (j == 0) ? w1 : w013[1][jw];
        u[j][2] = w256[0][j];
        u[j][3] = (j == C - 1) ? x3 : w013[2][je];
        u[j][4] = N[j][4];
        u[j][5] = (j == 0) ? w5 : w256[1][jw];
        u[j][6] = (j == C - 1) ? x6 : w256[2][je];
        u[j][7] = (j == C - 1) ? x7 : N[je][7];
        u[j][8] = (j == 0) ? w8 : N[jw][8];
      }
      const bool lid2 = (ro == a.accel_row) && a.accel_after;
      float R[C][kQ];
#pragma unroll
      for (int j = 0; j < C; j++) {
        float speed;
        relax_cell<MATH, LBM_STREAM_SPEED>(u[j], ((m_prev >> (8 * j)) & 0xffu) != 0, lid2, a.omega, a.a1, a.a2, R[j], speed);
        if (out_lane) sum2 += speed;
      }
      if (out_lane) {
        float* d_row = a.dst + (long)ro * a.row_pitch + x0;
#pragma unroll
        for (int k = 0; k < kQ; k++) {
          vec o;
#pragma unroll
          for (int j = 0; j < C; j++) o[j] = R[j][k];
          if constexpr (NTS) __builtin_nontemporal_store(o, reinterpret_cast<vec*>(d_row + k * ps));
          else *reinterpret_cast<vec*>(d_row + k * ps) = o;
        }
      }
    }

    // ---- rotate the window ------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < C; j++) {
      w256[0][j] = n256[0][j];  w256[1][j] = n256[1][j];  w256[2][j] = n256[2][j];
      n256[0][j] = N[j][2];     n256[1][j] = N[j][5];     n256[2][j] = N[j][6];
      w013[0][j] = N[j][0];     w013[1][j] = N[j][1];     w013[2][j] = N[j][3];
    }
    m_prev = p.m;
  }

  sum1 = wave_sum(sum1);
  sum2 = wave_sum(sum2);
  if (lane == 0) {
    a.partials1[blockIdx.x] = sum1;
    a.partials2[blockIdx.x] = sum2;
  }
}

// ---------------------------------------------------------------------------------------------
// K timesteps per pass over memory (K = 2, 3 or 4): the sliding register window of step2_stream generalised
// to a chain of K-1 windows.  The two-step kernel at 8192^2 is bound by DRAM traffic (round-2 PMC: 5.4-5.8 TB/s
// at the memory controllers whatever the band height and however cheap the arithmetic), so the only way
// on is fewer bytes per update: K = 3 reads and writes the lattice once per THREE updates (24 B per update).
//
// Iteration i of a wave pulls row r = y0 - (K-1) + i and relaxes it (stage 1); stage s+1 then relaxes row
// r - s from window s (speeds 2,5,6 of row r-s-1, speeds 0,1,3 of row r-s) and the stage-s results of row
// r-s+1 just produced (speeds 4,7,8), +-1 columns by DPP from the adjacent lanes; the last stage's row
// r - (K-1) is stored.  Every intermediate value is consumed exactly once: 36 floats per window and lane.
// Redundant work: 2 of 64 lanes (with 4 cells per lane one halo lane per side covers up to four steps: after
// stage s the s cells of a halo lane nearest the strip's edge are garbage, and stage s+1 of the first owned
// cell needs the halo lane's LAST cell of stage s) and 2(K-1) warm-up rows per band in stage 1, 2(K-2) in
// stage 2, ...  Per-cell arithmetic is relax_cell, as in every other kernel: the lattice stays bit-identical.
//
// PREFETCH: the next row's nine vectors are requested before the current row is relaxed (36 more VGPRs; with
// two resident waves per SIMD the loads of one wave would otherwise only overlap the other wave's arithmetic
// when the two happen to be out of phase).
// XCD: workgroups are handed to the 8 XCDs round-robin; with chunk > 0, consecutive workgroups OF ONE XCD take
// horizontally adjacent strips of one band (a chunk), so the 128-byte lines that straddle two strips
// (a strip is 62 x 16 B = 992 B wide) are fetched from the fabric once per chunk instead of once per strip.
// ---------------------------------------------------------------------------------------------
struct StepKArgs : LatticeArgs {
  int rows;        // rows owned by the slab
  int wrap;        // 1: rows wrap periodically (single slab); 0: K halo rows surround the slab
  int band_rows;   // output rows per wave (band height)
  int row_first;   // band b of this launch starts at row_first + b*band_pitch ...
  int band_pitch;  // (= band_rows for a contiguous region)
  int row_end;     // ... and ends before row_end
  int n_strips;    // waves across x
  int n_bands;     // bands of this launch
  int chunk;       // strips per XCD chunk (0: plain order, strip fastest)
  int halo_lanes;  // lanes at each end of a wave that only feed their neighbours: ceil(K / cells per lane) of the context
  int accel_row;
  int accel_row2;  // a second periodic image of the lid row among the halo rows, or kNoRow
  int accel_after;
  float omega, a1, a2;
  float* partials;      // partials[s * slot_stride + wave] = sum |u| after step t+s (own cells only)
  long slot_stride;
};

template <int C>
struct Window {
  float w256[3][C];  // speeds 2,5,6 of the row two below the newest
  float w013[3][C];  // speeds 0,1,3 of the row below the newest
  float n256[3][C];  // speeds 2,5,6 of the row below the newest (become w256 after the rotation)
  unsigned m;        // mask bytes of the row below the newest
};

template <int MATH, bool NTS, int C, int K, bool PREFETCH>
__global__ __launch_bounds__(64, (K >= 3 || PREFETCH || MATH == 0) ? 2 : 3) void stepk_stream(const StepKArgs a) {
  static_assert(K >= 2 && K <= 4 && (C == 4 || K == 2), "one halo lane per side covers K <= C steps");
  typedef typename RowPull<C>::vec vec;
  const int lane = threadIdx.x;
  int strip, band;
  if (a.chunk > 0) {
    // workgroup w runs on XCD w % 8 as that XCD's (w / 8)-th workgroup; chunk g = (strips [h*chunk, (h+1)*chunk) of band b)
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int chunks_per_band = (a.n_strips + a.chunk - 1) / a.chunk;
    const int g = (j / a.chunk) * 8 + xcd;
    band = g / chunks_per_band;
    strip = (g - band * chunks_per_band) * a.chunk + j % a.chunk;
    if (band >= a.n_bands || strip >= a.n_strips) return;
  } else {
    strip = blockIdx.x % a.n_strips;
    band = blockIdx.x / a.n_strips;
  }
  const int wave_id = band * a.n_strips + strip;
  const int units_x = a.nx / C;
  const int y0 = a.row_first + band * a.band_pitch;
  const int band_n = min(a.band_rows, a.row_end - y0);

  const int H = a.halo_lanes;  // H * C >= K cells of halo per side
  const int ux_raw = strip * (64 - 2 * H) + lane - H;
  int ux = ux_raw % units_x;
  if (ux < 0) ux += units_x;
  const int x0 = ux * C;
  const bool out_lane = (lane >= H) && (lane < 64 - H) && (ux_raw < units_x);
  const long ps = a.plane_stride;

  Step2Args pa;  // pull_row's view of the arguments
  pa.src = a.src;  pa.mask = a.mask;  pa.plane_stride = a.plane_stride;  pa.row_pitch = a.row_pitch;
  pa.pitch = a.pitch;  pa.rows = a.rows;  pa.wrap = a.wrap;

  Window<C> win[K - 1];
#pragma unroll
  for (int s = 0; s < K - 1; s++) {
    win[s].m = 0;
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
      for (int j = 0; j < C; j++) win[s].w256[q][j] = win[s].w013[q][j] = win[s].n256[q][j] = 0.f;
  }
  float sum[K];
#pragma unroll
  for (int s = 0; s < K; s++) sum[s] = 0.f;

  const int n_iter = band_n + 2 * (K - 1);
  RowPull<C> nextp;
  if constexpr (PREFETCH) nextp = pull_row<C>(pa, wrap_row(y0 - (K - 1), a.rows, a.wrap), x0);

  for (int i = 0; i < n_iter; i++) {
    // ---- stage 1: step t on row r, pulled from memory -------------------------------------------
    const int r = wrap_row(y0 - (K - 1) + i, a.rows, a.wrap);
    RowPull<C> p;
    if constexpr (PREFETCH) {
      p = nextp;
      if (i + 1 < n_iter) nextp = pull_row<C>(pa, wrap_row(y0 - (K - 1) + i + 1, a.rows, a.wrap), x0);
    } else {
      p = pull_row<C>(pa, r, x0);
    }
    float cur[C][kQ];
    {
      const float e1 = lane_from_west<2>(p.v[1][C - 1]), e5 = lane_from_west<2>(p.v[5][C - 1]),
                  e8 = lane_from_west<2>(p.v[8][C - 1]);
      const float e3 = lane_from_east<2>(p.v[3][0]), e6 = lane_from_east<2>(p.v[6][0]),
                  e7 = lane_from_east<2>(p.v[7][0]);
      const bool lid = (r == a.accel_row) || (r == a.accel_row2);
      const bool own_row = (i >= K - 1) && (i < band_n + K - 1);
#pragma unroll
      for (int j = 0; j < C; j++) {
        const int jw = (j == 0) ? 0 : j - 1, je = (j == C - 1) ? C - 1 : j + 1;
        const float t[kQ] = {p.v[0][j],
                             (j == 0) ? e1 : p.v[1][jw],
                             p.v[2][j],
                             (j == C - 1) ? e3 : p.v[3][je],
                             p.v[4][j],
                             (j == 0) ? e5 : p.v[5][jw],
                             (j == C - 1) ? e6 : p.v[6][je],
                             (j == C - 1) ? e7 : p.v[7][je],
                             (j == 0) ? e8 : p.v[8][jw]};
        float speed;
        relax_cell<MATH, LBM_STREAM_SPEED>(t, ((p.m >> (8 * j)) & 0xffu) != 0, lid, a.omega, a.a1, a.a2, cur[j], speed,
                                           own_row);
        if (own_row && out_lane) sum[0] += speed;
      }
    }
    unsigned m_cur = p.m;  // mask bytes of the row `cur` belongs to

    // ---- stages 2..K: step t+s on row r-s from window s and the stage-s results of row r-s+1 ----
#pragma unroll
    for (int s = 1; s < K; s++) {
      Window<C>& w = win[s - 1];
      float nxt[C][kQ];
      const bool active = (i >= 2 * s);
      if (active) {
        const int ro = wrap_row(y0 - (K - 1) + i - s, a.rows, a.wrap);
        const float w1 = lane_from_west<2>(w.w013[1][C - 1]);
        const float w5 = lane_from_west<2>(w.w256[1][C - 1]);
        const float w8 = lane_from_west<2>(cur[C - 1][8]);
        const float x3 = lane_from_east<2>(w.w013[2][0]);
        const float x6 = lane_from_east<2>(w.w256[2][0]);
        const float x7 = lane_from_east<2>(cur[0][7]);
        const bool last = (s == K - 1);
        const bool lid = ((ro == a.accel_row) || (ro == a.accel_row2)) && (!last || a.accel_after);
        // rows of this band: ro in [y0, y0 + band_n)  <=>  i - s - (K-1) in [0, band_n)
        const bool own_row = (i - s >= K - 1) && (i - s < band_n + K - 1);
#pragma unroll
        for (int j = 0; j < C; j++) {
          const int jw = (j == 0) ? 0 : j - 1, je = (j == C - 1) ? C - 1 : j + 1;
          const float u[kQ] = {w.w013[0][j],
                               (j == 0) ? w1 : w.w013[1][jw],
                               w.w256[0][j],
                               (j == C - 1) ? x3 : w.w013[2][je],
                               cur[j][4],
                               (j == 0) ? w5 : w.w256[1][jw],
                               (j == C - 1) ? x6 : w.w256[2][je],
                               (j == C - 1) ? x7 : cur[je][7],
                               (j == 0) ? w8 : cur[jw][8]};
          float speed;
          relax_cell<MATH, LBM_STREAM_SPEED>(u, ((w.m >> (8 * j)) & 0xffu) != 0, lid, a.omega, a.a1, a.a2, nxt[j], speed,
                                             own_row);
          if (own_row && out_lane) sum[s] += speed;
        }
      }
      // rotate window s with the stage-s row just consumed
      const unsigned m_below = w.m;
#pragma unroll
      for (int j = 0; j < C; j++) {
        w.w256[0][j] = w.n256[0][j];  w.w256[1][j] = w.n256[1][j];  w.w256[2][j] = w.n256[2][j];
        w.n256[0][j] = cur[j][2];     w.n256[1][j] = cur[j][5];     w.n256[2][j] = cur[j][6];
        w.w013[0][j] = cur[j][0];     w.w013[1][j] = cur[j][1];     w.w013[2][j] = cur[j][3];
      }
      w.m = m_cur;
      if (!active) break;
      m_cur = m_below;
#pragma unroll
      for (int j = 0; j < C; j++)
#pragma unroll
        for (int k = 0; k < kQ; k++) cur[j][k] = nxt[j][k];
      if (s == K - 1 && out_lane) {
        const int ro = wrap_row(y0 - (K - 1) + i - s, a.rows, a.wrap);
        float* d_row = a.dst + (long)ro * a.row_pitch + x0;
#pragma unroll
        for (int k = 0; k < kQ; k++) {
          vec o;
#pragma unroll
          for (int j = 0; j < C; j++) o[j] = cur[j][k];
          if constexpr (NTS) __builtin_nontemporal_store(o, reinterpret_cast<vec*>(d_row + k * ps));
          else *reinterpret_cast<vec*>(d_row + k * ps) = o;
        }
      }
    }
  }

#pragma unroll
  for (int s = 0; s < K; s++) {
    const float tot = wave_sum(sum[s]);
    if (lane == 0) a.partials[(long)s * a.slot_stride + wave_id] = tot;
  }
}

// ---------------------------------------------------------------------------------------------
// Packed arithmetic: two cells per instruction.
//
// With three or four timesteps per pass the stream kernel is bound by VALU issue again (a plain wave64 VALU
// instruction holds a CDNA4 SIMD for 4 cycles whatever it computes).  gfx950 has packed fp32 VALU operations
// (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32): one instruction, two independent IEEE fp32 results.  A lane's
// four cells are therefore kept as two PAIRS (cells 0,1 and 2,3: the two halves of the 16-byte vectors the lane
// loads and stores) and the whole collision is written on pairs.  Every packed operation below is the same
// IEEE operation, in the same order, as in collide_exact / collide_exact_body / moments_shared -- results are
// bit-identical; only the instruction count halves.  What cannot be packed stays per cell: v_rcp_f32, the range
// guards, v_sqrt_f32.  Blocked cells and the (rare, wave-uniform) lid row are patched afterwards; a lane whose
// guards fail (density outside [2^-60, 2^60) or |u|^2 >= 5e28: never in a physical run) recomputes its four
// cells with the scalar code, so the exactness argument of div_const_fast holds unchanged.
// ---------------------------------------------------------------------------------------------
typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f2 splat2(float v) { return f2{v, v}; }
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 div_const_fast2(f2 x, float C, float R) {
  const f2 q = x * splat2(R);
  const f2 r = fma2(splat2(-C), q, x);
  return fma2(r, splat2(R), q);
}
__device__ __forceinline__ f2 div_with_rcp2(f2 a, f2 b, f2 r) {
  f2 q = a * r;
  f2 e = fma2(-b, q, a);
  q = fma2(e, r, q);
  e = fma2(-b, q, a);
  return fma2(e, r, q);
}

// One PAIR of cells of one row, no exceptions: stream inputs f[k] -> relaxed r[k] as if both cells were fluid
// cells of an ordinary row; u_sq = their |u|^2 (pre-collision moments); returns false when a guard of the fast
// constant divides / the shared reciprocal fails for either cell.
__device__ __forceinline__ bool relax_pair_core(const f2 (&f)[kQ], float omega, f2 (&r)[kQ], f2& u_sq) {
  constexpr float kInvCsq = 1.0f / kCsq, kInvTwoCsq = 1.0f / kTwoCsq, kInvTwoCsqSq = 1.0f / kTwoCsqSq;
  f2 d = f[0];
#pragma unroll
  for (int k = 1; k < kQ; k++) d = d + f[k];
  const f2 X = ((f[1] + f[5]) + f[8]) - ((f[3] + f[6]) + f[7]);
  const f2 Y = ((f[2] + f[5]) + f[6]) - ((f[4] + f[7]) + f[8]);
  bool ok = density_in_plain_range(d.x) && density_in_plain_range(d.y);
  const f2 r0 = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
  const f2 e0 = fma2(-d, r0, splat2(1.f));
  const f2 rr = fma2(e0, r0, r0);
  const f2 ux = div_with_rcp2(X, d, rr);
  const f2 uy = div_with_rcp2(Y, d, rr);
  const f2 uxx = ux * ux, uyy = uy * uy;
  u_sq = uxx + uyy;
  ok = ok && (u_sq.x < 5.0e28f) && (u_sq.y < 5.0e28f);
  const f2 usq_term = div_const_fast2(u_sq, kTwoCsq, kInvTwoCsq);
  const f2 one = splat2(1.f), om = splat2(omega);
  {
    const f2 w0r = splat2(kW0) * d;
    r[0] = f[0] + om * (w0r * (one - usq_term) - f[0]);
  }
  {
    const f2 w1r = splat2(kW1) * d;
    const f2 x1 = div_const_fast2(ux, kCsq, kInvCsq), x2 = div_const_fast2(uxx, kTwoCsqSq, kInvTwoCsqSq);
    r[1] = f[1] + om * (w1r * (((one + x1) + x2) - usq_term) - f[1]);
    r[3] = f[3] + om * (w1r * (((one - x1) + x2) - usq_term) - f[3]);
    const f2 y1 = div_const_fast2(uy, kCsq, kInvCsq), y2 = div_const_fast2(uyy, kTwoCsqSq, kInvTwoCsqSq);
    r[2] = f[2] + om * (w1r * (((one + y1) + y2) - usq_term) - f[2]);
    r[4] = f[4] + om * (w1r * (((one - y1) + y2) - usq_term) - f[4]);
  }
  {
    const f2 w2r = splat2(kW2) * d;
    const f2 us = ux + uy, ud = uy - ux;  // -ux + uy
    const f2 s1 = div_const_fast2(us, kCsq, kInvCsq), s2 = div_const_fast2(us * us, kTwoCsqSq, kInvTwoCsqSq);
    r[5] = f[5] + om * (w2r * (((one + s1) + s2) - usq_term) - f[5]);
    r[7] = f[7] + om * (w2r * (((one - s1) + s2) - usq_term) - f[7]);
    const f2 d1 = div_const_fast2(ud, kCsq, kInvCsq), d2 = div_const_fast2(ud * ud, kTwoCsqSq, kInvTwoCsqSq);
    r[6] = f[6] + om * (w2r * (((one + d1) + d2) - usq_term) - f[6]);
    r[8] = f[8] + om * (w2r * (((one - d1) + d2) - usq_term) - f[8]);
  }
  return ok;
}

// the exceptions of a pair.  Blocked cells bounce back (rebound(): the mirrored copy of the streamed populations,
// speed 0 kept, SerialCode/d2q9-bgk.c:291-298): a select per population half under ONE wave-level branch -- on the
// reference's geometry (walls every few hundred columns) a third of all pair relaxations meet a blocked cell somewhere
// in the wave, and the per-cell scalar path they used to take cost 13.5 % of the 8192^2 step (0.2826 vs 0.2443 ms
// without obstacles).  The lid row is accelerated by selects too (accelerate_select: the resident kernel's band
// that holds the lid row sets the pace of all the others, and the scalar path cost it 2.4 x the collision time);
// only a failed guard sends a cell through the scalar code (IEEE divides): rare, per cell.  sp0 / sp1: the cells' |u|
// (0 for blocked cells).
__device__ __forceinline__ void bounce_select(const f2 (&f)[kQ], bool b0, bool b1, f2 (&r)[kQ], float& sp0, float& sp1) {
  constexpr int opp[kQ] = {0, 3, 4, 1, 2, 7, 8, 5, 6};
#pragma unroll
  for (int k = 0; k < kQ; k++) {
    r[k].x = b0 ? f[opp[k]].x : r[k].x;
    r[k].y = b1 ? f[opp[k]].y : r[k].y;
  }
  sp0 = b0 ? 0.f : sp0;
  sp1 = b1 ? 0.f : sp1;
}
// accelerate_flow on the relaxed cells of a pair (SerialCode/d2q9-bgk.c:196-213), per cell where c0 / c1 says so: the
// same three tests and six sums as accelerate(), as selects
__device__ __forceinline__ void accelerate_select(f2 (&r)[kQ], bool c0, bool c1, float a1, float a2) {
  const bool g0 = c0 && (r[3].x - a1) > 0.f && (r[6].x - a2) > 0.f && (r[7].x - a2) > 0.f;
  const bool g1 = c1 && (r[3].y - a1) > 0.f && (r[6].y - a2) > 0.f && (r[7].y - a2) > 0.f;
  constexpr int plus[3] = {1, 5, 8}, minus[3] = {3, 6, 7};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float a = (i == 0) ? a1 : a2;
    const f2 up = f2{r[plus[i]].x + a, r[plus[i]].y + a}, dn = f2{r[minus[i]].x - a, r[minus[i]].y - a};
    r[plus[i]] = f2{g0 ? up.x : r[plus[i]].x, g1 ? up.y : r[plus[i]].y};
    r[minus[i]] = f2{g0 ? dn.x : r[minus[i]].x, g1 ? dn.y : r[minus[i]].y};
  }
}
// the cells of a pair whose guard failed: the scalar code (IEEE divides), per cell -- rare
__device__ __forceinline__ void relax_pair_guard_path(const f2 (&f)[kQ], bool b0, bool b1, float omega, f2 (&r)[kQ],
                                                      bool want_speed, float& sp0, float& sp1) {
#pragma unroll
  for (int c = 0; c < 2; c++) {
    if (!(c == 0 ? b0 : b1)) {
      float ts[kQ], rs[kQ], speed;
#pragma unroll
      for (int k = 0; k < kQ; k++) ts[k] = f[k][c];
      relax_cell<0, 1>(ts, false, false, omega, 0.f, 0.f, rs, speed, want_speed);
#pragma unroll
      for (int k = 0; k < kQ; k++) r[k][c] = rs[k];
      if (c == 0) sp0 = speed; else sp1 = speed;
    }
  }
}
__device__ __forceinline__ void relax_pair_fixup(const f2 (&f)[kQ], bool ok, unsigned blocked, bool lid, float omega,
                                                 float a1, float a2, f2 (&r)[kQ], bool want_speed, float& sp0, float& sp1) {
  if (!ok || lid || blocked != 0) {  // ONE branch on the way of a wave without exceptions
    const bool b0 = (blocked & 0xffu) != 0, b1 = (blocked & 0xff00u) != 0;
    if (!ok) relax_pair_guard_path(f, b0, b1, omega, r, want_speed, sp0, sp1);
    if (lid) accelerate_select(r, !b0, !b1, a1, a2);
    if (blocked != 0) bounce_select(f, b0, b1, r, sp0, sp1);
  }
}

// One PAIR of cells of one row: stream inputs f[k] -> relaxed r[k]; returns the sum of |u| over its fluid cells
// (SPEED = 1 form: pre-collision moments, native sqrt) when want_speed.
// blocked: the pair's two mask bytes (bits 0-7, 8-15); lid: this row receives the next step's acceleration.
__device__ __forceinline__ float relax_pair_exact(const f2 (&f)[kQ], unsigned blocked, bool lid, float omega,
                                                  float a1, float a2, f2 (&r)[kQ], bool want_speed) {
  f2 u_sq;
  const bool ok = relax_pair_core(f, omega, r, u_sq);
  float sp0 = 0.f, sp1 = 0.f;
  if (want_speed) {
    sp0 = __builtin_amdgcn_sqrtf(u_sq.x);
    sp1 = __builtin_amdgcn_sqrtf(u_sq.y);
  }
  relax_pair_fixup(f, ok, blocked, lid, omega, a1, a2, r, want_speed, sp0, sp1);
  return sp0 + sp1;
}

// Both pairs of a lane in one basic block: two independent dependency chains the scheduler can interleave (with two
// waves per SIMD there is little else to fill the issue slots of a dependent chain); exceptions after both.
__device__ __forceinline__ float relax_quad_exact(const f2 (&f0)[kQ], const f2 (&f1)[kQ], unsigned blocked, bool lid,
                                                  float omega, float a1, float a2, f2 (&r0)[kQ], f2 (&r1)[kQ],
                                                  bool want_speed) {
  f2 usq0, usq1;
  const bool ok0 = relax_pair_core(f0, omega, r0, usq0);
  const bool ok1 = relax_pair_core(f1, omega, r1, usq1);
  float sp[4] = {0.f, 0.f, 0.f, 0.f};
  if (want_speed) {
    sp[0] = __builtin_amdgcn_sqrtf(usq0.x);  sp[1] = __builtin_amdgcn_sqrtf(usq0.y);
    sp[2] = __builtin_amdgcn_sqrtf(usq1.x);  sp[3] = __builtin_amdgcn_sqrtf(usq1.y);
  }
  relax_pair_fixup(f0, ok0, blocked & 0xffffu, lid, omega, a1, a2, r0, want_speed, sp[0], sp[1]);
  relax_pair_fixup(f1, ok1, blocked >> 16, lid, omega, a1, a2, r1, want_speed, sp[2], sp[3]);
  return (sp[0] + sp[1]) + (sp[2] + sp[3]);
}

// pair P of a plane (NP pairs per lane) shifted by one cell: the value each cell receives from its west (east)
// neighbour; W = the west lane's last cell, E = the east lane's first cell
template <int NP, int P>
__device__ __forceinline__ f2 pair_from_west(const f2 (&a)[NP], float W) {
  if constexpr (P == 0) return f2{W, a[0].x};
  else return f2{a[P - 1].y, a[P].x};
}
template <int NP, int P>
__device__ __forceinline__ f2 pair_from_east(const f2 (&a)[NP], float E) {
  if constexpr (P == NP - 1) return f2{a[P].y, E};
  else return f2{a[P].y, a[P + 1].x};
}

template <int NP>
struct WindowPk {
  f2 w256[3][NP];  // speeds 2,5,6 of the row two below the newest, as pairs
  f2 w013[3][NP];  // speeds 0,1,3 of the row below the newest
  f2 n256[3][NP];  // speeds 2,5,6 of the row below the newest
  unsigned m;
};

// stepk_stream with the collision on pairs (exact arithmetic, 4 cells per lane); same launch geometry and arguments.
// LW of the K-1 sliding windows (the last ones) live in LDS instead of registers: a window is 36 floats per lane,
// K = 4 needs three of them, and with all three in registers (252 VGPRs) nothing is left to prefetch the next row
// into -- at two waves per SIMD the kernel then waits out every row's load latency (8192^2: 0.284 ms per step,
// neither VALU- nor DRAM-bound).  An LDS window is nine 16-byte quads per lane (lane-linear: conflict-free
// ds_read_b128 / ds_write_b128), private to the lane that wrote it, so no barrier is involved; speeds 2,5,6 sit in
// a two-deep ring indexed by the row parity, speeds 0,1,3 in a single slot.  9 KB per window and wave.
// NP = pairs per lane: 2 (four cells, 16-byte accesses, K <= 4) or 1 (two cells, 8-byte accesses, K <= 2: a halo lane's
// two cells cover two steps) -- the form for grids too small to fill the chip with four-cell lanes.
template <bool NTS, int K, bool PREFETCH, int LW, bool QUAD = false, int NP = 2>
__global__ __launch_bounds__(64, NP == 1 ? (K > 2 ? 3 : (PREFETCH ? 2 : 4)) : 2) void stepk_pk(const StepKArgs a) {
  static_assert(K >= 2 && K <= 4 && LW >= 0 && LW <= K - 1 && (NP == 2 || !QUAD), "halo_lanes * C >= K is the host's job");
  constexpr int C = 2 * NP;
  typedef typename RowPull<C>::vec vec;
  __shared__ vec lds_win[LW > 0 ? LW : 1][9][64];
  const int lane = threadIdx.x;
  int strip, band;
  if (a.chunk > 0) {
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int chunks_per_band = (a.n_strips + a.chunk - 1) / a.chunk;
    const int g = (j / a.chunk) * 8 + xcd;
    band = g / chunks_per_band;
    strip = (g - band * chunks_per_band) * a.chunk + j % a.chunk;
    if (band >= a.n_bands || strip >= a.n_strips) return;
  } else {
    strip = blockIdx.x % a.n_strips;
    band = blockIdx.x / a.n_strips;
  }
  const int wave_id = band * a.n_strips + strip;
  const int units_x = a.nx / C;
  const int y0 = a.row_first + band * a.band_pitch;
  const int band_n = min(a.band_rows, a.row_end - y0);

  const int H = a.halo_lanes;  // H * C >= K cells of halo per side
  const int ux_raw = strip * (64 - 2 * H) + lane - H;
  int ux = ux_raw % units_x;
  if (ux < 0) ux += units_x;
  const int x0 = ux * C;
  const bool out_lane = (lane >= H) && (lane < 64 - H) && (ux_raw < units_x);
  const long ps = a.plane_stride;

  Step2Args pa;
  pa.src = a.src;  pa.mask = a.mask;  pa.plane_stride = a.plane_stride;  pa.row_pitch = a.row_pitch;
  pa.pitch = a.pitch;  pa.rows = a.rows;  pa.wrap = a.wrap;

  WindowPk<NP> win[K - 1];  // the first K-1-LW are used (registers); the others only for their mask bytes
#pragma unroll
  for (int s = 0; s < K - 1; s++) {
    win[s].m = 0;
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
      for (int p = 0; p < NP; p++) win[s].w256[q][p] = win[s].w013[q][p] = win[s].n256[q][p] = splat2(0.f);
  }
  if constexpr (LW > 0) {
#pragma unroll
    for (int l = 0; l < LW; l++)
#pragma unroll
      for (int q = 0; q < 9; q++) {
        vec z;
#pragma unroll
        for (int j = 0; j < C; j++) z[j] = 0.f;
        lds_win[l][q][lane] = z;
      }
  }
  float sum[K];
#pragma unroll
  for (int s = 0; s < K; s++) sum[s] = 0.f;

  // the NP pairs of one plane of a loaded / LDS vector, and back
  auto pairs_of = [](const vec& v, f2 (&o)[NP]) {
#pragma unroll
    for (int p = 0; p < NP; p++) o[p] = f2{v[2 * p], v[2 * p + 1]};
  };
  auto vec_of = [](const f2 (&c)[NP][kQ], int k) {
    vec o;
#pragma unroll
    for (int p = 0; p < NP; p++) { o[2 * p] = c[p][k].x;  o[2 * p + 1] = c[p][k].y; }
    return o;
  };
  // relax the NP pairs of one row: inputs by plane (already shifted), pair-major outputs
  auto relax_row = [&](const f2 (&in)[kQ][NP], unsigned m, bool lid, f2 (&out)[NP][kQ], bool own_row) {
    f2 t0[kQ];
#pragma unroll
    for (int k = 0; k < kQ; k++) t0[k] = in[k][0];
    if constexpr (NP == 1) {
      return relax_pair_exact(t0, m & 0xffffu, lid, a.omega, a.a1, a.a2, out[0], own_row);
    } else {
      f2 t1[kQ];
#pragma unroll
      for (int k = 0; k < kQ; k++) t1[k] = in[k][NP - 1];
      if constexpr (QUAD) {
        return relax_quad_exact(t0, t1, m, lid, a.omega, a.a1, a.a2, out[0], out[NP - 1], own_row);
      } else {
        const float s0 = relax_pair_exact(t0, m & 0xffffu, lid, a.omega, a.a1, a.a2, out[0], own_row);
        return s0 + relax_pair_exact(t1, m >> 16, lid, a.omega, a.a1, a.a2, out[NP - 1], own_row);
      }
    }
  };
  // the nine planes a cell pulls from: planes 0,2,4 as they are, 1,5,8 from the west, 3,6,7 from the east
  auto shifted = [](const f2 (&pl)[kQ][NP], const float (&W)[kQ], const float (&E)[kQ], f2 (&in)[kQ][NP]) {
#pragma unroll
    for (int k = 0; k < kQ; k++) {
      const bool west = (k == 1 || k == 5 || k == 8), east = (k == 3 || k == 6 || k == 7);
      if (west) {
        in[k][0] = pair_from_west<NP, 0>(pl[k], W[k]);
        if constexpr (NP == 2) in[k][NP - 1] = pair_from_west<NP, NP - 1>(pl[k], W[k]);
      } else if (east) {
        in[k][0] = pair_from_east<NP, 0>(pl[k], E[k]);
        if constexpr (NP == 2) in[k][NP - 1] = pair_from_east<NP, NP - 1>(pl[k], E[k]);
      } else {
#pragma unroll
        for (int p = 0; p < NP; p++) in[k][p] = pl[k][p];
      }
    }
  };

  const int n_iter = band_n + 2 * (K - 1);
  // Row bookkeeping kept incrementally (all wave-uniform, i.e. scalar registers): the row stage 1 pulls advances by
  // one per iteration, and stage s+1 works on the row stage 1 had s iterations ago -- so "is this the lid row" and
  // "does this row belong to the band" are shift registers (bit s = stage s+1), and the row the last stage stores is
  // the oldest of a K-deep history, instead of a wrap, two compares and a window test per stage, pair and iteration.
  int r_next = wrap_row(y0 - (K - 1), a.rows, a.wrap);  // the row iteration i pulls
  int r_hist[K];                                        // r_hist[s] = the row stage s+1 works on
#pragma unroll
  for (int s = 0; s < K; s++) r_hist[s] = 0;
  unsigned lid_hist = 0, own_hist = 0;
  RowPull<C> nextp;
  if constexpr (PREFETCH) nextp = pull_row<C>(pa, r_next, x0);

  // One row iteration.  WARM: the first 2 (K-1) iterations of a band, while the later stages have nothing to work on
  // yet; the iterations after them run a copy of the body without those tests (every stage active: no merges of
  // "relaxed" and "skipped" register sets, whose copies were 5 % of the steady state's vector instructions).
  auto row_iteration = [&](auto warm_c, const int i) {
    constexpr bool WARM = decltype(warm_c)::value;
    // ---- stage 1: step t on row r, pulled from memory -------------------------------------------
    const int r = r_next;
    r_next = r + 1;
    if (a.wrap && r_next >= a.rows) r_next -= a.rows;
#pragma unroll
    for (int s = K - 1; s > 0; s--) r_hist[s] = r_hist[s - 1];
    r_hist[0] = r;
    lid_hist = (lid_hist << 1) | ((r == a.accel_row || r == a.accel_row2) ? 1u : 0u);
    own_hist = (own_hist << 1) | ((i >= K - 1 && i < band_n + K - 1) ? 1u : 0u);
    RowPull<C> p;
    if constexpr (PREFETCH) {
      p = nextp;
      if (i + 1 < n_iter) nextp = pull_row<C>(pa, r_next, x0);
    } else {
      p = pull_row<C>(pa, r, x0);
    }
    f2 cur[NP][kQ];
    {
      float W[kQ] = {}, E[kQ] = {};
      W[1] = lane_from_west<2>(p.v[1][C - 1]);  W[5] = lane_from_west<2>(p.v[5][C - 1]);  W[8] = lane_from_west<2>(p.v[8][C - 1]);
      E[3] = lane_from_east<2>(p.v[3][0]);      E[6] = lane_from_east<2>(p.v[6][0]);      E[7] = lane_from_east<2>(p.v[7][0]);
      f2 pl[kQ][NP], in[kQ][NP];
#pragma unroll
      for (int k = 0; k < kQ; k++) pairs_of(p.v[k], pl[k]);
      shifted(pl, W, E, in);
      const bool lid = (lid_hist & 1u) != 0;
      const bool own_row = (own_hist & 1u) != 0;
      const float sp = relax_row(in, p.m, lid, cur, own_row);
      if (own_row && out_lane) sum[0] += sp;
    }
    unsigned m_cur = p.m;

    // ---- stages 2..K: step t+s on row r-s from window s and the stage-s results of row r-s+1 ------
    bool alive = true;
    auto stage = [&](auto sc) {
      constexpr int s = decltype(sc)::value;
      constexpr bool in_lds = (s - 1) >= (K - 1 - LW);
      constexpr int li = in_lds ? (s - 1) - (K - 1 - LW) : 0;
      if (!alive) return;
      WindowPk<NP>& w = win[s - 1];
      const int ring = (i & 1) * 3;
      f2 nxt[NP][kQ];
      const bool active = WARM ? (i >= 2 * s) : true;
      if (active) {
        // planes of the window rows: 2,5,6 of row ro-1, 0,1,3 of row ro, and 4,7,8 of row ro+1 (= cur)
        f2 pl[kQ][NP];
        constexpr int q256[3] = {2, 5, 6}, q013[3] = {0, 1, 3};
        if constexpr (in_lds) {
#pragma unroll
          for (int q = 0; q < 3; q++) {
            pairs_of(lds_win[li][ring + q][lane], pl[q256[q]]);
            pairs_of(lds_win[li][6 + q][lane], pl[q013[q]]);
          }
        } else {
#pragma unroll
          for (int q = 0; q < 3; q++)
#pragma unroll
            for (int p2 = 0; p2 < NP; p2++) { pl[q256[q]][p2] = w.w256[q][p2];  pl[q013[q]][p2] = w.w013[q][p2]; }
        }
#pragma unroll
        for (int p2 = 0; p2 < NP; p2++) { pl[4][p2] = cur[p2][4];  pl[7][p2] = cur[p2][7];  pl[8][p2] = cur[p2][8]; }
        float W[kQ] = {}, E[kQ] = {};
        W[1] = lane_from_west<2>(pl[1][NP - 1].y);  W[5] = lane_from_west<2>(pl[5][NP - 1].y);  W[8] = lane_from_west<2>(pl[8][NP - 1].y);
        E[3] = lane_from_east<2>(pl[3][0].x);       E[6] = lane_from_east<2>(pl[6][0].x);       E[7] = lane_from_east<2>(pl[7][0].x);
        f2 in[kQ][NP];
        shifted(pl, W, E, in);
        const bool last = (s == K - 1);
        const bool lid = ((lid_hist >> s) & 1u) != 0 && (!last || a.accel_after);
        const bool own_row = ((own_hist >> s) & 1u) != 0;
        const float sp = relax_row(in, w.m, lid, nxt, own_row);
        if (own_row && out_lane) sum[s] += sp;
      }
      // rotate window s with the stage-s row just consumed
      const unsigned m_below = w.m;
      if constexpr (in_lds) {
        lds_win[li][ring + 0][lane] = vec_of(cur, 2);
        lds_win[li][ring + 1][lane] = vec_of(cur, 5);
        lds_win[li][ring + 2][lane] = vec_of(cur, 6);
        lds_win[li][6][lane] = vec_of(cur, 0);
        lds_win[li][7][lane] = vec_of(cur, 1);
        lds_win[li][8][lane] = vec_of(cur, 3);
      } else {
#pragma unroll
        for (int p2 = 0; p2 < NP; p2++) {
          w.w256[0][p2] = w.n256[0][p2];  w.w256[1][p2] = w.n256[1][p2];  w.w256[2][p2] = w.n256[2][p2];
          w.n256[0][p2] = cur[p2][2];     w.n256[1][p2] = cur[p2][5];     w.n256[2][p2] = cur[p2][6];
          w.w013[0][p2] = cur[p2][0];     w.w013[1][p2] = cur[p2][1];     w.w013[2][p2] = cur[p2][3];
        }
      }
      w.m = m_cur;
      if (!active) { alive = false; return; }
      m_cur = m_below;
#pragma unroll
      for (int p2 = 0; p2 < NP; p2++)
#pragma unroll
        for (int k = 0; k < kQ; k++) cur[p2][k] = nxt[p2][k];
      if (s == K - 1 && out_lane) {
        const int ro = r_hist[K - 1];
        float* d_row = a.dst + (long)ro * a.row_pitch + x0;
#pragma unroll
        for (int k = 0; k < kQ; k++) {
          const vec o = vec_of(cur, k);
          if constexpr (NTS) __builtin_nontemporal_store(o, reinterpret_cast<vec*>(d_row + k * ps));
          else *reinterpret_cast<vec*>(d_row + k * ps) = o;
        }
      }
    };
    stage(std::integral_constant<int, 1>{});
    if constexpr (K > 2) stage(std::integral_constant<int, 2>{});
    if constexpr (K > 3) stage(std::integral_constant<int, 3>{});
  };
  const int n_warm = min(n_iter, 2 * (K - 1));
  int i = 0;
  for (; i < n_warm; i++) row_iteration(std::true_type{}, i);
  for (; i < n_iter; i++) row_iteration(std::false_type{}, i);

#pragma unroll
  for (int s = 0; s < K; s++) {
    const float tot = wave_sum(sum[s]);
    if (lane == 0) a.partials[(long)s * a.slot_stride + wave_id] = tot;
  }
}

// ---------------------------------------------------------------------------------------------
// Up to KMAX timesteps per launch from an LDS tile (temporal blocking for small, cache-resident grids,
// single periodic slab).
//
// A grid of a few hundred thousand cells is not bound by bandwidth or arithmetic but by the latency of
// one kernel (~3 us): every launch pays it, so the only lever is more timesteps per launch.  A workgroup
// stages its TW x TH tile plus a halo of KMAX cells on every side -- all 9 populations and the obstacle
// flags -- in LDS, and relaxes it n <= KMAX times in place: step j covers the cells at distance >= j from
// the staged border (their 9 sources are cells of step j-1 inside the region), each thread pulls its
// cells' populations from LDS into registers, the workgroup synchronises, the results go back to LDS.
// After n steps the tile's own cells are exact and are stored; the halo cells were relaxed redundantly,
// exactly as the neighbouring workgroups relax them (same per-cell code as every other kernel, so the
// lattice stays bit-identical).  Periodic wrap in x and y is resolved when the tile is staged.
// Sum of |u| per step: over the tile's own cells, one partial per workgroup and step.
// ---------------------------------------------------------------------------------------------
struct TileArgs : LatticeArgs {
  int ny;
  int tiles_x;      // workgroups across x
  int n_steps;      // timesteps this launch advances (1..KMAX)
  int accel_row;    // global row that receives accelerate_flow (ny - 2)
  int accel_after;  // also apply the acceleration of the step after this launch's last one
  float omega, a1, a2;
  float* partials;  // partials[j * slot_stride + workgroup] = sum |u| of the tile's own cells after step j
  long slot_stride;
};

template <int MATH, int TW, int TH, int KMAX, int THREADS = kBlock>
__global__ __launch_bounds__(THREADS) void step_tile(const TileArgs a) {
  constexpr int EW = TW + 2 * KMAX, EH = TH + 2 * KMAX, EC = EW * EH;
  constexpr int EWP = EW + 1;                                           // row padding against bank conflicts
  constexpr int MAXC = ((EW - 2) * (EH - 2) + THREADS - 1) / THREADS;   // cells per thread in step 1
  __shared__ float f[kQ][EH][EWP];
  __shared__ unsigned char blocked[EH][EW];
  __shared__ int global_row[EH];

  const int tid = threadIdx.x;
  const int bx = blockIdx.x % a.tiles_x, by = blockIdx.x / a.tiles_x;
  const int gx0 = bx * TW - KMAX, gy0 = by * TH - KMAX;
  const long ps = a.plane_stride;

  // stage the tile and its halo (periodic images where the halo leaves the grid)
  for (int idx = tid; idx < EC; idx += THREADS) {
    const int y = idx / EW, x = idx - y * EW;
    int gy = (gy0 + y) % a.ny;  if (gy < 0) gy += a.ny;
    int gx = (gx0 + x) % a.nx;  if (gx < 0) gx += a.nx;
    const float* cell = a.src + (long)gy * a.row_pitch + gx;
#pragma unroll
    for (int k = 0; k < kQ; k++) f[k][y][x] = cell[k * ps];
    blocked[y][x] = a.mask[(long)gy * a.pitch + gx];
    if (x == 0) global_row[y] = gy;
  }
  __syncthreads();

  for (int j = 1; j <= a.n_steps; j++) {
    const int w = EW - 2 * j, n = w * (EH - 2 * j);
    const bool accel = (j < a.n_steps) || a.accel_after;
    float r[MAXC][kQ];
    float my_sum = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
      const int idx = tid + c * THREADS;
      if (idx < n) {
        const int ry = idx / w;
        const int y = j + ry, x = j + (idx - ry * w);
        // pull (SerialCode/d2q9-bgk.c:263-271): speed k arrives from the cell it left one step ago
        const float t[kQ] = {f[0][y][x],         f[1][y][x - 1],     f[2][y - 1][x],
                             f[3][y][x + 1],     f[4][y + 1][x],     f[5][y - 1][x - 1],
                             f[6][y - 1][x + 1], f[7][y + 1][x + 1], f[8][y + 1][x - 1]};
        const int oy = y - KMAX, ox = x - KMAX;  // position inside the tile's own cells
        const bool own = (oy >= 0) && (oy < TH) && (ox >= 0) && (ox < TW) && (by * TH + oy < a.ny) &&
                         (bx * TW + ox < a.nx);
        const bool lid = accel && (global_row[y] == a.accel_row);
        float speed;
        relax_cell<MATH>(t, blocked[y][x] != 0, lid, a.omega, a.a1, a.a2, r[c], speed, own);
        if (own) my_sum += speed;
      }
    }
    __syncthreads();  // every source of this step has been read
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
      const int idx = tid + c * THREADS;
      if (idx < n) {
        const int ry = idx / w;
        const int y = j + ry, x = j + (idx - ry * w);
#pragma unroll
        for (int k = 0; k < kQ; k++) f[k][y][x] = r[c][k];
      }
    }
    const float total = block_sum<THREADS>(my_sum);  // synchronises the workgroup
    if (tid == 0) a.partials[(long)(j - 1) * a.slot_stride + blockIdx.x] = total;
    __syncthreads();
  }

  // the tile's own cells
  for (int idx = tid; idx < TW * TH; idx += THREADS) {
    const int oy = idx / TW, ox = idx - oy * TW;
    const int gy = by * TH + oy, gx = bx * TW + ox;
    if (gy < a.ny && gx < a.nx) {
      float* cell = a.dst + (long)gy * a.row_pitch + gx;
#pragma unroll
      for (int k = 0; k < kQ; k++) cell[k * ps] = f[k][oy + KMAX][ox + KMAX];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Resident lattice: ONE launch advances the whole (single, periodic) slab by many timesteps with the lattice kept
// in registers -- the form for cache-resident grids (the reference's own data sets, 128^2 ... 1024^2 x 20 000 - 80 000
// steps, dataSet/input_*.params; loop SerialCode/d2q9-bgk.c:166-170), where a launch per pass costs a kernel
// boundary (~1.5-3 us) plus a reload of the lattice through L2 however little it computes.
//
// Geometry: workgroup b owns the band of rows [4b, 4b+4), the full width; thread x owns column x of the band: four
// cells, kept as two PAIRS for the packed arithmetic -- the interior pair (rows 1, 2) and the edge pair (rows 0, 3).
// 36 VGPRs of state per lane; a 1024 x 1024 lattice is 256 workgroups of 1024 threads, one per CU.  (ROWS = 2: bands
// of two rows, one pair per lane, where the chip has CUs to spare.)
//   streaming in y inside the band : register renaming (free)
//   streaming in x                 : DPP wave_shr / wave_shl; lane 0 / 63 of a wave take the neighbouring wave's edge
//                                    lane from LDS (one s_barrier per timestep, two LDS slots by parity)
//   rows 0 and 3 also need the adjacent row of the neighbouring BAND: the 3 populations that cross the seam travel
//   through L2 as one 16-byte granule per cell and direction, {v, v, v, tag} -- ONE sc1 (write-through, L1-bypassing)
//   dwordx4 store, naturally aligned, so it lies inside one 64-byte memory request on the way out and on the way in;
//   the tag is the global timestep index + 1, i.e. the data is its own flag: no fence, no separate flag, no
//   device-wide barrier.  (8-byte {value, tag} granules, the form MI355X_MICROARCH.md prices, cost three narrow sc1
//   stores per cell and direction: 12.6 MB per step at 1024^2, store-bound at 5.9 us per step.)
//   Two slots by step parity: a slot is overwritten two steps later, by which time the neighbour has provably read
//   it (it cannot have published the step in between otherwise).  A lane loads the granule of its own column; the
//   diagonal populations shift by DPP, the wave's first / last lane taking the column beyond from a second load.
// Per timestep: publish the edge rows (computed last in the previous step) -> LDS edge lanes -> barrier -> relax the
// interior pair (hides the hop) -> poll the six halo granules -> relax the edge pair.  No redundant work at all.
// Every spin is bounded (wall clock): on expiry the workgroup raises *status and leaves; every other workgroup
// sees the status in its own spin and leaves too.  An error, never a hang.  The grid must be co-resident (host:
// one workgroup per CU at most as many as the device has CUs).
// Arithmetic: relax_pair_core + the per-cell exception path, i.e. the lattice stays bit-identical to the oracle;
// |u| from the pre-collision moments as in the stream kernels.
// ---------------------------------------------------------------------------------------------
// one lattice of a batch (lbm_create_batch): what a batched launch takes per member instead of ResidentArgs' fields
struct ResidentMember {
  float* src;                 // current lattice (the first step's accelerate_flow is applied to it in place)
  float* dst;
  const unsigned char* mask;
  uint4* gran;                // the member's own seam granules and tags
  float* partials;
  double* tot_u;              // the member's per-step sums of |u|
  float omega, a1, a2;
};
struct ResidentArgs : LatticeArgs {  // src: the lattice to start from, dst: where to leave the result (may equal src)
  int ny;
  int n_steps;                // timesteps this launch advances
  int accel_row;              // global row of accelerate_flow (ny - 2)
  int accel_last;             // also apply the acceleration of the step after this launch's last one
  float omega, a1, a2;
  uint4* gran;                // seam granules {v, v, v, tag}: [2 directions][bands][2 slots][nx]
  unsigned gran_bytes;        // size of the granule buffer
  unsigned epoch0;            // tag of this launch's step s = epoch0 + s + 1 (global step index + 1: never repeats)
  float* partials;            // partials[s * bands + b] = sum |u| over band b after step s
  int* status;                // 0, or kResidentTimeout once any workgroup gave up waiting
  long long timeout_ticks;    // bound of one halo wait in wall_clock64() ticks (100 MHz)
  int xcd_affinity;           // 1: seams inside one XCD use L2-resident stores (see resident_band); 0: sc1 everywhere
  int absent_band;            // tests: this band's workgroup returns at once, as if it had never been scheduled (-1: none)
  int group;                  // bands per workgroup (blockDim.x = group * nx)
  int one_xcd;                // 1: the launch has 8 workgroups per working one and only those dealt to the first XCD work
#ifdef LBM_RESIDENT_PROFILE
  long long* prof;            // tools/resident_profile.sh: [band][8] shader-clock sums of the phases of a step
#endif
};
// the layouts the kernels were compiled and measured with: an edit that shifts a field fails here, not in a profile
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(offsetof(StepArgs, rows) == 48 && offsetof(StepArgs, partials) == 80, "StepArgs layout");
static_assert(offsetof(Step2Args, rows) == 48 && offsetof(Step2Args, partials1) == 96, "Step2Args layout");
static_assert(offsetof(StepKArgs, rows) == 48 && offsetof(StepKArgs, partials) == 112, "StepKArgs layout");
static_assert(offsetof(TileArgs, ny) == 48 && offsetof(TileArgs, partials) == 80, "TileArgs layout");
static_assert(offsetof(ResidentArgs, ny) == 48 && offsetof(ResidentArgs, gran) == 80, "ResidentArgs layout");
#pragma clang diagnostic pop
// batched launches (resident_band<..., BATCH = true>): src, dst, mask, omega, a1, a2, gran and partials above are unused,
// each member brings its own; status is shared by all members of all launches of a batch
struct ResidentBatchArgs : ResidentArgs {
  const ResidentMember* members;  // this launch's members
  int n_members;
  int member_wgs;             // working workgroups of one member; without one_xcd member m starts at block
                              // m * round_up(member_wgs, 8), so the XCD-affinity band order holds inside every member
};
// animation frames (lbm_set_frames, resident_band<..., REC = kRecFrames>): after global step tt with tt % every == 0 the
// kernel stores |u| of every owned cell into slot (tt / every - ord0) % slots of base, one float[rows][nx] per slot.
// Kept out of ResidentArgs / ResidentMember so that the other forms read their arguments at the same offsets.
struct ResidentFrames {
  float* base;                // slot 0; nullptr / every = 0: no frames
  int every;
  int ord0;                   // tt / every of the first frame after arming
  int slots;
};
struct ResidentFramesArgs : ResidentArgs {
  ResidentFrames fr;
};
struct ResidentBatchFramesArgs : ResidentBatchArgs {
  const ResidentFrames* frames;  // [this launch's members], as members
};
// point probes (lbm_set_probes, resident_band<..., REC = kRecProbes>): after global step tt with tt % every == 0 the kernel
// stores {u_x, u_y, |u|, pressure} of every probed cell into row (tt / every - ord0) % slots of ring, one 16-byte sample
// per probe, in the caller's probe order.  The host sorts the probes by row: `table` holds them in that order, followed by
// one word per band of the resident kernel -- first entry | entries << 12 | (a probe lies on the lid row) << 31 -- so a
// band without probes learns so from one word.  Appended like ResidentFrames: the other forms' arguments do not move.
struct ProbeEntry {
  int row;                    // slab row of the cell
  unsigned xi;                // column | probe index << 20
};
typedef float probe_vec __attribute__((ext_vector_type(4)));
struct ResidentProbes {
  probe_vec* ring;            // row 0; nullptr / every = 0: no probes
  const ProbeEntry* table;
  int every;
  int ord0;                   // tt / every of the first sample row after arming
  int slots;
  int n_probes;
  float density;              // a blocked cell reports density * c_sq as its pressure
  int pad;
};
struct ResidentProbesArgs : ResidentArgs {
  ResidentProbes pr;
};
struct ResidentBatchProbesArgs : ResidentBatchArgs {
  const ResidentProbes* probes;  // [this launch's members], as members
};
// mean fields (lbm_set_mean, resident_band<..., REC = kRecMean>): after global step tt with tt % every == 0 the kernel adds
// {u_x, u_y, |u|, pressure} of every owned cell, each widened to double, to the cell's four sums: planes
// double[rows][nx] at base + j * plane_stride, j = 0..3 in that order.  The record is an accumulation, not a slot: there
// is no ordinal and no capacity, and a launch continues from whatever the planes hold.  Appended like ResidentFrames.
// order == 2 (lbm_set_mean_order): planes 4..7 follow in the same allocation, the sums of the products u_x u_x, u_y u_y,
// u_x u_y and pressure pressure of the same samples, acc = acc + (double)a * (double)b: the product of two floats is exact
// in a double, so the update rounds once, contracted into an FMA or not.
struct ResidentMean {
  double* base;               // plane 0, row 0; nullptr / every = 0: no mean
  long plane_stride;          // doubles between the planes (rows * nx)
  int every;
  float density;              // a blocked cell adds density * c_sq to its pressure sum
  int order;                  // 1: planes 0..3; 2: planes 0..7
  int pad;
};
struct ResidentMeanArgs : ResidentArgs {
  ResidentMean mn;
};
struct ResidentBatchMeanArgs : ResidentBatchArgs {
  const ResidentMean* means;  // [this launch's members], as members
};
// field frames (lbm_set_field_frames, resident_band<..., REC = kRecFields>): after global step tt with tt % every == 0 the
// kernel stores the selected ones of {u_x, u_y, |u|, pressure} (bits 0..3 of `fields`, planes in ascending bit order) of
// every cell of the window into slot (tt / every - ord0) % slots of base, one float[F][wny][wnx] per slot.  The window is
// slab-local: columns [wx0, wx0 + wnx), slab rows [wy0, wy0 + wny) -- the slab's own rows of the caller's window, so the
// ring of a slab holds nothing else.  Appended like ResidentFrames: the other forms' arguments do not move.
struct ResidentFields {
  float* base;                // slot 0; nullptr / every = 0: no field frames
  int every;
  int ord0;                   // tt / every of the first frame after arming
  int slots;
  int fields;                 // LBM_FIELD_* bits
  int wx0, wy0, wnx, wny;
  float density;              // a blocked cell reports density * c_sq as its pressure
  int pad;
};
struct ResidentFieldsArgs : ResidentArgs {
  ResidentFields fd;
};
struct ResidentBatchFieldsArgs : ResidentBatchArgs {
  const ResidentFields* fields;  // [this launch's members], as members
};
#ifdef LBM_RESIDENT_PROFILE
__device__ __forceinline__ long long prof_clock() {
  long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define RESIDENT_PROF(i) do { const long long now_ = prof_clock(); prof_acc[i] += now_ - prof_t; prof_t = now_; } while (0)
#else
#define RESIDENT_PROF(i) do { } while (0)
#endif
constexpr int kResidentTimeout = 1;

// per-cell lid flags (bit 0: cell .x, bit 1: cell .y): the pair's two cells lie in different rows here
__device__ __forceinline__ void relax_pair_fixup_rows(const f2 (&f)[kQ], bool ok, unsigned blocked, unsigned lid, float omega,
                                                      float a1, float a2, f2 (&r)[kQ], float& sp0, float& sp1) {
  if (!ok || lid != 0 || blocked != 0) {
    const bool b0 = (blocked & 0xffu) != 0, b1 = (blocked & 0xff00u) != 0;
    if (!ok) relax_pair_guard_path(f, b0, b1, omega, r, true, sp0, sp1);
    if (lid != 0) accelerate_select(r, (lid & 1u) != 0 && !b0, (lid & 2u) != 0 && !b1, a1, a2);
    if (blocked != 0) bounce_select(f, b0, b1, r, sp0, sp1);
  }
}
__device__ __forceinline__ float relax_pair_rows(const f2 (&f)[kQ], unsigned blocked, unsigned lid, float omega, float a1,
                                                 float a2, f2 (&r)[kQ]) {
  f2 u_sq;
  const bool ok = relax_pair_core(f, omega, r, u_sq);
  float sp0 = __builtin_amdgcn_sqrtf(u_sq.x), sp1 = __builtin_amdgcn_sqrtf(u_sq.y);
  relax_pair_fixup_rows(f, ok, blocked, lid, omega, a1, a2, r, sp0, sp1);
  return sp0 + sp1;
}

// |u| of cell c of a relaxed pair as lbm_read_final_state reports it (final_state: moments_exact, IEEE sqrt), 0 if blocked
__device__ __forceinline__ float frame_speed(const f2 (&r)[kQ], int c, bool blocked) {
  float f[kQ];
#pragma unroll
  for (int k = 0; k < kQ; k++) f[k] = r[k][c];
  float rho, ux, uy;
  moments_exact(f, rho, ux, uy);
  return blocked ? 0.f : sqrtf((ux * ux) + (uy * uy));
}

// the sample of one cell as lbm_read_final_state reports it (final_state: moments_exact, IEEE sqrt, the blocked constants)
__device__ __forceinline__ probe_vec probe_sample(const float (&f)[kQ], bool blocked, float density) {
  float rho, ux, uy;
  moments_exact(f, rho, ux, uy);
  const probe_vec fluid = {ux, uy, sqrtf((ux * ux) + (uy * uy)), rho * kCsq};
  const probe_vec solid = {0.f, 0.f, 0.f, density * kCsq};
  return blocked ? solid : fluid;
}

// sum over the first 16 lanes (one DPP row), valid in every lane of that row
__device__ __forceinline__ float row16_sum_dpp(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xb1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4e, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));  // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true));  // row_mirror
  return v;
}

// both pairs of a lane in one basic block (two independent dependency chains), the exceptions after both
__device__ __forceinline__ float relax_two_pairs_rows(const f2 (&fa)[kQ], const f2 (&fb)[kQ], unsigned blocked_a, unsigned blocked_b,
                                                      unsigned lid_a, unsigned lid_b, float omega, float a1, float a2,
                                                      f2 (&ra)[kQ], f2 (&rb)[kQ]) {
  f2 usq_a, usq_b;
  const bool ok_a = relax_pair_core(fa, omega, ra, usq_a);
  const bool ok_b = relax_pair_core(fb, omega, rb, usq_b);
  float sp[4] = {__builtin_amdgcn_sqrtf(usq_a.x), __builtin_amdgcn_sqrtf(usq_a.y), __builtin_amdgcn_sqrtf(usq_b.x), __builtin_amdgcn_sqrtf(usq_b.y)};
  relax_pair_fixup_rows(fa, ok_a, blocked_a, lid_a, omega, a1, a2, ra, sp[0], sp[1]);
  relax_pair_fixup_rows(fb, ok_b, blocked_b, lid_b, omega, a1, a2, rb, sp[2], sp[3]);
  return (sp[0] + sp[1]) + (sp[2] + sp[3]);
}

// lane i <- lane i-1 (i+1); the wave's first (last) lane, which has no such lane, keeps `edge`
__device__ __forceinline__ float shift_from_west(float v, float edge) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float shift_from_east(float v, float edge) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}

// sum over the wave by DPP (no LDS); valid in lane 63
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xb1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4e, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));  // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true));  // row_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, false));  // row_bcast:15 into rows 1 and 3
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xc, 0xf, false));  // row_bcast:31 into rows 2 and 3
  return v;
}

// 16-byte seam granule: three populations and the tag in ONE naturally aligned dwordx4 access with sc1 (agent scope:
// the store writes through the XCD's L2, the load bypasses L1 and refetches), i.e. the raw-buffer forms with aux = sc1
typedef int granule_vec __attribute__((ext_vector_type(4)));
typedef int mean_word __attribute__((ext_vector_type(2)));  // one double sum as the 8-byte buffer access moves it
__device__ __forceinline__ __amdgpu_buffer_rsrc_t granule_rsrc(uint4* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ void granule_store(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off, float a, float b, float c, unsigned tag) {
  const granule_vec v = {(int)__float_as_uint(a), (int)__float_as_uint(b), (int)__float_as_uint(c), (int)tag};
  __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (int)byte_off, 0, 16);  // aux 16 = sc1
}
// the same store without sc1: the line stays (dirty) in this XCD's L2, where a reader on the SAME XCD finds it with
// its sc1 (L1-bypassing) load at L2 latency instead of a round trip over the fabric
__device__ __forceinline__ void granule_store_local(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off, float a, float b, float c, unsigned tag) {
  const granule_vec v = {(int)__float_as_uint(a), (int)__float_as_uint(b), (int)__float_as_uint(c), (int)tag};
  __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (int)byte_off, 0, 0);
}
__device__ __forceinline__ granule_vec granule_load(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off) {
  return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)byte_off, 0, 16);
}

// field frames (resident_band<..., REC = kRecFields>): the selected values of a band's post-step cells inside the window --
// edge pair `pe` (band rows 0 and ROWS - 1), interior pair `ri` (rows 1 and 2 of four) -- into the slot, then the deferred
// accelerate_flow of the next step on `lidp`, the pair that holds the lid row (see take_frame), and the frames' count of
// f_next and f_slot.  band_row0 is the slab row of the band's row 0, x the lane's column.
template <int ROWS>
__device__ __forceinline__ void take_fields(const ResidentFields& fd, int band_row0, int x, const f2 (&pe)[kQ], const f2 (&ri)[kQ],
                                            f2 (&lidp)[kQ], unsigned blocked_e, unsigned blocked_i, unsigned lid, bool accel_next,
                                            float a1, float a2, unsigned& f_next, int& f_slot) {
  constexpr int TOP = ROWS - 1;
  // the band's rows against the window's: wave-uniform (a band without rows of the window stores nothing)
  const int row0 = __builtin_amdgcn_readfirstlane(band_row0) - fd.wy0;  // window row of band row 0
  if (row0 + ROWS > 0 && row0 < fd.wny) {
    // the slot as a buffer (scalar base, 32-bit lane offset): no 64-bit address stays live in VGPRs
    const unsigned row_bytes = (unsigned)fd.wnx * 4u, plane_bytes = row_bytes * (unsigned)fd.wny;
    const int planes = __builtin_popcount((unsigned)fd.fields);
    const __amdgpu_buffer_rsrc_t srsrc = __builtin_amdgcn_make_buffer_rsrc(fd.base + (long)f_slot * planes * fd.wny * fd.wnx, 0,
                                                                           (int)((unsigned)planes * plane_bytes), 0x00020000);
    const int col = x - fd.wx0;
    const int lane_off = col * 4;
    auto store_cell = [&](const f2 (&p)[kQ], int c, bool blocked, int rb) {
      const int wrow = row0 + rb;
      if (wrow < 0 || wrow >= fd.wny) return;  // wave-uniform
      float f[kQ];
#pragma unroll
      for (int k = 0; k < kQ; k++) f[k] = p[k][c];
      const probe_vec v = probe_sample(f, blocked, fd.density);
      unsigned soff = (unsigned)wrow * row_bytes;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (((unsigned)fd.fields >> j) & 1u) {  // wave-uniform
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[j]), srsrc, lane_off, (int)soff, 2);  // aux 2 = nt
          soff += plane_bytes;
        }
      }
    };
    if (col >= 0 && col < fd.wnx) {
      store_cell(pe, 0, (blocked_e & 0xffu) != 0, 0);
      store_cell(pe, 1, (blocked_e & 0xff00u) != 0, TOP);
      if constexpr (ROWS == 4) {
        store_cell(ri, 0, (blocked_i & 0xffu) != 0, 1);
        store_cell(ri, 1, (blocked_i & 0xff00u) != 0, 2);
      }
    }
  }
  const unsigned blk = (ROWS == 4) ? blocked_i : blocked_e;
  if (accel_next && lid != 0)
    accelerate_select(lidp, (lid & 1u) != 0 && (blk & 0xffu) == 0, (lid & 2u) != 0 && (blk & 0xff00u) == 0, a1, a2);
  f_next += (unsigned)fd.every;
  f_slot = (f_slot + 1 == fd.slots) ? 0 : f_slot + 1;
}

// JOINT: wait for the halo first and relax both pairs as ONE block of independent work -- for narrow grids, whose few
// waves sit alone on their SIMDs: there the step is the dependent-instruction latency of the two collisions one after
// the other, and two independent chains interleave (issue-bound instead of latency-bound).  Wide grids (four waves
// per SIMD) keep the interior pair in front of the halo wait: their SIMDs are busy anyway and the interior pair
// hides the hop.
// ROWS: rows per band, 4 (above) or 2 -- one pair per lane, both rows seam rows: twice the workgroups and half the
// dependent work per lane and step, for grids small enough that the chip has CUs to spare (ny / 2 <= CUs): there the
// step is one wave's chain "hop + collisions", and the shorter chain wins although nothing hides the hop any more.
// BATCH: one launch advances up to 8 independent lattices (ResidentMember); the member index is uniform over a
// workgroup, so the member's fields are scalar loads before the step loop and the loop itself is the same.  One-XCD
// shapes: member m = blockIdx.x & 7 runs on XCD m, on the workgroups the single form leaves idle; other shapes: members
// take consecutive ranges of round_up(member_wgs, 8) blocks.  The seam protocol is per member (own granules, own tags).
// REC = kRecFrames: also record animation frames (ResidentFrames).  On a frame step the lid cells are relaxed WITHOUT the next
// step's accelerate_flow, |u| of the post-step lattice goes to the frame slot, and only then is accelerate_select applied
// to the relaxed values: bit-identical to the fused epilogue, since accelerate_select is a pure select on the relaxed
// values that never touches a blocked cell (the only cells bounce_select changes).
// REC = kRecProbes: also record point probes (ResidentProbes).  On a sample step a band without probes does nothing further; a
// band with probes walks its entries wave-uniformly and the lane that holds the cell stores its sample (one dwordx4).
// Only a band with a probe ON the lid row defers the lid's acceleration on sample steps, exactly as the frames do.
// REC = kRecMean: also accumulate the mean fields (ResidentMean).  A sample step is a frame step in every respect -- the same
// wave-uniform test, the same deferred acceleration of the lid cells, the same place in the step -- but instead of storing
// |u| into a slot every lane adds the four values of each of its cells to the cell's double sums in memory (load, add,
// store: a lane is the only writer of its cells and launches are stream-ordered, so neither atomics nor fences).  The
// sums are not kept in registers across steps: the planes stay in L2 / Infinity Cache between samples.  At order 2
// (ResidentMean::order, a scalar: the branch is wave-uniform and lies inside the sample branch) four more sums per cell,
// of the products, are updated the same way through the same descriptor.
// REC = kRecFields: also record field frames (ResidentFields).  A sample step is a frame step in every respect, as for the
// mean fields; the four values of a cell are the mean fields' (probe_sample), stored instead of accumulated, and only by
// the rows (a wave-uniform test) and lanes (their column) inside the window (take_fields).
template <bool BATCH, int REC>
using ResidentArgsOf = std::tuple_element_t<
    REC, std::conditional_t<BATCH, std::tuple<ResidentBatchArgs, ResidentBatchFramesArgs, ResidentBatchProbesArgs, ResidentBatchMeanArgs, ResidentBatchFieldsArgs>,
                            std::tuple<ResidentArgs, ResidentFramesArgs, ResidentProbesArgs, ResidentMeanArgs, ResidentFieldsArgs>>>;
template <int MAXT, bool JOINT = false, int ROWS = 4, bool BATCH = false, int REC = kRecNone>
__global__ __launch_bounds__(MAXT) void resident_band(const ResidentArgsOf<BATCH, REC> a) {
  static_assert(ROWS == 4 || ROWS == 2, "bands of four or two rows");
  constexpr int NE = (ROWS == 4) ? 10 : 4;  // wave-edge values per side
  // a workgroup holds a.group bands side by side (1: the usual case; more where a band has fewer than four waves and
  // the whole grid fits one XCD with one wave per SIMD, see a.one_xcd): `wave`, `n_waves` count inside the band,
  // `wv` inside the workgroup
  const int grp = (int)threadIdx.x / a.nx;
  const int x = (int)threadIdx.x - grp * a.nx, lane = x & 63, wave = x >> 6, n_waves = a.nx >> 6, wv = (int)threadIdx.x >> 6, wv0 = wv - wave;
  int n_wgs = a.one_xcd ? (int)(gridDim.x >> 3) : (int)gridDim.x, wg = a.one_xcd ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  ResidentMember mb{};
  ResidentFrames fr{};
  ResidentProbes pr{};
  ResidentMean mn{};
  const ResidentFields* fdp = nullptr;  // read where it is (kernel arguments / the members' table) on sample steps: eleven words fewer to keep
  if constexpr (BATCH) {
    const int stride = (a.member_wgs + 7) & ~7;
    const int member = a.one_xcd ? (int)(blockIdx.x & 7) : (int)blockIdx.x / stride;
    if (!a.one_xcd) { n_wgs = a.member_wgs; wg = (int)blockIdx.x - member * stride; }
    if (member >= a.n_members || wg >= n_wgs) return;
    mb = a.members[member];
    if constexpr (REC == kRecFrames) fr = a.frames[member];
    if constexpr (REC == kRecProbes) pr = a.probes[member];
    if constexpr (REC == kRecMean) mn = a.means[member];
    if constexpr (REC == kRecFields) fdp = a.fields + member;
  } else if (a.one_xcd && (blockIdx.x & 7) != 0) return;
  if constexpr (REC == kRecFrames && !BATCH) fr = a.fr;
  if constexpr (REC == kRecProbes && !BATCH) pr = a.pr;
  if constexpr (REC == kRecMean && !BATCH) mn = a.mn;
  if constexpr (REC == kRecFields && !BATCH) fdp = &a.fd;
#define RES_M(field) (BATCH ? mb.field : a.field)
  const int bands = n_wgs * a.group;
  // Workgroups are dealt to the 8 XCDs round-robin (observed, not promised): consecutive bands are given to
  // workgroups 8 apart, so that most seams join two bands on ONE XCD.  Speed only -- which seams really do is
  // established below from the hardware's own XCC id, and the protocol is correct for any placement.
  const int b = a.group * ((!a.one_xcd && a.xcd_affinity && (n_wgs & 7) == 0) ? (wg & 7) * (n_wgs >> 3) + (wg >> 3) : wg) + grp;
  const long ps = a.plane_stride;
  // wave-edge values: [parity][wave][side: 0 = lane 0's west-moving, 1 = lane 63's east-moving][NE used of 12]
  __shared__ __attribute__((aligned(16))) float edge[2][MAXT / 64][2][12];
  __shared__ float wave_part[2][MAXT / 64];
  if (b == a.absent_band) return;

  // ---- the band's rows.  ROWS = 4: interior pair ri = rows (1, 2), edge pair re = rows (0, 3); ROWS = 2: re = rows (0, 1)
  constexpr int TOP = ROWS - 1;  // the band's last row: the .y half of the edge pair
  f2 ri[kQ], re[kQ];
  {
    const float* base = RES_M(src) + (long)(ROWS * b) * a.row_pitch + x;
#pragma unroll
    for (int k = 0; k < kQ; k++) {
      re[k] = f2{base[k * ps], base[TOP * a.row_pitch + k * ps]};
      if constexpr (ROWS == 4) ri[k] = f2{base[1 * a.row_pitch + k * ps], base[2 * a.row_pitch + k * ps]};
      else ri[k] = splat2(0.f);
    }
  }
  const unsigned char* mp = RES_M(mask) + (long)(ROWS * b) * a.pitch + x;
  const unsigned blocked_e = (unsigned)mp[0] | ((unsigned)mp[TOP * a.pitch] << 8);
  unsigned blocked_i = 0;
  if constexpr (ROWS == 4) blocked_i = (unsigned)mp[a.pitch] | ((unsigned)mp[2 * a.pitch] << 8);
  // accelerate_flow's row, if this band holds it: bit per cell of the pair it falls in
  const int lid_local = a.accel_row - ROWS * b;
  const unsigned lid_i = (ROWS == 4) ? ((lid_local == 1) ? 1u : (lid_local == 2 ? 2u : 0u)) : 0u;
  const unsigned lid_e = (lid_local == 0) ? 1u : (lid_local == TOP ? 2u : 0u);

  // seam granules: `up` carries a band's top-row populations 2,5,6 northwards, `down` its row-0 populations 4,7,8;
  // byte offsets into the one buffer (32-bit: it is at most 16 MiB)
  const __amdgpu_buffer_rsrc_t grsrc = granule_rsrc(RES_M(gran), a.gran_bytes);
  const unsigned band_bytes = 2u * (unsigned)a.nx * 16u, slot_bytes = (unsigned)a.nx * 16u;
  const unsigned down_base = (unsigned)bands * band_bytes;
  const int bs = (b == 0) ? bands - 1 : b - 1, bn = (b == bands - 1) ? 0 : b + 1;
  const int xw = (x == 0) ? a.nx - 1 : x - 1, xe = (x == a.nx - 1) ? 0 : x + 1;
  const unsigned my_up = (unsigned)b * band_bytes + (unsigned)x * 16u;
  const unsigned my_down = down_base + (unsigned)b * band_bytes + (unsigned)x * 16u;
  const unsigned from_south = (unsigned)bs * band_bytes, from_north = down_base + (unsigned)bn * band_bytes;
  // which XCD do my neighbours run on?  Every band announces its XCC id in a granule of its own (sc1, tag = this
  // launch's first epoch); a seam whose two bands share an XCD keeps its granules in that XCD's L2 (plain stores),
  // any other seam writes them through (sc1).  The reader's loads are sc1 either way.
  bool north_local = false, south_local = false;
  if (a.xcd_affinity) {
    const unsigned hello_base = 2u * down_base;
    const unsigned my_xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xfu;  // HW_REG_XCC_ID[3:0]
    const unsigned hello_tag = a.epoch0 + 1u;
    if (x == 0) granule_store(grsrc, hello_base + (unsigned)b * 16u, __uint_as_float(my_xcc), 0.f, 0.f, hello_tag);
    long long t_start = 0;
    for (unsigned spins = 0;; spins++) {
      asm volatile("" ::: "memory");
      const granule_vec hs = granule_load(grsrc, hello_base + (unsigned)bs * 16u);
      const granule_vec hn = granule_load(grsrc, hello_base + (unsigned)bn * 16u);
      if ((unsigned)hs.w == hello_tag && (unsigned)hn.w == hello_tag) {
        south_local = ((unsigned)hs.x == my_xcc);
        north_local = ((unsigned)hn.x == my_xcc);
        break;
      }
      if ((spins & 63u) == 63u) {
        const long long now = wall_clock64();
        if (t_start == 0) t_start = now;
        const int st = __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (st != 0 || now - t_start > a.timeout_ticks) {
          if (st == 0 && lane == 0) __hip_atomic_store(a.status, kResidentTimeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          return;
        }
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  const int west_wave = wv0 + ((wave == 0) ? n_waves - 1 : wave - 1), east_wave = wv0 + ((wave == n_waves - 1) ? 0 : wave + 1);

  // publish the edge rows of a state: step s of this launch reads what was published with its tag into its slot
  auto publish = [&](int s) {
    const unsigned tag = a.epoch0 + (unsigned)s + 1u;
    const unsigned off = (unsigned)(s & 1) * slot_bytes;
    if (north_local) granule_store_local(grsrc, my_up + off, re[2].y, re[5].y, re[6].y, tag);
    else granule_store(grsrc, my_up + off, re[2].y, re[5].y, re[6].y, tag);
    if (south_local) granule_store_local(grsrc, my_down + off, re[4].x, re[7].x, re[8].x, tag);
    else granule_store(grsrc, my_down + off, re[4].x, re[7].x, re[8].x, tag);
  };
  if (a.n_steps > 0) publish(0);
  // frames: local step of the next one (~0u: none) and its slot
  unsigned f_next = ~0u;
  int f_slot = 0;
  if constexpr (REC == kRecFrames) {
    if (fr.every > 0) {
      const unsigned e = (unsigned)fr.every, r = a.epoch0 % e;
      f_next = r ? e - r : 0u;
      f_slot = (int)(((a.epoch0 + f_next) / e - (unsigned)fr.ord0) % (unsigned)fr.slots);
    }
  }

  // frames: |u| of the band's post-step cells (re, ri) into the slot, then the deferred accelerate_flow of the next step
  // on `lidp`, the pair that holds the lid row (ROWS = 4: ri, ROWS = 2: the new edge pair)
  auto take_frame = [&](f2 (&lidp)[kQ], bool accel_next) {
    // the slot as a buffer (scalar base, 32-bit lane offset computed here): no 64-bit address stays live in VGPRs
    const unsigned row_bytes = (unsigned)a.nx * 4u;
    const __amdgpu_buffer_rsrc_t frsrc = __builtin_amdgcn_make_buffer_rsrc(fr.base + (long)f_slot * a.ny * a.nx, 0, (int)(row_bytes * (unsigned)a.ny), 0x00020000);
    const int lane_off = (int)((unsigned)(ROWS * b) * row_bytes + (unsigned)x * 4u);
    const f2 (&fe)[kQ] = (ROWS == 4) ? re : lidp;
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(frame_speed(fe, 0, (blocked_e & 0xffu) != 0)), frsrc, lane_off, 0, 2);  // aux 2 = nt
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(frame_speed(fe, 1, (blocked_e & 0xff00u) != 0)), frsrc, lane_off, (int)(TOP * row_bytes), 2);
    if constexpr (ROWS == 4) {
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(frame_speed(ri, 0, (blocked_i & 0xffu) != 0)), frsrc, lane_off, (int)row_bytes, 2);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(frame_speed(ri, 1, (blocked_i & 0xff00u) != 0)), frsrc, lane_off, (int)(2 * row_bytes), 2);
    }
    const unsigned lid = (ROWS == 4) ? lid_i : lid_e, blk = (ROWS == 4) ? blocked_i : blocked_e;
    if (accel_next && lid != 0)
      accelerate_select(lidp, (lid & 1u) != 0 && (blk & 0xffu) == 0, (lid & 2u) != 0 && (blk & 0xff00u) == 0, RES_M(a1), RES_M(a2));
    f_next += (unsigned)fr.every;
    f_slot = (f_slot + 1 == fr.slots) ? 0 : f_slot + 1;
  };

  // probes: the same bookkeeping (f_next, f_slot count sample rows) and this band's word of the table
  unsigned p_range = 0;
  if constexpr (REC == kRecProbes) {
    if (pr.every > 0) {
      const unsigned e = (unsigned)pr.every, r = a.epoch0 % e;
      f_next = r ? e - r : 0u;
      f_slot = (int)(((a.epoch0 + f_next) / e - (unsigned)pr.ord0) % (unsigned)pr.slots);
      p_range = (unsigned)__builtin_amdgcn_readfirstlane((int)reinterpret_cast<const unsigned*>(pr.table + pr.n_probes)[b]);
    }
  }
  // probes: the samples of this band's probed cells -- edge pair `pe`, interior pair ri, both post-step -- into the ring's
  // row, then the deferred accelerate_flow on `lidp` (see take_frame) where this band deferred it
  auto take_probes = [&](const f2 (&pe)[kQ], f2 (&lidp)[kQ], bool deferred) {
    const unsigned count = (p_range >> 12) & 0xfffu;
    if (count != 0) {
      const __amdgpu_buffer_rsrc_t prsrc = __builtin_amdgcn_make_buffer_rsrc(pr.ring, 0, pr.slots * pr.n_probes * 16, 0x00020000);
      const ProbeEntry* ent = pr.table + (p_range & 0xfffu);
      const int row0 = __builtin_amdgcn_readfirstlane(ROWS * b);
      for (unsigned j = 0; j < count; j++) {  // wave-uniform
        const int rb = __builtin_amdgcn_readfirstlane(ent[j].row) - row0;
        const unsigned xi = (unsigned)__builtin_amdgcn_readfirstlane((int)ent[j].xi);
        if ((int)(xi & 0xfffffu) == x) {
          float f[kQ];
          unsigned blk;
          if constexpr (ROWS == 4) {
#pragma unroll
            for (int k = 0; k < kQ; k++) f[k] = (rb == 0) ? pe[k].x : (rb == 3) ? pe[k].y : (rb == 1) ? ri[k].x : ri[k].y;
            blk = (rb == 0) ? (blocked_e & 0xffu) : (rb == 3) ? (blocked_e & 0xff00u) : (rb == 1) ? (blocked_i & 0xffu) : (blocked_i & 0xff00u);
          } else {
#pragma unroll
            for (int k = 0; k < kQ; k++) f[k] = (rb == 0) ? pe[k].x : pe[k].y;
            blk = (rb == 0) ? (blocked_e & 0xffu) : (blocked_e & 0xff00u);
          }
          const probe_vec v = probe_sample(f, blk != 0, pr.density);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(granule_vec, v), prsrc, 0, (f_slot * pr.n_probes + (int)(xi >> 20)) * 16, 0);
        }
      }
    }
    if (deferred) {
      const unsigned lid = (ROWS == 4) ? lid_i : lid_e, blk = (ROWS == 4) ? blocked_i : blocked_e;
      accelerate_select(lidp, (lid & 1u) != 0 && (blk & 0xffu) == 0, (lid & 2u) != 0 && (blk & 0xff00u) == 0, RES_M(a1), RES_M(a2));
    }
    f_next += (unsigned)pr.every;
    f_slot = (f_slot + 1 == pr.slots) ? 0 : f_slot + 1;
  };

  // mean fields: the frames' test for the next sample step (f_next); nothing else is counted
  if constexpr (REC == kRecMean) {
    if (mn.every > 0) {
      const unsigned e = (unsigned)mn.every, r = a.epoch0 % e;
      f_next = r ? e - r : 0u;
    }
  }
  // mean fields: the four values of the band's post-step cells -- edge pair `pe`, interior pair ri -- added to the cells'
  // sums, then the deferred accelerate_flow of the next step on `lidp` (see take_frame)
  auto take_mean = [&](const f2 (&pe)[kQ], f2 (&lidp)[kQ], bool accel_next) {
    // the armed planes, four or eight, as one buffer (scalar base, 32-bit lane offset; at most 32 MiB at order 1 and
    // 64 MiB at order 2, the 1024 x 1024 lattice): no 64-bit address lives in VGPRs
    const bool second = (mn.order == 2);  // wave-uniform
    const unsigned row_bytes = (unsigned)a.nx * 8u, plane_bytes = (unsigned)mn.plane_stride * 8u;
    const __amdgpu_buffer_rsrc_t mrsrc = __builtin_amdgcn_make_buffer_rsrc(mn.base, 0, (int)((second ? 8u : 4u) * plane_bytes), 0x00020000);
    const int lane_off = (int)((unsigned)(ROWS * b) * row_bytes + (unsigned)x * 8u);
    auto add_cell = [&](const f2 (&p)[kQ], int c, bool blocked, int row) {
      float f[kQ];
#pragma unroll
      for (int k = 0; k < kQ; k++) f[k] = p[k][c];
      const probe_vec v = probe_sample(f, blocked, mn.density);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int soff = (int)((unsigned)j * plane_bytes + (unsigned)row * row_bytes);
        const double acc = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(mrsrc, lane_off, soff, 0));
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(mean_word, acc + (double)v[j]), mrsrc, lane_off, soff, 0);
      }
      if (second) {
        // planes 4..7: u_x u_x, u_y u_y, u_x u_y, pressure pressure; each product is exact in a double
        const double ux = (double)v[0], uy = (double)v[1], pr = (double)v[3];
        const double prod[4] = {ux * ux, uy * uy, ux * uy, pr * pr};
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int soff = (int)((unsigned)(4 + j) * plane_bytes + (unsigned)row * row_bytes);
          const double acc = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(mrsrc, lane_off, soff, 0));
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(mean_word, acc + prod[j]), mrsrc, lane_off, soff, 0);
        }
      }
    };
    add_cell(pe, 0, (blocked_e & 0xffu) != 0, 0);
    add_cell(pe, 1, (blocked_e & 0xff00u) != 0, TOP);
    if constexpr (ROWS == 4) {
      add_cell(ri, 0, (blocked_i & 0xffu) != 0, 1);
      add_cell(ri, 1, (blocked_i & 0xff00u) != 0, 2);
    }
    const unsigned lid = (ROWS == 4) ? lid_i : lid_e, blk = (ROWS == 4) ? blocked_i : blocked_e;
    if (accel_next && lid != 0)
      accelerate_select(lidp, (lid & 1u) != 0 && (blk & 0xffu) == 0, (lid & 2u) != 0 && (blk & 0xff00u) == 0, RES_M(a1), RES_M(a2));
    f_next += (unsigned)mn.every;
  };

  // field frames: the frames' bookkeeping (f_next, f_slot); the sample itself is take_fields (a function, not a lambda
  // of this kernel: a closure defined here, used or not, reorders the scalar moves of the other forms' prologues)
  if constexpr (REC == kRecFields) {
    if (fdp->every > 0) {
      const unsigned e = (unsigned)fdp->every, r = a.epoch0 % e;
      f_next = r ? e - r : 0u;
      f_slot = (int)(((a.epoch0 + f_next) / e - (unsigned)fdp->ord0) % (unsigned)fdp->slots);
    }
  }

  bool alive = true;
#ifdef LBM_RESIDENT_PROFILE
  long long prof_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, prof_t = prof_clock();
#endif
  for (int s = 0; s < a.n_steps && alive; s++) {
    const unsigned tag = a.epoch0 + (unsigned)s + 1u;
    const int slot = s & 1;
    // (the edge rows of the current state were published as soon as they existed: before the loop / at the end of
    // the previous iteration)
    // ---- wave-edge lanes through LDS ------------------------------------------------------------------------
    // ROWS = 4: east-moving (from lane 63) 1 of rows 0..3, 5 of rows 0..2, 8 of rows 1..3; west-moving (from lane 0) 3, 6, 7
    // ROWS = 2: east-moving 1 of rows 0, 1, 5 of row 0, 8 of row 1; west-moving 3 of rows 0, 1, 6 of row 0, 7 of row 1
    if (lane == 63) {
      float* e = edge[slot][wv][1];
      if constexpr (ROWS == 4) {
        e[0] = re[1].x; e[1] = ri[1].x; e[2] = ri[1].y; e[3] = re[1].y;
        e[4] = re[5].x; e[5] = ri[5].x; e[6] = ri[5].y; e[7] = ri[8].x;
        e[8] = ri[8].y; e[9] = re[8].y;
      } else {
        e[0] = re[1].x; e[1] = re[1].y; e[2] = re[5].x; e[3] = re[8].y;
      }
    }
    if (lane == 0) {
      float* e = edge[slot][wv][0];
      if constexpr (ROWS == 4) {
        e[0] = re[3].x; e[1] = ri[3].x; e[2] = ri[3].y; e[3] = re[3].y;
        e[4] = re[6].x; e[5] = ri[6].x; e[6] = ri[6].y; e[7] = ri[7].x;
        e[8] = ri[7].y; e[9] = re[7].y;
      } else {
        e[0] = re[3].x; e[1] = re[3].y; e[2] = re[6].x; e[3] = re[7].y;
      }
    }
    RESIDENT_PROF(0);  // wave-edge values into LDS
    __syncthreads();
    RESIDENT_PROF(1);  // barrier
    if (s > 0 && wave == 0) {
      // the per-wave sums of the previous step, written before this barrier: one partial per band and step
      const float v = row16_sum_dpp((lane < n_waves) ? wave_part[slot ^ 1][wv0 + lane] : 0.f);
      if (lane == 0) RES_M(partials)[(long)(s - 1) * bands + b] = v;
    }
    float W[NE], E[NE];
    {
      const float* w = edge[slot][west_wave][1];
      const float* e = edge[slot][east_wave][0];
#pragma unroll
      for (int j = 0; j < NE; j++) { W[j] = w[j]; E[j] = e[j]; }
    }
    // ---- the halo granules are asked for NOW, before anything else is computed: when the neighbours are not late
    // (the usual case: their edge rows were published about when ours were) the answer is there by the time the
    // interior pair is done, and the round trip of the load is hidden behind it
    const unsigned gs = from_south + (unsigned)slot * slot_bytes, gn = from_north + (unsigned)slot * slot_bytes;
    // the wave's first lane also needs the column west of it, its last lane the column east of it (every lane issues
    // the second load, the inner lanes for their own column again: four loads in flight, one wait, no divergence)
    const bool first = (lane == 0), last = (lane == 63);
    const unsigned x_side = (unsigned)(first ? xw : (last ? xe : x)) * 16u;
    granule_vec cs = granule_load(grsrc, gs + (unsigned)x * 16u);
    granule_vec cn = granule_load(grsrc, gn + (unsigned)x * 16u);
    granule_vec ss = granule_load(grsrc, gs + x_side);
    granule_vec sn = granule_load(grsrc, gn + x_side);

    bool frame_now = false;
    if constexpr (REC == kRecFrames || REC == kRecMean || REC == kRecFields) frame_now = ((unsigned)s == f_next);  // wave-uniform
    // probes: a sample step; only a band with a probe on the lid row defers the lid's acceleration as a frame step does
    bool sample_now = false;
    if constexpr (REC == kRecProbes) {
      sample_now = ((unsigned)s == f_next);
      frame_now = sample_now && (p_range >> 31) != 0;
    }
    const bool accel_next = (s + 1 < a.n_steps) || a.accel_last;
    // a frame step applies the lid's acceleration after taking the frame (take_frame).  ROWS = 4: the lid row is
    // band row 2 (ny - 2 with ny % 4 == 0; run_resident checks it), an interior row, so only the interior pair defers
    const bool accel = accel_next && !(ROWS == 2 && frame_now);
    const bool accel_i = (REC != kRecNone) ? accel_next && !frame_now : accel;
    // shifted populations (the value each cell receives from its west / east neighbour) and the streamed inputs of
    // the pair(s), as far as they come from inside the band
    f2 ti[kQ], te[kQ];
    if constexpr (ROWS == 4) {
      const float s1_0 = shift_from_west(re[1].x, W[0]), s1_1 = shift_from_west(ri[1].x, W[1]);
      const float s1_2 = shift_from_west(ri[1].y, W[2]), s1_3 = shift_from_west(re[1].y, W[3]);
      const float s5_0 = shift_from_west(re[5].x, W[4]), s5_1 = shift_from_west(ri[5].x, W[5]), s5_2 = shift_from_west(ri[5].y, W[6]);
      const float s8_1 = shift_from_west(ri[8].x, W[7]), s8_2 = shift_from_west(ri[8].y, W[8]), s8_3 = shift_from_west(re[8].y, W[9]);
      const float s3_0 = shift_from_east(re[3].x, E[0]), s3_1 = shift_from_east(ri[3].x, E[1]);
      const float s3_2 = shift_from_east(ri[3].y, E[2]), s3_3 = shift_from_east(re[3].y, E[3]);
      const float s6_0 = shift_from_east(re[6].x, E[4]), s6_1 = shift_from_east(ri[6].x, E[5]), s6_2 = shift_from_east(ri[6].y, E[6]);
      const float s7_1 = shift_from_east(ri[7].x, E[7]), s7_2 = shift_from_east(ri[7].y, E[8]), s7_3 = shift_from_east(re[7].y, E[9]);
      // interior pair: rows 1 and 2 pull from rows 0..3 of the band only
      ti[0] = ri[0];               ti[1] = f2{s1_1, s1_2};      ti[2] = f2{re[2].x, ri[2].x};
      ti[3] = f2{s3_1, s3_2};      ti[4] = f2{ri[4].y, re[4].y}; ti[5] = f2{s5_0, s5_1};
      ti[6] = f2{s6_0, s6_1};      ti[7] = f2{s7_2, s7_3};      ti[8] = f2{s8_2, s8_3};
      // edge pair: rows 0 and 3; the halves that come from the neighbouring bands are filled in below
      te[0] = re[0];               te[1] = f2{s1_0, s1_3};      te[2] = f2{0.f, ri[2].y};
      te[3] = f2{s3_0, s3_3};      te[4] = f2{ri[4].x, 0.f};     te[5] = f2{0.f, s5_2};
      te[6] = f2{0.f, s6_2};       te[7] = f2{s7_1, 0.f};       te[8] = f2{s8_1, 0.f};
    } else {
      const float s1_0 = shift_from_west(re[1].x, W[0]), s1_1 = shift_from_west(re[1].y, W[1]);
      const float s5_0 = shift_from_west(re[5].x, W[2]), s8_1 = shift_from_west(re[8].y, W[3]);
      const float s3_0 = shift_from_east(re[3].x, E[0]), s3_1 = shift_from_east(re[3].y, E[1]);
      const float s6_0 = shift_from_east(re[6].x, E[2]), s7_1 = shift_from_east(re[7].y, E[3]);
      te[0] = re[0];               te[1] = f2{s1_0, s1_1};      te[2] = f2{0.f, re[2].x};
      te[3] = f2{s3_0, s3_1};      te[4] = f2{re[4].y, 0.f};     te[5] = f2{0.f, s5_0};
      te[6] = f2{0.f, s6_0};       te[7] = f2{s7_1, 0.f};       te[8] = f2{s8_1, 0.f};
#pragma unroll
      for (int k = 0; k < kQ; k++) ti[k] = splat2(0.f);
    }
    f2 ni[kQ];
    float sum = 0.f;
    if constexpr (ROWS == 4 && !JOINT) sum = relax_pair_rows(ti, blocked_i, accel_i ? lid_i : 0u, RES_M(omega), RES_M(a1), RES_M(a2), ni);

    RESIDENT_PROF(2);  // partial of the previous step, LDS edges read, shifts, halo loads issued, interior pair (ROWS 4, !JOINT)
    // ---- edge pair: rows 0 and TOP also pull from the neighbouring bands --------------------------------------
    {
      long long t_start = 0;
      for (unsigned spins = 0;; spins++) {
        const bool ok = ((unsigned)cs.w == tag) & ((unsigned)cn.w == tag) & ((unsigned)ss.w == tag) & ((unsigned)sn.w == tag);
#ifdef LBM_RESIDENT_PROFILE
        if (spins == 0) RESIDENT_PROF(3);  // first answer of the halo loads
        else prof_acc[7] += 1;
#endif
        if (__all(ok)) break;
        // not there yet: every so often look at the clock and at what the other workgroups say (wave-uniform)
        if ((spins & 63u) == 63u) {
          const long long now = wall_clock64();
          if (t_start == 0) t_start = now;
          const int st = __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (st != 0 || now - t_start > a.timeout_ticks) {
            if (st == 0 && lane == 0) __hip_atomic_store(a.status, kResidentTimeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            alive = false;
            break;
          }
        }
        // how long to stay off the issue ports before asking again: short where the wave sits alone on its SIMD
        // (latency is everything), long where three other waves want the slots (a poll is ~25 instructions)
        // (a compile-time choice: measured over 0 ... 16 at every size the value hardly matters, and as a run-time switch
        // it cost a dozen scalar instructions and four branches per look)
        __builtin_amdgcn_s_sleep(MAXT > 512 ? 4 : 1);
        asm volatile("" ::: "memory");  // the loads must be issued again in every spin
        cs = granule_load(grsrc, gs + (unsigned)x * 16u);
        cn = granule_load(grsrc, gn + (unsigned)x * 16u);
        ss = granule_load(grsrc, gs + x_side);
        sn = granule_load(grsrc, gn + x_side);
      }
    }
    RESIDENT_PROF(4);  // further polls
    // south: {2, 5, 6} of its top row; north: {4, 7, 8} of its row 0; 5 and 8 come from the west column, 6 and 7 from the east
    const float side_s = __uint_as_float((unsigned)(first ? ss.y : ss.z)), side_n = __uint_as_float((unsigned)(first ? sn.z : sn.y));
    te[2].x = __uint_as_float((unsigned)cs.x);
    te[4].y = __uint_as_float((unsigned)cn.x);
    te[5].x = shift_from_west(__uint_as_float((unsigned)cs.y), side_s);
    te[6].x = shift_from_east(__uint_as_float((unsigned)cs.z), side_s);
    te[7].y = shift_from_east(__uint_as_float((unsigned)cn.y), side_n);
    te[8].y = shift_from_west(__uint_as_float((unsigned)cn.z), side_n);
    f2 ne[kQ];
    if constexpr (ROWS == 4 && JOINT) sum = relax_two_pairs_rows(ti, te, blocked_i, blocked_e, accel_i ? lid_i : 0u, accel ? lid_e : 0u, RES_M(omega), RES_M(a1), RES_M(a2), ni, ne);
    else sum += relax_pair_rows(te, blocked_e, accel ? lid_e : 0u, RES_M(omega), RES_M(a1), RES_M(a2), ne);
    if constexpr (REC == kRecFrames && ROWS == 2) {
      if (frame_now) take_frame(ne, accel_next);
    }
    if constexpr (REC == kRecProbes && ROWS == 2) {
      if (sample_now) take_probes(ne, ne, frame_now && accel_next && lid_e != 0);
    }
    if constexpr (REC == kRecMean && ROWS == 2) {
      if (frame_now) take_mean(ne, ne, accel_next);
    }
    if constexpr (REC == kRecFields && ROWS == 2) {
      if (frame_now) take_fields<ROWS>(*fdp, ROWS * b, x, ne, ri, ne, blocked_e, blocked_i, lid_e, accel_next, RES_M(a1), RES_M(a2), f_next, f_slot);
    }
#pragma unroll
    for (int k = 0; k < kQ; k++) {
      re[k] = ne[k];
      if constexpr (ROWS == 4) ri[k] = ni[k];
    }
    RESIDENT_PROF(5);  // collision(s)
    // the neighbours wait for exactly these rows: out they go, before anything else
    if (s + 1 < a.n_steps && alive) publish(s + 1);
    // blocked cells report 0; sum over the wave, one partial per wave into LDS (summed after the next barrier)
    const float tot = wave_sum_dpp(sum);
    if (lane == 63) wave_part[slot][wv] = tot;
    // ROWS = 4: the frame once the step's own work is out (fewest live registers: the 128-VGPR form does not spill)
    if constexpr (REC == kRecFrames && ROWS == 4) {
      if (frame_now) take_frame(ri, accel_next);
    }
    if constexpr (REC == kRecProbes && ROWS == 4) {
      if (sample_now) take_probes(re, ri, frame_now && accel_next && lid_i != 0);
    }
    if constexpr (REC == kRecMean && ROWS == 4) {
      if (frame_now) take_mean(re, ri, accel_next);
    }
    if constexpr (REC == kRecFields && ROWS == 4) {
      if (frame_now) take_fields<ROWS>(*fdp, ROWS * b, x, re, ri, ri, blocked_e, blocked_i, lid_i, accel_next, RES_M(a1), RES_M(a2), f_next, f_slot);
    }
    RESIDENT_PROF(6);  // publish, wave sum
    // (a wave that gave up leaves the loop alone: the hardware barrier counts only waves that have not ended, and
    // the others find *status set in their next spin)
  }

#ifdef LBM_RESIDENT_PROFILE
  if (x == 0)
    for (int i = 0; i < 8; i++) a.prof[b * 8 + i] = prof_acc[i];
#endif
  __syncthreads();
  if (a.n_steps > 0 && wave == 0) {
    const float v = row16_sum_dpp((lane < n_waves) ? wave_part[(a.n_steps - 1) & 1][wv0 + lane] : 0.f);
    if (lane == 0) RES_M(partials)[(long)(a.n_steps - 1) * bands + b] = v;
  }
  float* out = RES_M(dst) + (long)(ROWS * b) * a.row_pitch + x;
#pragma unroll
  for (int k = 0; k < kQ; k++) {
    out[k * ps] = re[k].x;
    out[TOP * a.row_pitch + k * ps] = re[k].y;
    if constexpr (ROWS == 4) {
      out[1 * a.row_pitch + k * ps] = ri[k].x;
      out[2 * a.row_pitch + k * ps] = ri[k].y;
    }
  }
}
#undef RES_M

// resident kernel: sum the per-band partials of each step in a fixed order (double) -> tot_u[step_base + s]
__device__ __forceinline__ void reduce_band_partials_at(const float* p, int bands, double* out) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < bands; i += 64) acc += (double)p[i];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (threadIdx.x == 0) *out = acc;
}
__global__ __launch_bounds__(64) void reduce_band_partials(const float* partials, int bands, double* tot_u, int step_base) {
  reduce_band_partials_at(partials + (long)blockIdx.x * bands, bands, tot_u + step_base + blockIdx.x);
}
// the same for every member of a batch at once: grid (steps, members)
__global__ __launch_bounds__(64) void reduce_band_partials_batch(const ResidentMember* members, int bands, int step_base) {
  const ResidentMember& m = members[blockIdx.y];
  reduce_band_partials_at(m.partials + (long)blockIdx.x * bands, bands, m.tot_u + step_base + blockIdx.x);
}

// ---------------------------------------------------------------------------------------------
// fused step, 1 cell per lane: any nx (fallback for widths that are not a multiple of 4)
// ---------------------------------------------------------------------------------------------
template <bool EXACT>
__global__ __launch_bounds__(kBlock) void step_scalar(const StepArgs a) {
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  const long n_cells = (long)a.nx * a.n_rows;
  float my_sum = 0.f;
  if (q < n_cells) {
    const int rsel = (int)(q / a.nx);
    const int x = (int)(q - (long)rsel * a.nx);
    const int row = a.row_first + rsel * a.row_stride;
    const int xw = (x == 0) ? a.nx - 1 : x - 1;
    const int xe = (x + 1 == a.nx) ? 0 : x + 1;
    const long ps = a.plane_stride;
    const float* c_row = a.src + (long)row * a.row_pitch;
    const int rs = (row == 0 && a.wrap) ? a.rows - 1 : row - 1;
    const int rn = (row == a.rows - 1 && a.wrap) ? 0 : row + 1;
    const float* sb = a.src + (long)rs * a.row_pitch;
    const float* nb = a.src + (long)rn * a.row_pitch;
    const float *s2 = sb + 2 * ps, *s5 = sb + 5 * ps, *s6 = sb + 6 * ps;
    const float *n4 = nb + 4 * ps, *n7 = nb + 7 * ps, *n8 = nb + 8 * ps;
    float t[kQ] = {c_row[x], c_row[1 * ps + xw], s2[x], c_row[3 * ps + xe], n4[x],
                   s5[xw],   s6[xe],             n7[xe], n8[xw]};
    float r[kQ];
    if (a.mask[(long)row * a.pitch + x]) {
      bounce(t, r);
    } else {
      float speed;
      collide<EXACT>(t, a.omega, r, speed);
      my_sum = speed;
      if (row == a.accel_row) accelerate(r, a.a1, a.a2);
    }
    float* d = a.dst + (long)row * a.row_pitch + x;
#pragma unroll
    for (int k = 0; k < kQ; k++) d[k * ps] = r[k];
  }
  const float total = block_sum(my_sum);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------------------------
// small kernels around the step
// ---------------------------------------------------------------------------------------------

// accelerate_flow() as its own pass (SerialCode/d2q9-bgk.c:216-246): used once before the first
// step of a run; later steps get it from the epilogue of the step kernel.
__device__ __forceinline__ void accelerate_row_at(const LatticeArgs& a, int row, float a1, float a2) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= a.nx) return;
  if (cell_blocked(a, row, x)) return;
  const long ps = a.plane_stride;
  float* lat = a.dst + (long)row * a.row_pitch + x;
  float f[kQ];
#pragma unroll
  for (int k = 0; k < kQ; k++) f[k] = lat[k * ps];
  accelerate(f, a1, a2);
  lat[1 * ps] = f[1];  lat[3 * ps] = f[3];  lat[5 * ps] = f[5];
  lat[6 * ps] = f[6];  lat[7 * ps] = f[7];  lat[8 * ps] = f[8];
}
__global__ void accelerate_row(const LatticeArgs a, int row, float a1, float a2) { accelerate_row_at(a, row, a1, a2); }
// the same on the current lattice of every member of a batch: grid (ceil(nx / block), members); `a` gives the members'
// common strides, each member its own lattice and mask
__global__ void accelerate_row_batch(const ResidentMember* members, LatticeArgs a, int row) {
  const ResidentMember& m = members[blockIdx.y];
  a.dst = m.src;
  a.mask = m.mask;
  accelerate_row_at(a, row, m.a1, m.a2);
}

// ---------------------------------------------------------------------------------------------
// steady-state runs (lbm_run_until): the convergence verdict is taken on the device, next to tot_u
// ---------------------------------------------------------------------------------------------
// what one lattice's checks have found so far; lives on the device, reset at the start of every lbm_run_until call
struct SteadyState {
  double prev_mean;   // m_j of the last segment seen
  double last_rel;    // r_j of the last check (+inf before the first)
  int streak;         // consecutive checks met
  int checks;         // checks made (segments 2, 3, ...)
  int segments;       // segments seen
  int stop;           // 1 once streak == patience: later checks change nothing, accelerate_row_unless does nothing
  int steady_step;    // steps of the call after which that happened (-1: not yet)
  int pad;
};
struct SteadyMember {  // one lattice of a batch, as steady_check_batch sees it
  const double* tot_u;
  float cells;         // (float)fluid_cells
};
struct SteadyBatch {
  int n_steady;        // members whose stop is set
  int all_steady;      // 1 once that is all of them
};

__global__ void steady_reset(SteadyState* st, int n, SteadyBatch* batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) st[i] = SteadyState{0.0, __builtin_inf(), 0, 0, 0, 0, -1, 0};
  if (i == 0 && batch) *batch = SteadyBatch{0, 0};
}

// One wave: the mean of the segment's av_vels -- av[s] = (float)tot_u[s] / cells as lbm_read_av_vels computes it, summed
// as doubles in the order of reduce_band_partials_at -- against the mean of the segment before.  Returns true (lane 0)
// when this check made the lattice steady.
__device__ __forceinline__ bool steady_check_at(const double* tot_u, int n, float cells, double tol, int patience,
                                                int steps_after, SteadyState* st) {
  if (st->stop) return false;  // uniform: the verdict stands, a look-ahead segment's check changes nothing
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) acc += (double)((float)tot_u[i] / cells);
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (threadIdx.x != 0) return false;
  const double m = acc / (double)n;
  const int seg = st->segments + 1;
  bool now_steady = false;
  if (seg >= 2) {
    const double prev = st->prev_mean;
    const double r = (m == 0.0) ? (prev == 0.0 ? 0.0 : __builtin_inf()) : fabs(m - prev) / fabs(m);
    const int streak = (r <= tol) ? st->streak + 1 : 0;
    st->streak = streak;
    st->checks += 1;
    st->last_rel = r;
    if (streak >= patience) {
      st->stop = 1;
      st->steady_step = steps_after;
      now_steady = true;
    }
  }
  st->segments = seg;
  st->prev_mean = m;
  return now_steady;
}
__global__ __launch_bounds__(64) void steady_check(const double* tot_u, int first, int n, float cells, double tol,
                                                   int patience, int steps_after, SteadyState* st) {
  steady_check_at(tot_u + first, n, cells, tol, patience, steps_after, st);
}
// every member of a batch at once, one wave per member: grid (members).  The member that completes the set raises
// all_steady (an integer count: the outcome does not depend on the order the waves run in).
__global__ __launch_bounds__(64) void steady_check_batch(const SteadyMember* members, int n_members, int first, int n,
                                                         double tol, int patience, int steps_after, SteadyState* st,
                                                         SteadyBatch* batch) {
  const SteadyMember m = members[blockIdx.x];
  if (steady_check_at(m.tot_u + first, n, m.cells, tol, patience, steps_after, st + blockIdx.x)) {
    const int before = __hip_atomic_fetch_add(&batch->n_steady, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (before + 1 == n_members) __hip_atomic_store(&batch->all_steady, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// accelerate_row for the first step of a segment that was enqueued before the verdict of the segment in front of it was
// known: nothing happens once that verdict is "stop", so the lattice the call returns is not accelerated a second time
__global__ void accelerate_row_unless(const LatticeArgs a, int row, float a1, float a2, const SteadyState* st) {
  if (st->stop) return;  // one scalar load, wave-uniform
  accelerate_row_at(a, row, a1, a2);
}

// ---------------------------------------------------------------------------------------------
// "freshest available" halo mode (LBM_HALO_FRESHEST): the reference's MPI_Testall idea, MPI_Testall_OptimizedVersion/
// d2q9-bgk.c:279-290 -- look once whether this step's halo rows have arrived, never wait for them.  The rows travel
// into a staging row per side, followed in stream order by the id of the step they belong to (fresh_mark / a 4-byte
// copy); after the interior rows, fresh_decide looks at the ids ONCE, notes which sides made it (the engine's log of
// decisions) and fresh_adopt moves those staging rows into the halo rows, whole rows only.  The sides that did not make
// it keep the rows of the step before, which the one-pass-late exchange of the stale mode has put there.
// ---------------------------------------------------------------------------------------------
__global__ void fresh_mark(unsigned* a, unsigned* b, unsigned id) {
  if (a) __hip_atomic_store(a, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (b) __hip_atomic_store(b, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// tests (LBM_FRESH_TEST_DELAY_US): holds a comm stream back so that looks find nothing; bounded by the clock
__global__ void fresh_test_delay(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
// arrived[0] / arrived[1]: id of the step whose south / north halo row the staging holds; mode 0: look (the product),
// 1: this pass's halo rows are fresh anyway (first pass of a call): note 3, adopt nothing
__global__ void fresh_decide(const unsigned* arrived, unsigned id, int mode, int* decision, unsigned char* log_entry) {
  unsigned d = 0;
  if (mode == 0) {
    d = (__hip_atomic_load(arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == id ? 1u : 0u) |
        (__hip_atomic_load(arrived + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == id ? 2u : 0u);
    *decision = (int)d;
  } else {
    *decision = 0;
    d = 3;
  }
  *log_entry = (unsigned char)d;
}
// staging rows (written by a peer: read past the caches) -> halo rows, per side as decided
__global__ void fresh_adopt(const int* decision, const unsigned* stage_s, const unsigned* stage_n, unsigned* halo_s, unsigned* halo_n, long n) {
  const int d = *decision;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (d & 1) halo_s[i] = __hip_atomic_load(stage_s + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (d & 2) halo_n[i] = __hip_atomic_load(stage_n + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// sum the per-workgroup partials of up to gridDim.x steps: block s adds partials[s][0..n[s])
// in a fixed order (double accumulation) -> tot_u[step_base + s].  Deterministic, no atomics.
constexpr int kPartSlotsMax = 64;
struct SlotCounts {
  int n[kPartSlotsMax];  // valid partials in each slot (launch geometries differ between kernels)
};
// base_dev (optional): the first step's index is read from device memory, so that a captured hipGraph can be
// replayed for later steps (advance_counter moves it on)
__global__ __launch_bounds__(kBlock) void reduce_partials(const float* partials, SlotCounts counts,
                                                          long slot_stride, double* tot_u,
                                                          int step_base, const int* base_dev) {
  __shared__ double sh[kBlock];
  if (base_dev) step_base += *base_dev;
  const float* p = partials + (long)blockIdx.x * slot_stride;
  const int n_part = counts.n[blockIdx.x];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_part; i += kBlock) acc += (double)p[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) tot_u[step_base + blockIdx.x] = sh[0];
}

__global__ void set_counter(int* p, int value) { *p = value; }
__global__ void advance_counter(int* p, int by) { *p += by; }

// obstacle flags: the reference's int map (1 = blocked, SerialCode/d2q9-bgk.c:541, 570-601) -> uint8 rows of `pitch`
__global__ void mask_from_int(const int* src, unsigned char* dst, int nx, int pitch, int nrows) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)nx * nrows) return;
  const int r = (int)(i / nx), x = (int)(i - (long)r * nx);
  dst[(long)r * pitch + x] = src[i] ? 1 : 0;
}

// ... or a small tile repeated over the grid: cell (x, y) is blocked iff the tile's cell (x mod tnx, y mod tny) is
// (the synthetic 8192^2 / 16384^2 grids tile the reference's 1024^2 map).  Mask row r is
// global row row0 + r, folded periodically into [0, ny).
__global__ void mask_from_tile(const unsigned char* tile, int tnx, int tny, unsigned char* dst, int nx, int pitch,
                               int row0, int nrows, int ny) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)nx * nrows) return;
  const int r = (int)(i / nx), x = (int)(i - (long)r * nx);
  int g = (row0 + r) % ny;
  if (g < 0) g += ny;
  dst[(long)r * pitch + x] = tile[(long)(g % tny) * tnx + (x % tnx)];
}

// number of blocked cells among n mask bytes (pitch padding is zero)
__global__ __launch_bounds__(256) void count_blocked(const unsigned char* mask, long n, unsigned long long* out) {
  __shared__ unsigned int sh[256];
  unsigned int acc = 0;
  const long base = ((long)blockIdx.x * 256 + threadIdx.x) * 16;
  for (int k = 0; k < 16; k++)
    if (base + k < n) acc += mask[base + k] ? 1u : 0u;
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && sh[0]) atomicAdd(out, (unsigned long long)sh[0]);
}

// uniform equilibrium start (SerialCode/d2q9-bgk.c:546-567)
__global__ void init_equilibrium(const LatticeArgs a, int rows, float r0, float r1, float r2) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (long)a.nx * rows) return;
  const long row = j / a.nx;
  const long ps = a.plane_stride;
  float* lat = a.dst + row * a.row_pitch + (j - row * a.nx);
  lat[0] = r0;
  lat[1 * ps] = r1;  lat[2 * ps] = r1;  lat[3 * ps] = r1;  lat[4 * ps] = r1;
  lat[5 * ps] = r2;  lat[6 * ps] = r2;  lat[7 * ps] = r2;  lat[8 * ps] = r2;
}

// AoS (reference host layout, 9 floats per cell) <-> SoA planes, rows [row0, row0+nrows)
__global__ void aos_to_soa(const float* aos, const LatticeArgs a, int row0, int nrows) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)a.nx * nrows * kQ;
  if (i >= n) return;
  const long cell = i / kQ;
  const int k = (int)(i - cell * kQ);
  const int r = (int)(cell / a.nx), x = (int)(cell - (long)r * a.nx);
  a.dst[k * a.plane_stride + (long)(row0 + r) * a.row_pitch + x] = aos[i];
}

__global__ void soa_to_aos(const LatticeArgs a, float* aos, int row0, int nrows) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)a.nx * nrows * kQ;
  if (i >= n) return;
  const long cell = i / kQ;
  const int k = (int)(i - cell * kQ);
  const int r = (int)(cell / a.nx), x = (int)(cell - (long)r * a.nx);
  aos[i] = a.src[k * a.plane_stride + (long)(row0 + r) * a.row_pitch + x];
}

// write_values() quantities (SerialCode/d2q9-bgk.c:684-719), always in the exact arithmetic
__global__ void final_state(const LatticeArgs a, int row0, int nrows, float density, float* ux_o, float* uy_o, float* um_o,
                            float* pr_o) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)a.nx * nrows;
  if (i >= n) return;
  const int r = (int)(i / a.nx), x = (int)(i - (long)r * a.nx);
  if (cell_blocked(a, row0 + r, x)) {
    ux_o[i] = 0.f;  uy_o[i] = 0.f;  um_o[i] = 0.f;
    pr_o[i] = density * kCsq;
  } else {
    float f[kQ];
    gather_cell(a, row0 + r, x, f);
    float rho, ux, uy;
    moments_exact(f, rho, ux, uy);
    ux_o[i] = ux;  uy_o[i] = uy;
    um_o[i] = sqrtf((ux * ux) + (uy * uy));
    pr_o[i] = rho * kCsq;
  }
}

// one animation frame of a stored lattice (lbm_set_frames, per-pass paths): final_state's |u| alone, into out[nrows][nx]
__global__ void frame_umag(const LatticeArgs a, int nrows, float* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)a.nx * nrows;
  if (i >= n) return;
  const int r = (int)(i / a.nx), x = (int)(i - (long)r * a.nx);
  if (cell_blocked(a, r, x)) {
    out[i] = 0.f;
  } else {
    float f[kQ];
    gather_cell(a, r, x, f);
    float rho, ux, uy;
    moments_exact(f, rho, ux, uy);
    out[i] = sqrtf((ux * ux) + (uy * uy));
  }
}

// one sample row of a stored lattice (lbm_set_probes, per-pass paths): final_state's four values at the slab's probed
// cells, one thread per probe, into row[probe index]
__global__ void probe_gather(const LatticeArgs a, float density, const ProbeEntry* table, int n, probe_vec* row) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const ProbeEntry e = table[i];
  const int x = (int)(e.xi & 0xfffffu);
  float f[kQ];
  gather_cell(a, e.row, x, f);
  row[e.xi >> 20] = probe_sample(f, cell_blocked(a, e.row, x), density);
}

// one sample of a stored lattice added to the mean fields (lbm_set_mean, per-pass paths): final_state's four values of
// every owned cell, each widened to double and added to the cell's sum in sums[j * plane + i], j = u_x, u_y, |u|, pressure;
// at order 2 also their exact products u_x u_x, u_y u_y, u_x u_y, pressure pressure to planes 4..7.
// One thread per cell, the only writer of its sums; plain loads and stores (the sums are read again at the next sample)
__global__ void mean_accumulate(const LatticeArgs a, int nrows, float density, double* sums, long plane, int order) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)a.nx * nrows;
  if (i >= n) return;
  const int r = (int)(i / a.nx), x = (int)(i - (long)r * a.nx);
  float f[kQ];
  gather_cell(a, r, x, f);
  const probe_vec v = probe_sample(f, cell_blocked(a, r, x), density);
#pragma unroll
  for (int j = 0; j < 4; j++) sums[j * plane + i] = sums[j * plane + i] + (double)v[j];
  if (order == 2) {
    const double ux = (double)v[0], uy = (double)v[1], pr = (double)v[3];
    const double prod[4] = {ux * ux, uy * uy, ux * uy, pr * pr};
#pragma unroll
    for (int j = 0; j < 4; j++) sums[(4 + j) * plane + i] = sums[(4 + j) * plane + i] + prod[j];
  }
}

// one field frame of a stored lattice (lbm_set_field_frames, per-pass paths): final_state's values of the slab's cells of
// the window -- columns [wx0, wx0 + wnx), slab rows [wy0, wy0 + wny) -- one thread per cell, the selected planes
// (bits of `fields`, ascending) into out[F][wny][wnx]
__global__ void field_frame(const LatticeArgs a, float density, int fields, int wx0, int wy0, int wnx, int wny, float* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)wnx * wny;
  if (i >= n) return;
  const int wr = (int)(i / wnx), wc = (int)(i - (long)wr * wnx);
  const int r = wy0 + wr, x = wx0 + wc;
  float f[kQ];
  gather_cell(a, r, x, f);
  const probe_vec v = probe_sample(f, cell_blocked(a, r, x), density);
  long at = i;
#pragma unroll
  for (int j = 0; j < 4; j++)
    if ((fields >> j) & 1) {
      out[at] = v[j];
      at += n;
    }
}

// av_velocity() of a stored lattice (SerialCode/d2q9-bgk.c:409-458): per-workgroup partials of
// sum |u| in double; reduced by reduce_doubles.  Also serves total_density() (:644-660).
__global__ __launch_bounds__(kBlock) void lattice_sums(const LatticeArgs a, int rows, double* speed_part, double* mass_part) {
  __shared__ double sh_s[kBlock], sh_m[kBlock];
  double s = 0.0, m = 0.0;
  const long n = (long)a.nx * rows;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long)gridDim.x * kBlock) {
    const int r = (int)(i / a.nx), x = (int)(i - (long)r * a.nx);
    float f[kQ];
    gather_cell(a, r, x, f);
    float rho, ux, uy;
    moments_exact(f, rho, ux, uy);
    m += (double)rho;
    if (!cell_blocked(a, r, x)) s += (double)sqrtf((ux * ux) + (uy * uy));
  }
  sh_s[threadIdx.x] = s;  sh_m[threadIdx.x] = m;
  __syncthreads();
  for (int k = kBlock / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) {
      sh_s[threadIdx.x] += sh_s[threadIdx.x + k];
      sh_m[threadIdx.x] += sh_m[threadIdx.x + k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    speed_part[blockIdx.x] = sh_s[0];
    mass_part[blockIdx.x] = sh_m[0];
  }
}

// ---------------------------------------------------------------------------------------------
// obstacle forces (lbm_set_forces): the boundary links of a slab, and the momentum they handed over
// ---------------------------------------------------------------------------------------------
// A boundary link is (b, k), k in 1..8, with b blocked and b + c_k (both periodic wraps) not.  After a timestep
// speeds[k] of b holds what arrived over that link and was turned round (SerialCode/d2q9-bgk.c, propagate + rebound):
// the solid received -2 c_k f.  The list of a slab holds the links of its owned blocked cells as cell * 8 + (k - 1),
// cell = row * nx + x slab-local, ordered by body, then cell, then k; starts[body] .. starts[body + 1] are a body's.
// It is built once at arming, in three launches over (kLinkCells cells per workgroup) x (bodies): link_count, link_scan,
// link_fill.  The neighbour rows of the slab's first and last row are the mask's halo rows.
constexpr int kLinkCells = 4 * kBlock;  // cells per workgroup of link_count / link_fill: four consecutive cells per lane
constexpr int kForceWords = 20;         // int64 words of a body in a ring row: F_x limbs 0..8, F_y limbs 9..17, 18 = terms
                                        // that were not finite, 19 unused
static_assert(2 * lbm_exact::kExactLimbs + 1 < kForceWords, "a body's words hold both accumulators and the count");

// c_k of the reference's numbering (SerialCode/d2q9-bgk.c:224-232): 1 E, 2 N, 3 W, 4 S, 5 NE, 6 NW, 7 SW, 8 SE
__device__ __forceinline__ int link_cx(int k) { return (int)((0x122u >> k) & 1u) - (int)((0x0c8u >> k) & 1u); }
__device__ __forceinline__ int link_cy(int k) { return (int)((0x064u >> k) & 1u) - (int)((0x190u >> k) & 1u); }

// bit k - 1 set: (cell, k) is a boundary link of body `body` (labels == nullptr: every blocked cell is body 0)
__device__ __forceinline__ unsigned link_bits(const unsigned char* mask, int pitch, int nx, const unsigned char* labels, int body,
                                              long cell) {
  const int row = (int)(cell / nx), x = (int)(cell - (long)row * nx);
  if (mask[(long)row * pitch + x] == 0) return 0u;
  if ((labels ? (int)labels[cell] : 0) != body) return 0u;
  unsigned bits = 0u;
#pragma unroll
  for (int k = 1; k < kQ; k++) {
    int xn = x + link_cx(k);
    xn = (xn < 0) ? nx - 1 : (xn == nx ? 0 : xn);
    if (mask[(long)(row + link_cy(k)) * pitch + xn] == 0) bits |= 1u << (k - 1);
  }
  return bits;
}

// *bad = the lowest owned cell that is blocked and labelled 255 (the host's mark for "outside 0 .. n_bodies - 1")
__global__ void label_check(const unsigned char* mask, int pitch, int nx, const unsigned char* labels, long n, unsigned* bad) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int row = (int)(i / nx), x = (int)(i - (long)row * nx);
  if (mask[(long)row * pitch + x] != 0 && labels[i] == 255) atomicMin(bad, (unsigned)i);
}

// the links of a lane's four cells; n = owned cells of the slab
__device__ __forceinline__ void lane_links(const unsigned char* mask, int pitch, int nx, const unsigned char* labels, long n,
                                           unsigned (&bits)[4], int& count) {
  const long cell0 = (long)blockIdx.x * kLinkCells + (long)threadIdx.x * 4;
  count = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    bits[i] = (cell0 + i < n) ? link_bits(mask, pitch, nx, labels, (int)blockIdx.y, cell0 + i) : 0u;
    count += __builtin_popcount(bits[i]);
  }
}

// the workgroup's exclusive prefix of v in lane order and its total (kBlock lanes; sh: one word per wave + 1)
__device__ __forceinline__ unsigned block_exclusive(unsigned v, unsigned* sh, unsigned& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned up = __shfl_up(inc, off, 64);
    if (lane >= off) inc += up;
  }
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  unsigned before = 0u, all = 0u;
  for (int w = 0; w < waves; w++) {
    const unsigned t = sh[w];
    if (w < wave) before += t;
    all += t;
  }
  __syncthreads();  // sh may be reused
  total = all;
  return before + inc - v;
}

// counts[body * gridDim.x + workgroup] = links of that body among the workgroup's cells
__global__ __launch_bounds__(kBlock) void link_count(const unsigned char* mask, int pitch, int nx, const unsigned char* labels, long n,
                                                     unsigned* counts) {
  __shared__ unsigned sh[kBlock / 64];
  unsigned bits[4];
  int count;
  lane_links(mask, pitch, nx, labels, n, bits, count);
  unsigned total;
  (void)block_exclusive((unsigned)count, sh, total);
  if (threadIdx.x == 0) counts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// one workgroup: counts[0 .. m) become their exclusive prefix sums (in place), starts[b] the prefix at b * per_body
// (b < m / per_body), starts[m / per_body] and *total the sum of all
__global__ __launch_bounds__(kBlock) void link_scan(unsigned* counts, long m, long per_body, unsigned* starts, unsigned long long* total) {
  __shared__ unsigned sh[kBlock / 64];
  unsigned long long carry = 0ull;
  for (long base = 0; base < m; base += kBlock) {
    const long i = base + threadIdx.x;
    const unsigned v = (i < m) ? counts[i] : 0u;
    unsigned chunk;
    const unsigned ex = block_exclusive(v, sh, chunk);
    if (i < m) {
      const unsigned at = (unsigned)carry + ex;
      counts[i] = at;
      if (i % per_body == 0) starts[i / per_body] = at;
    }
    carry += chunk;
  }
  if (threadIdx.x == 0) {
    starts[m / per_body] = (unsigned)carry;
    *total = carry;
  }
}

// links[offsets[body * gridDim.x + workgroup] ...] = the workgroup's links of that body, by cell, then k
__global__ __launch_bounds__(kBlock) void link_fill(const unsigned char* mask, int pitch, int nx, const unsigned char* labels, long n,
                                                    const unsigned* offsets, unsigned* links, unsigned n_links) {
  __shared__ unsigned sh[kBlock / 64];
  unsigned bits[4];
  int count;
  lane_links(mask, pitch, nx, labels, n, bits, count);
  unsigned total;
  unsigned at = offsets[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + block_exclusive((unsigned)count, sh, total);
  const long cell0 = (long)blockIdx.x * kLinkCells + (long)threadIdx.x * 4;
#pragma unroll
  for (int i = 0; i < 4; i++)
    for (unsigned b = bits[i]; b != 0u; b &= b - 1u) {
      if (at < n_links) links[at] = (unsigned)(cell0 + i) * 8u + (unsigned)__builtin_ctz(b);
      at++;
    }
}

// One sample of the forces on a stored lattice (per-pass and resident paths alike: launched behind the sub-call that
// ends at the sample step).  Workgroup (g, body): its lanes walk the body's links g * kBlock + lane, + gridDim.x * kBlock,
// ..., each adding -c_k f -- exactly, see lbm_exact_sum.h -- to its own pair of fixed-point accumulators; the pairs are
// added across the wave by shuffles, across the workgroup's waves through LDS, and across workgroups by 64-bit INTEGER
// atomics into the body's words of the ring row (zeroed by the host before the launch).  Every one of these additions
// is exact and commutes, so the row does not depend on scheduling; no floating-point addition happens on the device.
// The host rounds the sum once and doubles it (lbm_read_forces).
__global__ __launch_bounds__(kBlock) void force_gather(const LatticeArgs a, const unsigned* links, const unsigned* starts, long long* row) {
  constexpr int L = lbm_exact::kExactLimbs;
  __shared__ long long sh[kBlock / 64][2 * L + 1];
  const int body = blockIdx.y;
  const unsigned first = starts[body], end = starts[body + 1];
  if (first + (unsigned)blockIdx.x * kBlock >= end) return;  // (workgroup-uniform) nothing to add: the row keeps its zeros
  long long fx[L], fy[L], bad = 0;
#pragma unroll
  for (int i = 0; i < L; i++) fx[i] = fy[i] = 0;
  for (unsigned i = first + (unsigned)blockIdx.x * kBlock + threadIdx.x; i < end; i += gridDim.x * kBlock) {
    const unsigned e = links[i];
    const int k = (int)(e & 7u) + 1;
    const long cell = (long)(e >> 3);
    const int r = (int)(cell / a.nx), x = (int)(cell - (long)r * a.nx);
    const unsigned bits = __float_as_uint(a.src[k * a.plane_stride + (long)r * a.row_pitch + x]);
    if (lbm_exact::exact_sum_finite(bits)) {
      lbm_exact::exact_sum_add(fx, bits, -link_cx(k));
      lbm_exact::exact_sum_add(fy, bits, -link_cy(k));
    } else {
      bad++;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto wave_total = [&](long long v, int word) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) sh[wave][word] = v;
  };
#pragma unroll
  for (int i = 0; i < L; i++) {
    wave_total(fx[i], i);
    wave_total(fy[i], L + i);
  }
  wave_total(bad, 2 * L);
  __syncthreads();
  if (threadIdx.x < 2 * L + 1) {
    long long v = 0;
    for (int w = 0; w < kBlock / 64; w++) v += sh[w][threadIdx.x];
    if (v != 0) atomicAdd(reinterpret_cast<unsigned long long*>(row + (size_t)body * kForceWords + threadIdx.x), (unsigned long long)v);
  }
}

// a batch member's list of boundary links (lbm_batch_set_forces): built like a slab's, from the member's own mask and labels
struct ForceMember {
  const unsigned* links;
  const unsigned* starts;  // [bodies + 1]
};

// force_gather's twin for a batch: one sample of every member, in one launch behind the sub-call that ends at the sample
// step.  Workgroup (g, body, member) walks that member's links of that body on the member's current lattice
// (members[member].src; `a` carries the strides all members share) exactly as force_gather does, and adds into the
// member's and body's words of the row, [members][bodies][kForceWords] (zeroed by the host before the launch).  The
// x-extent of the grid suits the largest body of any member: a workgroup whose (member, body) has nothing left returns
// before the barrier, all of it.
__global__ __launch_bounds__(kBlock) void force_gather_batch(const LatticeArgs a, const ResidentMember* members, const ForceMember* lists,
                                                             long long* row) {
  constexpr int L = lbm_exact::kExactLimbs;
  __shared__ long long sh[kBlock / 64][2 * L + 1];
  const int body = blockIdx.y, member = blockIdx.z;
  const ForceMember list = lists[member];
  const unsigned first = list.starts[body], end = list.starts[body + 1];
  if (first + (unsigned)blockIdx.x * kBlock >= end) return;  // (workgroup-uniform) nothing to add: the words keep their zeros
  const float* src = members[member].src;
  long long fx[L], fy[L], bad = 0;
#pragma unroll
  for (int i = 0; i < L; i++) fx[i] = fy[i] = 0;
  for (unsigned i = first + (unsigned)blockIdx.x * kBlock + threadIdx.x; i < end; i += gridDim.x * kBlock) {
    const unsigned e = list.links[i];
    const int k = (int)(e & 7u) + 1;
    const long cell = (long)(e >> 3);
    const int r = (int)(cell / a.nx), x = (int)(cell - (long)r * a.nx);
    const unsigned bits = __float_as_uint(src[k * a.plane_stride + (long)r * a.row_pitch + x]);
    if (lbm_exact::exact_sum_finite(bits)) {
      lbm_exact::exact_sum_add(fx, bits, -link_cx(k));
      lbm_exact::exact_sum_add(fy, bits, -link_cy(k));
    } else {
      bad++;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto wave_total = [&](long long v, int word) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) sh[wave][word] = v;
  };
#pragma unroll
  for (int i = 0; i < L; i++) {
    wave_total(fx[i], i);
    wave_total(fy[i], L + i);
  }
  wave_total(bad, 2 * L);
  __syncthreads();
  if (threadIdx.x < 2 * L + 1) {
    long long v = 0;
    for (int w = 0; w < kBlock / 64; w++) v += sh[w][threadIdx.x];
    long long* words = row + ((size_t)member * gridDim.y + body) * kForceWords;
    if (v != 0) atomicAdd(reinterpret_cast<unsigned long long*>(words + threadIdx.x), (unsigned long long)v);
  }
}

// ---------------------------------------------------------------------------------------------
// lattice statistics (lbm_set_stats): exact mass, momentum and sum of |u|^2, the largest |u| and the cells that are
// not finite, of a whole stored lattice
// ---------------------------------------------------------------------------------------------
// One sample (launched behind the sub-call that ends at the sample step, like force_gather).  The owned cells are dealt
// out V at a time along x -- V = 4 where nx % 4 == 0: each of the nine planes is read with one 16-byte load per lane, the
// mask with one 4-byte load; V = 1 otherwise -- to the lanes of a capped grid, unit g * kBlock + lane, + gridDim.x * kBlock,
// ...: consecutive lanes read consecutive addresses of a row, and no unit reaches into the pitch padding (x + V <= nx).
// A lane keeps four fixed-point accumulators (rho, jx, jy, usq: lbm_exact_sum.h), its count of non-finite cells and its
// max key (lbm_stats_row.h); a cell that does not contribute is added with sign 0, so the lanes of a wave do not diverge.
// Per cell the arithmetic is final_state's (moments_exact, IEEE divide and sqrt, no contraction).  The lanes' values are
// combined across the wave by shuffles, across the waves through LDS, and across workgroups by 64-bit integer atomicAdd /
// atomicMax into `words` (kStatsWords of them, zeroed by the host before the launch): every combination is exact and
// commutes, so the words do not depend on scheduling or on the grid; no floating-point addition happens on the device.
constexpr int kStatsMaxGroups = 512;  // two workgroups per CU: a few thousand atomics per sample (words that stay 0 send none)

template <int V>
__device__ __forceinline__ void stats_cells(const LatticeArgs& a, const float* src, const unsigned char* mask, int rows, unsigned cell_first,
                                            long long* words) {
  constexpr int L = lbm_exact::kExactLimbs, S = lbm_stats::kStatsSums, W = lbm_stats::kStatsKeyWord + 1;
  __shared__ long long sh[kBlock / 64][W];
  long long acc[S][L], bad = 0;
  unsigned long long key = 0ull;
#pragma unroll
  for (int j = 0; j < S; j++)
#pragma unroll
    for (int i = 0; i < L; i++) acc[j][i] = 0;
  const long per_row = a.nx / V, n_units = (long)rows * per_row;
  for (long u = (long)blockIdx.x * kBlock + threadIdx.x; u < n_units; u += (long)gridDim.x * kBlock) {
    const int r = (int)(u / per_row), x = (int)(u - (long)r * per_row) * V;
    const float* p = src + (long)r * a.row_pitch + x;
    float f[V][kQ];
    unsigned blocked;  // byte v: the mask of cell x + v
    if constexpr (V == 4) {
#pragma unroll
      for (int k = 0; k < kQ; k++) {
        const float4 q = *reinterpret_cast<const float4*>(p + k * a.plane_stride);
        f[0][k] = q.x;  f[1][k] = q.y;  f[2][k] = q.z;  f[3][k] = q.w;
      }
      blocked = *reinterpret_cast<const unsigned*>(mask + (long)r * a.pitch + x);
    } else {
#pragma unroll
      for (int k = 0; k < kQ; k++) f[0][k] = p[k * a.plane_stride];
      blocked = mask[(long)r * a.pitch + x];
    }
    const unsigned cell = cell_first + (unsigned)r * (unsigned)a.nx + (unsigned)x;
#pragma unroll
    for (int v = 0; v < V; v++) {
      const float(&g)[kQ] = f[v];
      float rho, ux, uy;
      moments_exact(g, rho, ux, uy);
      const float jx = g[1] + g[5] + g[8] - (g[3] + g[6] + g[7]);
      const float jy = g[2] + g[5] + g[6] - (g[4] + g[7] + g[8]);
      const float usq = (ux * ux) + (uy * uy);
      const float umag = sqrtf(usq);
      const unsigned b_rho = __float_as_uint(rho), b_jx = __float_as_uint(jx), b_jy = __float_as_uint(jy), b_usq = __float_as_uint(usq);
      const bool fluid = ((blocked >> (8 * v)) & 0xffu) == 0u;
      const bool finite = lbm_exact::exact_sum_finite(b_rho) && (!fluid || (lbm_exact::exact_sum_finite(b_jx) && lbm_exact::exact_sum_finite(b_jy) &&
                                                                            lbm_exact::exact_sum_finite(b_usq)));
      const int s_all = finite ? 1 : 0, s_fluid = (finite && fluid) ? 1 : 0;
      lbm_exact::exact_sum_add(acc[0], b_rho, s_all);
      lbm_exact::exact_sum_add(acc[1], b_jx, s_fluid);
      lbm_exact::exact_sum_add(acc[2], b_jy, s_fluid);
      lbm_exact::exact_sum_add(acc[3], b_usq, s_fluid);
      bad += finite ? 0 : 1;
      const unsigned long long cell_key = lbm_stats::stats_key(__float_as_uint(umag), cell + (unsigned)v);
      key = (s_fluid && cell_key > key) ? cell_key : key;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto wave_total = [&](long long t, int word) {
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
    if (lane == 0) sh[wave][word] = t;
  };
#pragma unroll
  for (int j = 0; j < S; j++)
#pragma unroll
    for (int i = 0; i < L; i++) wave_total(acc[j][i], j * L + i);
  wave_total(bad, lbm_stats::kStatsBadWord);
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = (unsigned long long)__shfl_down((long long)key, off, 64);
    key = other > key ? other : key;
  }
  if (lane == 0) sh[wave][lbm_stats::kStatsKeyWord] = (long long)key;
  __syncthreads();
  if (threadIdx.x < W) {
    unsigned long long* word = reinterpret_cast<unsigned long long*>(words + threadIdx.x);
    if (threadIdx.x == lbm_stats::kStatsKeyWord) {
      unsigned long long m = 0ull;
      for (int w = 0; w < kBlock / 64; w++) m = (unsigned long long)sh[w][threadIdx.x] > m ? (unsigned long long)sh[w][threadIdx.x] : m;
      if (m != 0ull) atomicMax(word, m);
    } else {
      long long t = 0;
      for (int w = 0; w < kBlock / 64; w++) t += sh[w][threadIdx.x];
      if (t != 0) atomicAdd(word, (unsigned long long)t);
    }
  }
}

// a slab's owned rows into its words of the ring row; cell_first: the GLOBAL index of its first owned cell
template <int V>
__global__ __launch_bounds__(kBlock) void stats_gather(const LatticeArgs a, int rows, unsigned cell_first, long long* words) {
  stats_cells<V>(a, a.src, a.mask, rows, cell_first, words);
}

// stats_gather's twin for a batch: one sample of every member in one launch, workgroup (g, 0, member) on the member's
// current lattice and mask (members[member]; `a` carries the strides all members share), into the member's words of the
// row, [members][kStatsWords]
template <int V>
__global__ __launch_bounds__(kBlock) void stats_gather_batch(const LatticeArgs a, const ResidentMember* members, int rows, long long* row) {
  const int member = blockIdx.z;
  stats_cells<V>(a, members[member].src, members[member].mask, rows, 0u, row + (size_t)member * lbm_stats::kStatsWords);
}

// ---------------------------------------------------------------------------------------------
// velocity residuals (lbm_set_residual): the exact sums of |u - u_remembered|^2 and of |u|^2 over the finite fluid cells,
// the largest |u - u_remembered| with its cell and the fluid cells that are not finite, of a whole stored lattice
// ---------------------------------------------------------------------------------------------
// One sample, built the way stats_cells is: the same deal of the owned cells (V at a time along x, a capped grid that
// strides), the same reduction (shuffles, LDS, 64-bit integer atomics into `words`, kResidualWords of them, zeroed by
// the host; no floating-point addition on the device).  Besides the lattice a lane reads the remembered field of its
// cells from the dense planes px, py ([rows][nx]: a V = 4 unit is 16-byte aligned where nx % 4 == 0) and writes the
// current (u_x, u_y) back to them -- blocked cells 0, 0 -- with one 16-byte load and one 16-byte store per plane and unit.
// Each cell is read and written by one lane only, so there is no race.  A lane keeps two fixed-point accumulators (dsq,
// usq), its count and its key, stats_key(bits of dmag, global cell); a cell that does not contribute is added with sign
// 0.  BASELINE: the field is stored and nothing else happens (arming; `words` is not touched).
template <int V, bool BASELINE>
__device__ __forceinline__ void residual_cells(const LatticeArgs& a, const float* src, const unsigned char* mask, int rows, unsigned cell_first,
                                               float* px, float* py, long long* words) {
  constexpr int L = lbm_exact::kExactLimbs, S = lbm_residual::kResidualSums, W = lbm_residual::kResidualKeyWord + 1;
  long long acc[S][L], bad = 0;
  unsigned long long key = 0ull;
#pragma unroll
  for (int j = 0; j < S; j++)
#pragma unroll
    for (int i = 0; i < L; i++) acc[j][i] = 0;
  const long per_row = a.nx / V, n_units = (long)rows * per_row;
  for (long u = (long)blockIdx.x * kBlock + threadIdx.x; u < n_units; u += (long)gridDim.x * kBlock) {
    const int r = (int)(u / per_row), x = (int)(u - (long)r * per_row) * V;
    const float* p = src + (long)r * a.row_pitch + x;
    const long at = (long)r * a.nx + x;  // in the planes
    float f[V][kQ], pux[V], puy[V], nux[V], nuy[V];
    unsigned blocked;  // byte v: the mask of cell x + v
    if constexpr (V == 4) {
#pragma unroll
      for (int k = 0; k < kQ; k++) {
        const float4 q = *reinterpret_cast<const float4*>(p + k * a.plane_stride);
        f[0][k] = q.x;  f[1][k] = q.y;  f[2][k] = q.z;  f[3][k] = q.w;
      }
      blocked = *reinterpret_cast<const unsigned*>(mask + (long)r * a.pitch + x);
      if constexpr (!BASELINE) {
        const float4 qx = *reinterpret_cast<const float4*>(px + at), qy = *reinterpret_cast<const float4*>(py + at);
        pux[0] = qx.x;  pux[1] = qx.y;  pux[2] = qx.z;  pux[3] = qx.w;
        puy[0] = qy.x;  puy[1] = qy.y;  puy[2] = qy.z;  puy[3] = qy.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kQ; k++) f[0][k] = p[k * a.plane_stride];
      blocked = mask[(long)r * a.pitch + x];
      if constexpr (!BASELINE) {
        pux[0] = px[at];
        puy[0] = py[at];
      }
    }
    const unsigned cell = cell_first + (unsigned)r * (unsigned)a.nx + (unsigned)x;
#pragma unroll
    for (int v = 0; v < V; v++) {
      const float(&g)[kQ] = f[v];
      float rho, ux, uy;
      moments_exact(g, rho, ux, uy);
      const bool fluid = ((blocked >> (8 * v)) & 0xffu) == 0u;
      nux[v] = fluid ? ux : 0.f;
      nuy[v] = fluid ? uy : 0.f;
      if constexpr (!BASELINE) {
        const float jx = g[1] + g[5] + g[8] - (g[3] + g[6] + g[7]);
        const float jy = g[2] + g[5] + g[6] - (g[4] + g[7] + g[8]);
        const float usq = (ux * ux) + (uy * uy);
        const float dux = ux - pux[v], duy = uy - puy[v];
        const float dsq = (dux * dux) + (duy * duy);
        const float dmag = sqrtf(dsq);
        const unsigned b_usq = __float_as_uint(usq), b_dsq = __float_as_uint(dsq);
        const bool finite = lbm_exact::exact_sum_finite(__float_as_uint(rho)) && lbm_exact::exact_sum_finite(__float_as_uint(jx)) &&
                            lbm_exact::exact_sum_finite(__float_as_uint(jy)) && lbm_exact::exact_sum_finite(b_usq) &&
                            lbm_exact::exact_sum_finite(b_dsq);
        const int s = (finite && fluid) ? 1 : 0;
        lbm_exact::exact_sum_add(acc[0], b_dsq, s);
        lbm_exact::exact_sum_add(acc[1], b_usq, s);
        bad += (fluid && !finite) ? 1 : 0;
        const unsigned long long cell_key = lbm_stats::stats_key(__float_as_uint(dmag), cell + (unsigned)v);
        key = (s && cell_key > key) ? cell_key : key;
      }
    }
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(px + at) = make_float4(nux[0], nux[1], nux[2], nux[3]);
      *reinterpret_cast<float4*>(py + at) = make_float4(nuy[0], nuy[1], nuy[2], nuy[3]);
    } else {
      px[at] = nux[0];
      py[at] = nuy[0];
    }
  }
  if constexpr (!BASELINE) {
    __shared__ long long sh[kBlock / 64][W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto wave_total = [&](long long t, int word) {
      for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
      if (lane == 0) sh[wave][word] = t;
    };
#pragma unroll
    for (int j = 0; j < S; j++)
#pragma unroll
      for (int i = 0; i < L; i++) wave_total(acc[j][i], j * L + i);
    wave_total(bad, lbm_residual::kResidualBadWord);
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long other = (unsigned long long)__shfl_down((long long)key, off, 64);
      key = other > key ? other : key;
    }
    if (lane == 0) sh[wave][lbm_residual::kResidualKeyWord] = (long long)key;
    __syncthreads();
    if (threadIdx.x < W) {
      unsigned long long* word = reinterpret_cast<unsigned long long*>(words + threadIdx.x);
      if (threadIdx.x == lbm_residual::kResidualKeyWord) {
        unsigned long long m = 0ull;
        for (int w = 0; w < kBlock / 64; w++) m = (unsigned long long)sh[w][threadIdx.x] > m ? (unsigned long long)sh[w][threadIdx.x] : m;
        if (m != 0ull) atomicMax(word, m);
      } else {
        long long t = 0;
        for (int w = 0; w < kBlock / 64; w++) t += sh[w][threadIdx.x];
        if (t != 0) atomicAdd(word, (unsigned long long)t);
      }
    }
  }
}

// a slab's owned rows against its planes (px, py: [rows][nx]) into its words of the ring row; cell_first: the GLOBAL
// index of its first owned cell.  baseline != 0: the planes are filled and `words` is not read (arming)
template <int V>
__global__ __launch_bounds__(kBlock) void residual_gather(const LatticeArgs a, int rows, unsigned cell_first, float* px, float* py,
                                                          long long* words, int baseline) {
  if (baseline)
    residual_cells<V, true>(a, a.src, a.mask, rows, cell_first, px, py, words);
  else
    residual_cells<V, false>(a, a.src, a.mask, rows, cell_first, px, py, words);
}

// residual_gather's twin for a batch: one sample (or the baseline) of every member in one launch, workgroup (g, 0, member)
// on the member's current lattice and mask (members[member]; `a` carries the strides all members share), the member's
// planes -- planes[member][2][rows][nx] -- and the member's words of the row, [members][kResidualWords]
template <int V>
__global__ __launch_bounds__(kBlock) void residual_gather_batch(const LatticeArgs a, const ResidentMember* members, int rows, float* planes,
                                                                long long* row, int baseline) {
  const int member = blockIdx.z;
  const size_t n = (size_t)rows * a.nx;
  float* px = planes + (size_t)member * 2 * n;
  if (baseline)
    residual_cells<V, true>(a, members[member].src, members[member].mask, rows, 0u, px, px + n, row);
  else
    residual_cells<V, false>(a, members[member].src, members[member].mask, rows, 0u, px, px + n,
                             row + (size_t)member * lbm_residual::kResidualWords);
}

// ---------------------------------------------------------------------------------------------
// residual-steady runs (lbm_run_until_residual): a sample of the residuals after every segment, judged on the device
// ---------------------------------------------------------------------------------------------
// residual_gather's sample for a segment that was enqueued before the verdict of the segment in front of it was known:
// once that verdict is "stop" (gate->stop: the word accelerate_row_unless reads) neither the words nor the remembered
// field move.  The words are not zeroed by the host: residual_check leaves them zero behind every sample it has read.
template <int V>
__global__ __launch_bounds__(kBlock) void residual_gather_unless(const LatticeArgs a, int rows, unsigned cell_first, float* px, float* py,
                                                                 long long* words, const SteadyState* gate) {
  if (gate->stop) return;  // one scalar load, uniform over the grid
  residual_cells<V, false>(a, a.src, a.mask, rows, cell_first, px, py, words);
}

__global__ void residual_until_reset(lbm_residual::UntilState* st, long long* words, int n, SteadyBatch* batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    lbm_residual::until_reset(st[i]);
    for (int k = 0; k < lbm_residual::kResidualWords; k++) words[(size_t)i * lbm_residual::kResidualWords + k] = 0;
  }
  if (i == 0 && batch) *batch = SteadyBatch{0, 0};
}

// One wave and one lattice: lanes 0 and 1 round the two sums (lbm_residual_until.h: exact_sum_round_hd), lane 0 takes
// the verdict (until_verdict), the first kResidualWords lanes copy the words into the history row (hist: NULL beyond the
// capacity) and leave them zero for the next sample.  FROZEN_ROWS: a lattice whose verdict stands still hands its words
// on (a batch member steps on with the others, and its later rows are real rows); without it nothing at all happens
// after a stop, which is what a dropped look-ahead segment needs.  Returns the stop word this check set (lane 0).
template <bool FROZEN_ROWS>
__device__ __forceinline__ int residual_check_at(long long* words, long long* hist, double tol, int patience, int steps_after,
                                                 lbm_residual::UntilState* st) {
  const bool stopped = st->stop != lbm_residual::kUntilGoOn;  // uniform
  if (stopped && !FROZEN_ROWS) return lbm_residual::kUntilGoOn;
  const int lane = threadIdx.x;
  int code = lbm_residual::kUntilGoOn;
  if (!stopped) {
    double sum = 0.0;
    if (lane < lbm_residual::kResidualSums) sum = lbm_residual::exact_sum_round_hd(words + lane * lbm_exact::kExactLimbs);
    const double sum_u_sq = __shfl(sum, 1, 64);
    if (lane == 0) code = lbm_residual::until_verdict(*st, words, sum, sum_u_sq, tol, patience, steps_after);
  }
  long long w = 0;
  if (lane < lbm_residual::kResidualWords) {
    w = words[lane];
    if (hist) hist[lane] = w;
  }
  __syncthreads();  // lane 0 has read the words (until_verdict keeps them) before they are cleared
  if (lane < lbm_residual::kResidualWords) words[lane] = 0;
  return code;
}
// gate->stop takes the stop word: the look-ahead segment's accelerate_row_unless and residual_gather_unless read it, and
// it is what travels back to the host
__global__ __launch_bounds__(64) void residual_check(long long* words, long long* hist, double tol, int patience, int steps_after,
                                                     lbm_residual::UntilState* st, SteadyState* gate) {
  const int code = residual_check_at<false>(words, hist, tol, patience, steps_after, st);
  if (threadIdx.x == 0 && code != lbm_residual::kUntilGoOn) gate->stop = code;
}
// every member of a batch at once, one wave per member: grid (members); words and hist are [members][kResidualWords].
// The member that completes the set of finished (steady or diverged) members raises all_steady, as in steady_check_batch.
__global__ __launch_bounds__(64) void residual_check_batch(long long* words, long long* hist, int n_members, double tol, int patience,
                                                           int steps_after, lbm_residual::UntilState* st, SteadyBatch* batch) {
  const size_t at = (size_t)blockIdx.x * lbm_residual::kResidualWords;
  const int code = residual_check_at<true>(words + at, hist ? hist + at : nullptr, tol, patience, steps_after, st + blockIdx.x);
  if (threadIdx.x == 0 && code != lbm_residual::kUntilGoOn) {
    const int before = __hip_atomic_fetch_add(&batch->n_steady, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (before + 1 == n_members) __hip_atomic_store(&batch->all_steady, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------------------------
// line profiles (lbm_set_profiles): per row and per column the exact sums of rho, jx, jy, ux, uy over the line's finite
// fluid cells, their number and the number of fluid cells that are not finite, of a whole stored lattice
// ---------------------------------------------------------------------------------------------
// One sample is one launch per selected axis (behind the sub-call that ends at the sample step, like stats_gather), into
// the record's lines of kProfileWords words each (lbm_profile_row.h), zeroed by the host before the launches.  The two
// axes reduce in different directions, so a lane owns different things in each: in profile_rows a wave owns a row and its
// lanes stride along it; in profile_columns a lane owns a column and walks down it.  Both keep five fixed-point
// accumulators per lane (lbm_exact_sum.h) and two counts; a cell that does not contribute (blocked or not finite) is
// added with sign 0, so the lanes of a wave do not diverge.  Per cell the arithmetic is the statistics' (moments_exact,
// IEEE divide, no contraction).  Every combination is an integer add: the words do not depend on the grid or on
// scheduling, and no floating-point addition happens on the device.
constexpr int kProfileColumns = 64;  // profile_columns: columns of a workgroup (one per lane of a wave; its waves share them)
constexpr int kProfileMinBand = 8;   // ... and the fewest rows of a band: two per wave

// one cell into a lane's accumulators
__device__ __forceinline__ void profile_cell(const float (&g)[kQ], bool fluid, long long (&acc)[lbm_profile::kProfileSums][lbm_exact::kExactLimbs],
                                             int& n_fluid, int& n_bad) {
  float rho, ux, uy;
  moments_exact(g, rho, ux, uy);
  const float jx = g[1] + g[5] + g[8] - (g[3] + g[6] + g[7]);
  const float jy = g[2] + g[5] + g[6] - (g[4] + g[7] + g[8]);
  const float usq = (ux * ux) + (uy * uy);
  const unsigned b_rho = __float_as_uint(rho), b_jx = __float_as_uint(jx), b_jy = __float_as_uint(jy);
  const bool finite = lbm_exact::exact_sum_finite(b_rho) && lbm_exact::exact_sum_finite(b_jx) && lbm_exact::exact_sum_finite(b_jy) &&
                      lbm_exact::exact_sum_finite(__float_as_uint(usq));
  const int s = (fluid && finite) ? 1 : 0;
  lbm_exact::exact_sum_add(acc[0], b_rho, s);
  lbm_exact::exact_sum_add(acc[1], b_jx, s);
  lbm_exact::exact_sum_add(acc[2], b_jy, s);
  lbm_exact::exact_sum_add(acc[3], __float_as_uint(ux), s);  // (usq finite: ux and uy are)
  lbm_exact::exact_sum_add(acc[4], __float_as_uint(uy), s);
  n_fluid += s;
  n_bad += (fluid && !finite) ? 1 : 0;
}

// Sums along x.  Wave w of workgroup g owns the owned row g * (kBlock / 64) + w; its lanes take the units lane, lane + 64,
// ... of the row, a unit being V cells: V = 4 where nx % 4 == 0 (one 16-byte load per plane and lane, the mask with one
// 4-byte load), else V = 1; no unit reaches into the pitch padding (x + V <= nx).  The accumulators are lane-private; one
// butterfly of shuffles per word totals them across the wave, lane i keeps word i, and lanes 0 .. 46 store the line.
// Nothing else writes a row line: no atomics.
template <int V>
__device__ __forceinline__ void profile_row_lines(const LatticeArgs& a, const float* src, const unsigned char* mask, int rows, long long* lines) {
  constexpr int L = lbm_exact::kExactLimbs, S = lbm_profile::kProfileSums;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;  // uniform over the wave
  long long acc[S][L];
  int n_fluid = 0, n_bad = 0;
#pragma unroll
  for (int j = 0; j < S; j++)
#pragma unroll
    for (int i = 0; i < L; i++) acc[j][i] = 0;
  const int per_row = a.nx / V;
#pragma unroll 1
  for (int u = lane; u < per_row; u += 64) {
    const int x = u * V;
    const float* p = src + (long)r * a.row_pitch + x;
    float f[V][kQ];
    unsigned blocked;  // byte v: the mask of cell x + v
    if constexpr (V == 4) {
#pragma unroll
      for (int k = 0; k < kQ; k++) {
        const float4 q = *reinterpret_cast<const float4*>(p + k * a.plane_stride);
        f[0][k] = q.x;  f[1][k] = q.y;  f[2][k] = q.z;  f[3][k] = q.w;
      }
      blocked = *reinterpret_cast<const unsigned*>(mask + (long)r * a.pitch + x);
    } else {
#pragma unroll
      for (int k = 0; k < kQ; k++) f[0][k] = p[k * a.plane_stride];
      blocked = mask[(long)r * a.pitch + x];
    }
#pragma unroll
    for (int v = 0; v < V; v++) profile_cell(f[v], ((blocked >> (8 * v)) & 0xffu) == 0u, acc, n_fluid, n_bad);
  }
  long long mine = 0;
  auto wave_total = [&](long long t, int word) {
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    mine = (lane == word) ? t : mine;
  };
#pragma unroll
  for (int j = 0; j < S; j++)
#pragma unroll
    for (int i = 0; i < L; i++) wave_total(acc[j][i], j * L + i);
  wave_total((long long)n_fluid, lbm_profile::kProfileFluidWord);
  wave_total((long long)n_bad, lbm_profile::kProfileBadWord);
  if (lane <= lbm_profile::kProfileBadWord) lines[(size_t)r * lbm_profile::kProfileWords + lane] = mine;
}

// a slab's owned rows into its row lines of the record, [rows][kProfileWords]; grid: ceil(rows / (kBlock / 64))
template <int V>
__global__ __launch_bounds__(kBlock) void profile_rows(const LatticeArgs a, int rows, long long* lines) {
  profile_row_lines<V>(a, a.src, a.mask, rows, lines);
}

// profile_rows' twin for a batch: workgroup (g, 0, member) on the member's current lattice and mask (members[member];
// `a` carries the strides all members share), into the member's lines, member_words words apart
template <int V>
__global__ __launch_bounds__(kBlock) void profile_rows_batch(const LatticeArgs a, const ResidentMember* members, int rows, long long* lines,
                                                             long member_words) {
  const int member = blockIdx.z;
  profile_row_lines<V>(a, members[member].src, members[member].mask, rows, lines + (size_t)member * member_words);
}

// Sums along y.  Workgroup (g, b) owns the columns [g * kProfileColumns, + kProfileColumns) of the rows of band b,
// [b * band_rows, + band_rows): lane l of every wave owns column g * kProfileColumns + l -- consecutive lanes read
// consecutive addresses of a row -- and wave w walks the band's rows w, w + kBlock / 64, ...  The waves of a workgroup
// combine through LDS (integer atomics on words that start from zero), then the workgroup's lanes walk its
// kProfileColumns lines word by word -- consecutive lanes, consecutive addresses -- and send every word that is not 0 by
// one 64-bit atomicAdd into the column's words, where the bands meet.
__device__ __forceinline__ void profile_column_lines(const LatticeArgs& a, const float* src, const unsigned char* mask, int rows, int band_rows,
                                                     long long* lines) {
  constexpr int L = lbm_exact::kExactLimbs, S = lbm_profile::kProfileSums, W = lbm_profile::kProfileWords;
  __shared__ unsigned long long sh[kProfileColumns * W];  // [column][word], 24 KiB
  for (int i = threadIdx.x; i < kProfileColumns * W; i += kBlock) sh[i] = 0ull;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = (int)blockIdx.x * kProfileColumns, x = x0 + lane;
  const int r0 = (int)blockIdx.y * band_rows, r1 = (r0 + band_rows < rows) ? r0 + band_rows : rows;
  long long acc[S][L];
  int n_fluid = 0, n_bad = 0;
#pragma unroll
  for (int j = 0; j < S; j++)
#pragma unroll
    for (int i = 0; i < L; i++) acc[j][i] = 0;
  if (x < a.nx) {
    for (int r = r0 + wave; r < r1; r += kBlock / 64) {
      const float* p = src + (long)r * a.row_pitch + x;
      float f[kQ];
#pragma unroll
      for (int k = 0; k < kQ; k++) f[k] = p[k * a.plane_stride];
      profile_cell(f, mask[(long)r * a.pitch + x] == 0, acc, n_fluid, n_bad);
    }
  }
  __syncthreads();
  unsigned long long* mine = sh + lane * W;
#pragma unroll
  for (int j = 0; j < S; j++)
#pragma unroll
    for (int i = 0; i < L; i++)
      if (acc[j][i] != 0) atomicAdd(mine + j * L + i, (unsigned long long)acc[j][i]);
  if (n_fluid != 0) atomicAdd(mine + lbm_profile::kProfileFluidWord, (unsigned long long)n_fluid);
  if (n_bad != 0) atomicAdd(mine + lbm_profile::kProfileBadWord, (unsigned long long)n_bad);
  __syncthreads();
  const int columns = (a.nx - x0 < kProfileColumns) ? a.nx - x0 : kProfileColumns;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(lines) + (size_t)x0 * W;
  for (int i = threadIdx.x; i < columns * W; i += kBlock) {
    const unsigned long long t = sh[i];
    if (t != 0ull) atomicAdd(out + i, t);
  }
}

// a slab's owned rows into its column lines of the record, [nx][kProfileWords]; grid: (ceil(nx / kProfileColumns), bands)
__global__ __launch_bounds__(kBlock) void profile_columns(const LatticeArgs a, int rows, int band_rows, long long* lines) {
  profile_column_lines(a, a.src, a.mask, rows, band_rows, lines);
}

// profile_columns' twin for a batch: workgroup (g, b, member), as profile_rows_batch
__global__ __launch_bounds__(kBlock) void profile_columns_batch(const LatticeArgs a, const ResidentMember* members, int rows, int band_rows,
                                                                long long* lines, long member_words) {
  const int member = blockIdx.z;
  profile_column_lines(a, members[member].src, members[member].mask, rows, band_rows, lines + (size_t)member * member_words);
}

// ---------------------------------------------------------------------------------------------
// coarse frames (lbm_set_coarse_frames, lbm_read_coarse): per box of bx x by cells what a line profile holds per line --
// the exact sums of rho, jx, jy, ux, uy over the box's finite fluid cells and the two counts -- of a whole stored lattice
// ---------------------------------------------------------------------------------------------
// One sample is one launch per slab (behind the sub-call that ends at the sample step, like the profiles), over the box
// rows that touch the slab (lbm_coarse_row.h: SlabBoxRows).  As in profile_columns a lane owns a column -- consecutive
// lanes read consecutive addresses of a row -- and walks down it, here the rows of its box row that the slab owns, at most
// LBM_COARSE_MAX_BOX of them, with profile_cell unchanged: five fixed-point accumulators and two counts per lane, a cell
// that does not count added with sign 0.  The host picks one of two forms by bx:
//   WIDE = false, bx <= 64: a wave owns a span of floor(64 / bx) whole boxes of one box row, lane l column l of the span;
//     the lanes past the span's last box idle.  Workgroup g of a box row takes the spans 4 g .. 4 g + 3.  A box's lanes
//     are totalled by a segmented reduction of shuffles -- offsets 1, 2, 4, ... below bx, a lane adds only what comes
//     from a lane of its own box -- which leaves the box's total in its first lane, the head.  No LDS, no atomics.
//   WIDE = true, 64 < bx <= 256: a workgroup owns one box, thread t < the box's width its column t.  A butterfly totals
//     every word over the wave (as in profile_rows), lane i keeps word i, and the four waves meet in 48 words of LDS.
// A box of a WHOLE box row is rounded here (exact_sum_round_hd: five roundings per box) and leaves as its 48-byte
// line; a box of a PARTIAL box row leaves as its 47 limb and count words, stored plainly into the slot's seam area, whose
// spare word the host has zeroed.  Every box has exactly one writer per slab: no global atomics, and no floating-point
// addition happens on the device.
template <bool WIDE>
__device__ __forceinline__ void coarse_box_lines(const LatticeArgs& a, const float* src, const unsigned char* mask,
                                                 const lbm_coarse::SlabBoxRows& g, int groups, long long* words) {
  constexpr int L = lbm_exact::kExactLimbs, S = lbm_profile::kProfileSums, W = lbm_profile::kProfileWords;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Y = g.first + (int)(blockIdx.x / (unsigned)groups), gx = (int)(blockIdx.x % (unsigned)groups);
  // the slab's rows of box row Y, as rows of the slab
  const int y0 = lbm_coarse::box_row_begin(g, Y), y1 = lbm_coarse::box_row_end(g, Y);
  const int r0 = (y0 > g.row_first ? y0 : g.row_first) - g.row_first;
  const int r1 = (y1 < g.row_first + g.rows ? y1 : g.row_first + g.rows) - g.row_first;
  int X, x;       // this lane's box and column
  bool active;    // the lane owns a column of the grid
  bool head;      // ... the first of its box
  if constexpr (WIDE) {
    X = gx;
    x = X * g.bx + (int)threadIdx.x;
    active = (int)threadIdx.x < g.bx && x < a.nx;
    head = threadIdx.x == 0;
  } else {
    const int per_wave = 64 / g.bx;  // boxes of a span
    const int in_span = lane / g.bx;
    X = (gx * (kBlock / 64) + wave) * per_wave + in_span;
    x = (gx * (kBlock / 64) + wave) * per_wave * g.bx + lane;
    active = in_span < per_wave && x < a.nx;
    head = active && lane == in_span * g.bx;
  }
  long long acc[S][L];
  int n_fluid = 0, n_bad = 0;
#pragma unroll
  for (int j = 0; j < S; j++)
#pragma unroll
    for (int i = 0; i < L; i++) acc[j][i] = 0;
  if (active) {
#pragma unroll 1
    for (int r = r0; r < r1; r++) {
      const float* p = src + (long)r * a.row_pitch + x;
      float f[kQ];
#pragma unroll
      for (int k = 0; k < kQ; k++) f[k] = p[k * a.plane_stride];
      profile_cell(f, mask[(long)r * a.pitch + x] == 0, acc, n_fluid, n_bad);
    }
  }
  bool whole;
  if constexpr (WIDE) {
    __shared__ unsigned long long sh[W];
    if (threadIdx.x < W) sh[threadIdx.x] = 0ull;
    long long mine = 0;
    auto wave_total = [&](long long t, int word) {
      for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
      mine = (lane == word) ? t : mine;
    };
#pragma unroll
    for (int j = 0; j < S; j++)
#pragma unroll
      for (int i = 0; i < L; i++) wave_total(acc[j][i], j * L + i);
    wave_total((long long)n_fluid, lbm_profile::kProfileFluidWord);
    wave_total((long long)n_bad, lbm_profile::kProfileBadWord);
    __syncthreads();
    if (lane <= lbm_profile::kProfileBadWord && mine != 0) atomicAdd(sh + lane, (unsigned long long)mine);
    __syncthreads();
    long long* out = words + lbm_coarse::box_offset(g, X, Y, &whole);
    if (whole) {  // threads 0 .. 4 round a sum each, thread 5 packs the counts
      if (threadIdx.x < S) {
        long long limbs[L];
#pragma unroll
        for (int i = 0; i < L; i++) limbs[i] = (long long)sh[threadIdx.x * L + i];
        out[threadIdx.x] = __double_as_longlong(lbm_exact::exact_sum_round_hd(limbs));
      } else if (threadIdx.x == S) {
        out[S] = (long long)((sh[lbm_profile::kProfileBadWord] << 32) | (sh[lbm_profile::kProfileFluidWord] & 0xffffffffull));
      }
    } else if (threadIdx.x <= lbm_profile::kProfileBadWord) {
      out[threadIdx.x] = (long long)sh[threadIdx.x];
    }
  } else {
    // the segmented reduction: after the step of offset `off` a lane holds the sum of its box's lanes [lane, lane + 2 off)
    const int box_end = (lane / g.bx + 1) * g.bx;  // one past the box's last lane
    for (int off = 1; off < g.bx; off <<= 1) {
      const bool take = lane + off < box_end;  // (a box's lanes lie in one wave: box_end <= 64 for every lane that counts)
#pragma unroll
      for (int j = 0; j < S; j++)
#pragma unroll
        for (int i = 0; i < L; i++) {
          const long long t = __shfl_down(acc[j][i], off, 64);
          acc[j][i] += take ? t : 0LL;
        }
      const int tf = __shfl_down(n_fluid, off, 64), tb = __shfl_down(n_bad, off, 64);
      n_fluid += take ? tf : 0;
      n_bad += take ? tb : 0;
    }
    if (head) {
      long long* out = words + lbm_coarse::box_offset(g, X, Y, &whole);
      if (whole) {
        long long line[lbm_coarse::kCoarseLineWords];
        lbm_coarse::line_words_from_sums(acc, n_fluid, n_bad, line);
#pragma unroll
        for (int i = 0; i < lbm_coarse::kCoarseLineWords; i++) out[i] = line[i];
      } else {
#pragma unroll
        for (int j = 0; j < S; j++)
#pragma unroll
          for (int i = 0; i < L; i++) out[j * L + i] = acc[j][i];
        out[lbm_profile::kProfileFluidWord] = (long long)n_fluid;
        out[lbm_profile::kProfileBadWord] = (long long)n_bad;
      }
    }
  }
}

// a slab's share of one coarse frame into its slot; grid: (box rows that touch the slab) * groups workgroups, box row
// major, where groups = the workgroups of one box row: cx if WIDE, else ceil(ceil(cx / floor(64 / bx)) / 4)
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void coarse_gather(const LatticeArgs a, const lbm_coarse::SlabBoxRows g, int groups, long long* words) {
  coarse_box_lines<WIDE>(a, a.src, a.mask, g, groups, words);
}

// coarse_gather's twin for a batch: workgroup (., 0, member) on the member's current lattice and mask (members[member];
// `a` carries the strides all members share), into the member's slot, member_words words apart
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void coarse_gather_batch(const LatticeArgs a, const ResidentMember* members, const lbm_coarse::SlabBoxRows g,
                                                              int groups, long long* words, long member_words) {
  const int member = blockIdx.z;
  coarse_box_lines<WIDE>(a, members[member].src, members[member].mask, g, groups, words + (size_t)member * member_words);
}

// ---------------------------------------------------------------------------------------------
// vorticity and enstrophy (lbm_read_vorticity, lbm_set_enstrophy): w = 0.5f * ((uy(x+1) - uy(x-1)) - (ux(y+1) - ux(y-1)))
// of every fluid cell of a stored lattice, as a field and / or as the exact sums of w * w and w, the largest |w| with its
// cell and the counts of a row (lbm_enstrophy_row.h)
// ---------------------------------------------------------------------------------------------
// The first gather that reads a cell's neighbours.  A wave owns a unit: a strip of 64 * V columns -- V = 4 where
// nx % 4 == 0: each of the nine planes is read with one 16-byte load per lane, the mask with one 4-byte load; V = 1
// otherwise; no lane reaches into the pitch padding (x + V <= nx, the other lanes load nothing) -- of a band of rows
// [r0, r1).  It sweeps the rows r0 - 1 .. r1, computes (ux, uy) of its cells once per row (moments_exact, blocked: 0, 0)
// and carries the three-row window in registers: a lattice row is read once per band, plus the two rows around the band.
// The x neighbours inside the strip come from the adjacent lanes (shuffles); the two cells just outside it, x0 - 1 and
// the cell behind the last VALID lane, both wrapped modulo nx, are gathered per owned row by lane 0 and by the last valid
// lane as scalar nine-plane loads -- so a strip narrower than the wave (the ragged last strip, nx < 64 * V) takes cell 0's
// velocity for the right neighbour of its last cell, not the next lane's.
// Row -1 of a slab is `south`, row `rows` is `north`: each one whole lattice row (nine planes, plane_stride apart).  A
// single periodic slab and a batch member pass their own rows rows - 1 and 0; a slab among several passes its edge
// buffer, filled by the host from the neighbours' boundary rows -- the lattice halo rows are not read.  The mask rows -1
// and `rows` are the mask's own halo rows.
// The reduction is stats_cells': a cell that does not contribute is added with sign 0, the lanes are combined by
// shuffles, the waves through LDS, the workgroups by 64-bit integer atomicAdd / atomicMax into `words`
// (kEnstrophyWords, zeroed by the host before the launch; words that stayed 0 send nothing): no floating-point addition
// happens on the device, and the words do not depend on the grid, the bands or scheduling.
// Either of `field` (dense, row row_begin first, nx floats per row) and `words` may be null.  FIELD = false is the form
// that never stores a field (`field` is not read): the recorder's; without the store's addresses it keeps two waves per
// SIMD where the other form keeps one.
constexpr int kVortMaxGroups = 512;   // two workgroups per CU; the waves stride over the units beyond
constexpr int kVortMinBand = 8;       // the fewest rows of a band: at most 10 rows read for 8

// uy of the cell x of a lattice row as lbm_read_final_state reports it: blocked -> 0
__device__ __forceinline__ float vorticity_edge_uy(const float* row, const unsigned char* mrow, long plane_stride, int x) {
  float f[kQ], rho, ux, uy;
#pragma unroll
  for (int k = 0; k < kQ; k++) f[k] = row[k * plane_stride + x];
  moments_exact(f, rho, ux, uy);
  return mrow[x] != 0 ? 0.f : uy;
}

template <int V, bool FIELD>
__device__ __forceinline__ void vorticity_cells(const LatticeArgs& a, const float* src, const unsigned char* mask, const float* south,
                                                const float* north, int rows, int row_begin, int row_end, int band_rows, unsigned cell_first,
                                                float* field, long long* words) {
  constexpr int L = lbm_exact::kExactLimbs, S = lbm_enstrophy::kEnstrophySums, W = lbm_enstrophy::kEnstrophyKeyWord + 1;
  constexpr int kWaves = kBlock / 64, kSpan = 64 * V;
  __shared__ long long sh[kWaves][W];
  long long acc[S][L], bad = 0, n_fluid = 0;
  unsigned long long key = 0ull;
#pragma unroll
  for (int j = 0; j < S; j++)
#pragma unroll
    for (int i = 0; i < L; i++) acc[j][i] = 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int strips = (a.nx + kSpan - 1) / kSpan;
  const int bands = (row_end - row_begin + band_rows - 1) / band_rows;
  const long n_units = (long)strips * bands;
  for (long u = (long)blockIdx.x * kWaves + wave; u < n_units; u += (long)gridDim.x * kWaves) {  // (uniform over the wave)
    const int band = (int)(u / strips), strip = (int)(u - (long)band * strips);
    const int x0 = strip * kSpan, x = x0 + lane * V;
    const bool valid = x < a.nx;  // (V == 4: nx % 4 == 0, so x + V <= nx)
    const int n_valid = (a.nx - x0) / V < 64 ? (a.nx - x0) / V : 64;  // lanes of this strip with cells: 1 .. 64
    const int last = n_valid - 1;
    const int xl = x0 == 0 ? a.nx - 1 : x0 - 1;                        // the cell before the strip ...
    const int xr = x0 + n_valid * V >= a.nx ? 0 : x0 + n_valid * V;    // ... and behind its last valid lane, both wrapped
    const int r0 = row_begin + band * band_rows, r1 = (r0 + band_rows < row_end) ? r0 + band_rows : row_end;
    // the window: ux of row rr - 2 (ux_a); ux, dvdx and the flags of row rr - 1 (_b); row rr is loaded (_c)
    float ux_a[V], ux_b[V], dvdx_b[V];
    unsigned fluid_b = 0u, fin_b = 0u;  // bit v: cell x + v is fluid / its own rho, jx, jy, usq are finite
#pragma unroll
    for (int v = 0; v < V; v++) ux_a[v] = ux_b[v] = dvdx_b[v] = 0.f;
#pragma unroll 1
    for (int rr = r0 - 1; rr <= r1; rr++) {
      const float* row = rr < 0 ? south : (rr >= rows ? north : src + (long)rr * a.row_pitch);
      const unsigned char* mrow = mask + (long)rr * a.pitch;
      float f[V][kQ];
      unsigned blocked = 0x01010101u;  // byte v: the mask of cell x + v; a lane without cells: blocked
#pragma unroll
      for (int v = 0; v < V; v++)
#pragma unroll
        for (int k = 0; k < kQ; k++) f[v][k] = 0.f;
      if (valid) {
        const float* p = row + x;
        if constexpr (V == 4) {
#pragma unroll
          for (int k = 0; k < kQ; k++) {
            const float4 q = *reinterpret_cast<const float4*>(p + k * a.plane_stride);
            f[0][k] = q.x;  f[1][k] = q.y;  f[2][k] = q.z;  f[3][k] = q.w;
          }
          blocked = *reinterpret_cast<const unsigned*>(mrow + x);
        } else {
#pragma unroll
          for (int k = 0; k < kQ; k++) f[0][k] = p[k * a.plane_stride];
          blocked = mrow[x];
        }
      }
      float ux_c[V], uy_c[V], dvdx_c[V];
      unsigned fluid_c = 0u, fin_c = 0u;
#pragma unroll
      for (int v = 0; v < V; v++) {
        const float(&g)[kQ] = f[v];
        float rho, ux, uy;
        moments_exact(g, rho, ux, uy);
        const float jx = g[1] + g[5] + g[8] - (g[3] + g[6] + g[7]);
        const float jy = g[2] + g[5] + g[6] - (g[4] + g[7] + g[8]);
        const float usq = (ux * ux) + (uy * uy);
        const bool fluid = ((blocked >> (8 * v)) & 0xffu) == 0u;
        const bool finite = lbm_exact::exact_sum_finite(__float_as_uint(rho)) && lbm_exact::exact_sum_finite(__float_as_uint(jx)) &&
                            lbm_exact::exact_sum_finite(__float_as_uint(jy)) && lbm_exact::exact_sum_finite(__float_as_uint(usq));
        ux_c[v] = fluid ? ux : 0.f;
        uy_c[v] = fluid ? uy : 0.f;
        fluid_c |= (fluid ? 1u : 0u) << v;
        fin_c |= (finite ? 1u : 0u) << v;
        dvdx_c[v] = 0.f;
      }
      if (rr >= r0 && rr < r1) {  // (uniform) an owned row: its x differences; the rows around the band give ux alone
        float west = __shfl_up(uy_c[V - 1], 1, 64), east = __shfl_down(uy_c[0], 1, 64);
        if (lane == 0) west = vorticity_edge_uy(row, mrow, a.plane_stride, xl);
        if (lane == last) east = vorticity_edge_uy(row, mrow, a.plane_stride, xr);
#pragma unroll
        for (int v = 0; v < V; v++) dvdx_c[v] = (v == V - 1 ? east : uy_c[v + 1 < V ? v + 1 : v]) - (v == 0 ? west : uy_c[v > 0 ? v - 1 : v]);
      }
      if (rr > r0) {  // (uniform) row e = rr - 1 is complete: ux_a is row e - 1's, ux_c row e + 1's
        const int e = rr - 1;
        const unsigned cell = cell_first + (unsigned)e * (unsigned)a.nx + (unsigned)x;
        [[maybe_unused]] float w_out[V];
#pragma unroll
        for (int v = 0; v < V; v++) {
          const bool fluid = ((fluid_b >> v) & 1u) != 0u;
          const float dudy = ux_c[v] - ux_a[v];
          const float w = fluid ? 0.5f * (dvdx_b[v] - dudy) : 0.f;
          const float wsq = w * w;
          if constexpr (FIELD) w_out[v] = w;
          const unsigned b_w = __float_as_uint(w), b_wsq = __float_as_uint(wsq);
          const bool finite = ((fin_b >> v) & 1u) != 0u && lbm_exact::exact_sum_finite(b_w) && lbm_exact::exact_sum_finite(b_wsq);
          const int s = (fluid && finite) ? 1 : 0;
          lbm_exact::exact_sum_add(acc[0], b_wsq, s);
          lbm_exact::exact_sum_add(acc[1], b_w, s);
          bad += (fluid && !finite) ? 1 : 0;
          n_fluid += s;
          const unsigned long long cell_key = lbm_stats::stats_key(__float_as_uint(fabsf(w)), cell + (unsigned)v);
          key = (s && cell_key > key) ? cell_key : key;
        }
        if constexpr (FIELD) {
          if (field && valid) {
            float* out = field + (size_t)(e - row_begin) * a.nx + x;
            if constexpr (V == 4)
              *reinterpret_cast<float4*>(out) = make_float4(w_out[0], w_out[1], w_out[2], w_out[3]);
            else
              out[0] = w_out[0];
          }
        }
      }
#pragma unroll
      for (int v = 0; v < V; v++) {
        ux_a[v] = ux_b[v];
        ux_b[v] = ux_c[v];
        dvdx_b[v] = dvdx_c[v];
      }
      fluid_b = fluid_c;
      fin_b = fin_c;
    }
  }
  if (!words) return;  // (uniform) the field alone
  auto wave_total = [&](long long t, int word) {
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
    if (lane == 0) sh[wave][word] = t;
  };
#pragma unroll
  for (int j = 0; j < S; j++)
#pragma unroll
    for (int i = 0; i < L; i++) wave_total(acc[j][i], j * L + i);
  wave_total(bad, lbm_enstrophy::kEnstrophyBadWord);
  wave_total(n_fluid, lbm_enstrophy::kEnstrophyFluidWord);
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = (unsigned long long)__shfl_down((long long)key, off, 64);
    key = other > key ? other : key;
  }
  if (lane == 0) sh[wave][lbm_enstrophy::kEnstrophyKeyWord] = (long long)key;
  __syncthreads();
  if (threadIdx.x < W) {
    unsigned long long* word = reinterpret_cast<unsigned long long*>(words + threadIdx.x);
    if (threadIdx.x == lbm_enstrophy::kEnstrophyKeyWord) {
      unsigned long long m = 0ull;
      for (int w = 0; w < kWaves; w++) m = (unsigned long long)sh[w][threadIdx.x] > m ? (unsigned long long)sh[w][threadIdx.x] : m;
      if (m != 0ull) atomicMax(word, m);
    } else {
      long long t = 0;
      for (int w = 0; w < kWaves; w++) t += sh[w][threadIdx.x];
      if (t != 0) atomicAdd(word, (unsigned long long)t);
    }
  }
}

// the rows [row_begin, row_end) of a slab's `rows` owned rows into `field` and / or its words of the ring row; cell_first:
// the GLOBAL index of its first owned cell; grid: vorticity_groups (the host's rule) workgroups
template <int V, bool FIELD>
__global__ __launch_bounds__(kBlock) void vorticity_gather(const LatticeArgs a, const float* south, const float* north, int rows, int row_begin,
                                                           int row_end, int band_rows, unsigned cell_first, float* field, long long* words) {
  vorticity_cells<V, FIELD>(a, a.src, a.mask, south, north, rows, row_begin, row_end, band_rows, cell_first, field, words);
}

// vorticity_gather's twin for a batch: one sample of every member in one launch, workgroup (g, 0, member) on the member's
// current lattice and mask (members[member]; `a` carries the strides all members share), a periodic slab each, into the
// member's words of the row, [members][kEnstrophyWords]
template <int V>
__global__ __launch_bounds__(kBlock) void vorticity_gather_batch(const LatticeArgs a, const ResidentMember* members, int rows, int band_rows,
                                                                 long long* row) {
  const int member = blockIdx.z;
  const float* src = members[member].src;
  vorticity_cells<V, false>(a, src, members[member].mask, src + (long)(rows - 1) * a.row_pitch, src, rows, 0, rows, band_rows, 0u, nullptr,
                     row + (size_t)member * lbm_enstrophy::kEnstrophyWords);
}

// ---------------------------------------------------------------------------------------------
// stress and dissipation (lbm_read_stress, lbm_set_stress): the kinematic non-equilibrium stress t_ab = Pi_ab / rho of
// every cell of a stored lattice from its second moment, as three fields and / or as the exact sums of q = t:t and of
// txy, the largest q with its cell and the counts of a row (lbm_stress_row.h)
// ---------------------------------------------------------------------------------------------
// The definition of include/lbm_hip.h, in its order: fp32, IEEE divide, no contraction (the build's -ffp-contract=off).
// rho, jx, jy, ux, uy, usq are the statistics' (moments_exact).  The second moments of the D2Q9 equilibrium are rho/3 +
// rho ux^2, rho/3 + rho uy^2 and rho ux uy exactly, so no per-direction equilibrium is evaluated.  The one place where the
// row form and the field form get their per-cell values: they cannot drift apart.
struct StressCell {
  float txx, txy, tyy, q;
  bool finite;  // rho, jx, jy, usq, txx, tyy, txy and q are all finite
};
__device__ __forceinline__ StressCell stress_cell(const float (&f)[kQ]) {
  float rho, ux, uy;
  moments_exact(f, rho, ux, uy);
  const float jx = f[1] + f[5] + f[8] - (f[3] + f[6] + f[7]);
  const float jy = f[2] + f[5] + f[6] - (f[4] + f[7] + f[8]);
  const float usq = (ux * ux) + (uy * uy);
  const float a56 = f[5] + f[6], a78 = f[7] + f[8];
  const float mxx = ((f[1] + f[3]) + a56) + a78;
  const float myy = ((f[2] + f[4]) + a56) + a78;
  const float mxy = (f[5] + f[7]) - (f[6] + f[8]);
  const float third = rho / 3.0f;
  const float pxx = (mxx - third) - (jx * ux);
  const float pyy = (myy - third) - (jy * uy);
  const float pxy = mxy - (jx * uy);
  StressCell c;
  c.txx = pxx / rho;
  c.tyy = pyy / rho;
  c.txy = pxy / rho;
  c.q = ((c.txx * c.txx) + (c.tyy * c.tyy)) + (2.0f * (c.txy * c.txy));
  c.finite = lbm_exact::exact_sum_finite(__float_as_uint(rho)) && lbm_exact::exact_sum_finite(__float_as_uint(jx)) &&
             lbm_exact::exact_sum_finite(__float_as_uint(jy)) && lbm_exact::exact_sum_finite(__float_as_uint(usq)) &&
             lbm_exact::exact_sum_finite(__float_as_uint(c.txx)) && lbm_exact::exact_sum_finite(__float_as_uint(c.tyy)) &&
             lbm_exact::exact_sum_finite(__float_as_uint(c.txy)) && lbm_exact::exact_sum_finite(__float_as_uint(c.q));
  return c;
}

// One sample, built the way stats_cells is: the cells of the rows [row_begin, row_begin + rows) of a slab are dealt out V
// at a time along x (V = 4 where nx % 4 == 0: nine 16-byte plane loads and one 4-byte mask load per lane; V = 1 otherwise)
// to the lanes of a capped grid that strides; no unit reaches into the pitch padding (x + V <= nx).  A lane keeps two
// fixed-point accumulators (q, txy), its two counts and its key, stats_key(bits of q, global cell) -- q >= +0; a cell that
// does not contribute is added with sign 0.  The reduction is stats_cells': shuffles, LDS, 64-bit integer atomicAdd /
// atomicMax into `words` (kStressWords of them, zeroed by the host); no floating-point addition across cells happens on
// the device.  FIELD = true also stores txx, txy, tyy of every cell -- blocked cells 0, a non-finite value as computed --
// to the dense planes field + {0, 1, 2} * field_stride ([rows][nx], row row_begin first; a null `field` or `words` is
// skipped), with 16-byte stores at V = 4 (a unit is 16-byte aligned where nx % 4 == 0 and field_stride % 4 == 0).
template <int V, bool FIELD>
__device__ __forceinline__ void stress_cells(const LatticeArgs& a, const float* src, const unsigned char* mask, int row_begin, int rows,
                                             unsigned cell_first, float* field, long field_stride, long long* words) {
  constexpr int L = lbm_exact::kExactLimbs, S = lbm_stress::kStressSums, W = lbm_stress::kStressKeyWord + 1;
  __shared__ long long sh[kBlock / 64][W];
  long long acc[S][L], bad = 0, n_fluid = 0;
  unsigned long long key = 0ull;
#pragma unroll
  for (int j = 0; j < S; j++)
#pragma unroll
    for (int i = 0; i < L; i++) acc[j][i] = 0;
  const long per_row = a.nx / V, n_units = (long)rows * per_row;
  for (long u = (long)blockIdx.x * kBlock + threadIdx.x; u < n_units; u += (long)gridDim.x * kBlock) {
    const int rr = (int)(u / per_row), x = (int)(u - (long)rr * per_row) * V, r = row_begin + rr;
    const float* p = src + (long)r * a.row_pitch + x;
    float f[V][kQ];
    unsigned blocked;  // byte v: the mask of cell x + v
    if constexpr (V == 4) {
#pragma unroll
      for (int k = 0; k < kQ; k++) {
        const float4 q = *reinterpret_cast<const float4*>(p + k * a.plane_stride);
        f[0][k] = q.x;  f[1][k] = q.y;  f[2][k] = q.z;  f[3][k] = q.w;
      }
      blocked = *reinterpret_cast<const unsigned*>(mask + (long)r * a.pitch + x);
    } else {
#pragma unroll
      for (int k = 0; k < kQ; k++) f[0][k] = p[k * a.plane_stride];
      blocked = mask[(long)r * a.pitch + x];
    }
    const unsigned cell = cell_first + (unsigned)r * (unsigned)a.nx + (unsigned)x;
    [[maybe_unused]] float oxx[V], oxy[V], oyy[V];
#pragma unroll
    for (int v = 0; v < V; v++) {
      const StressCell c = stress_cell(f[v]);
      const bool fluid = ((blocked >> (8 * v)) & 0xffu) == 0u;
      if constexpr (FIELD) {
        oxx[v] = fluid ? c.txx : 0.f;
        oxy[v] = fluid ? c.txy : 0.f;
        oyy[v] = fluid ? c.tyy : 0.f;
      }
      const int s = (fluid && c.finite) ? 1 : 0;
      lbm_exact::exact_sum_add(acc[0], __float_as_uint(c.q), s);
      lbm_exact::exact_sum_add(acc[1], __float_as_uint(c.txy), s);
      bad += (fluid && !c.finite) ? 1 : 0;
      n_fluid += s;
      const unsigned long long cell_key = lbm_stats::stats_key(__float_as_uint(c.q), cell + (unsigned)v);
      key = (s && cell_key > key) ? cell_key : key;
    }
    if constexpr (FIELD) {
      if (field) {
        float* out = field + (long)rr * a.nx + x;
        if constexpr (V == 4) {
          *reinterpret_cast<float4*>(out) = make_float4(oxx[0], oxx[1], oxx[2], oxx[3]);
          *reinterpret_cast<float4*>(out + field_stride) = make_float4(oxy[0], oxy[1], oxy[2], oxy[3]);
          *reinterpret_cast<float4*>(out + 2 * field_stride) = make_float4(oyy[0], oyy[1], oyy[2], oyy[3]);
        } else {
          out[0] = oxx[0];
          out[field_stride] = oxy[0];
          out[2 * field_stride] = oyy[0];
        }
      }
    }
  }
  if (!words) return;  // (uniform) the field alone
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto wave_total = [&](long long t, int word) {
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
    if (lane == 0) sh[wave][word] = t;
  };
#pragma unroll
  for (int j = 0; j < S; j++)
#pragma unroll
    for (int i = 0; i < L; i++) wave_total(acc[j][i], j * L + i);
  wave_total(bad, lbm_stress::kStressBadWord);
  wave_total(n_fluid, lbm_stress::kStressFluidWord);
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = (unsigned long long)__shfl_down((long long)key, off, 64);
    key = other > key ? other : key;
  }
  if (lane == 0) sh[wave][lbm_stress::kStressKeyWord] = (long long)key;
  __syncthreads();
  if (threadIdx.x < W) {
    unsigned long long* word = reinterpret_cast<unsigned long long*>(words + threadIdx.x);
    if (threadIdx.x == lbm_stress::kStressKeyWord) {
      unsigned long long m = 0ull;
      for (int w = 0; w < kBlock / 64; w++) m = (unsigned long long)sh[w][threadIdx.x] > m ? (unsigned long long)sh[w][threadIdx.x] : m;
      if (m != 0ull) atomicMax(word, m);
    } else {
      long long t = 0;
      for (int w = 0; w < kBlock / 64; w++) t += sh[w][threadIdx.x];
      if (t != 0) atomicAdd(word, (unsigned long long)t);
    }
  }
}

// the rows [row_begin, row_begin + rows) of a slab's owned rows into `field` and / or its words of the ring row;
// cell_first: the GLOBAL index of its first owned cell; grid: stats_groups (the host's rule) workgroups
template <int V, bool FIELD>
__global__ __launch_bounds__(kBlock) void stress_gather(const LatticeArgs a, int row_begin, int rows, unsigned cell_first, float* field,
                                                        long field_stride, long long* words) {
  stress_cells<V, FIELD>(a, a.src, a.mask, row_begin, rows, cell_first, field, field_stride, words);
}

// stress_gather's twin for a batch: one sample of every member in one launch, workgroup (g, 0, member) on the member's
// current lattice and mask (members[member]; `a` carries the strides all members share), into the member's words of the
// row, [members][kStressWords].  The recorder's form only, as vorticity_gather_batch: a batch member's lbm_read_stress
// runs stress_gather<V, true> on the member's handle.
template <int V>
__global__ __launch_bounds__(kBlock) void stress_gather_batch(const LatticeArgs a, const ResidentMember* members, int rows, long long* row) {
  const int member = blockIdx.z;
  stress_cells<V, false>(a, members[member].src, members[member].mask, 0, rows, 0u, nullptr, 0,
                         row + (size_t)member * lbm_stress::kStressWords);
}

// ---------------------------------------------------------------------------------------------
// stream function (lbm_read_psi, lbm_set_psi): psi(x, y) = the exact sum of jx over the finite fluid cells (x, 0 .. y) of a
// stored lattice, rounded once per cell, as a field and / or as its extrema with their cells and the counts of a row
// (lbm_psi_row.h)
// ---------------------------------------------------------------------------------------------
// The one recorded quantity that is a PREFIX along an axis.  Totals meet in atomics, prefixes do not: the scan is blocked
// into bands of band_rows rows whose partial results are fixed-point limbs (lbm_exact_sum.h).  Integer limb addition is
// associative, so neither the band height, the slabs nor scheduling can change a bit of any psi.  As in profile_columns a
// lane owns a column -- consecutive lanes read consecutive addresses of a row -- and walks down the rows of its band;
// workgroup (g, b) owns the columns [g * kPsiColumns, + kPsiColumns) of band b.  Three sweeps:
//   psi_band_totals  each lane adds the terms of its band's rows into one accumulator and stores the limbs to
//                    totals[band][x][kExactLimbs] (plain stores, no atomics: a lane owns its limbs),
//   psi_band_bases   a lane per limb of a column turns the totals, in place, into their exclusive prefix over the bands, starting
//                    from the limbs of everything below the slab (`incoming`, null: nothing), and leaves the limbs of
//                    everything up to the slab's last row in `outgoing` (null: nobody asks) -- the next slab's incoming,
//   psi_scan         each lane starts from its band's base limbs, walks the band's rows again and, after adding a row's
//                    term, rounds the running accumulator (exact_sum_round_hd, lbm_exact_round.h): the inclusive prefix.
//                    FIELD = true stores the double; FIELD = false, the recorder's form, stores nothing per cell: a lane
//                    keeps its running (smallest psi, cell) and (largest psi, cell) over the finite fluid cells -- values
//                    compared as doubles, equal values by the smaller GLOBAL cell index -- the lanes are combined by
//                    shuffles, the waves through LDS, and the workgroup leaves one PsiCandidate,
//   psi_extrema      one wave per slab (or member) reduces the workgroups' candidates in the same order into the row's
//                    words.  A double and a cell do not fit one 64-bit atomic key, so the candidates are reduced explicitly;
//                    the order (value, then cell) is total, so the result does not depend on how they were grouped.
// A term is jx of a finite fluid cell (profile_cell's jx and its rule for finite), 0 of every other cell: added with sign 0.
constexpr int kPsiColumns = kBlock;  // columns of a workgroup: one per lane
constexpr int kPsiMinBand = 8;       // the fewest rows of a band the host chooses by itself
constexpr unsigned kPsiNoCell = 0xffffffffu;

struct PsiCandidate {
  double psi_min, psi_max;      // 0 with kPsiNoCell
  unsigned min_cell, max_cell;  // GLOBAL cell index; kPsiNoCell: the workgroup saw no finite fluid cell
  int fluid, bad;               // its finite fluid cells; its fluid cells that are not finite
};
static_assert(sizeof(PsiCandidate) == 32, "the host sizes the candidates' buffer");

// the term of one cell: the bits of jx, the sign it is added with (1: a finite fluid cell) and whether it is a fluid cell
// that is not finite
__device__ __forceinline__ void psi_term(const float (&g)[kQ], bool fluid, unsigned& bits, int& s, int& bad) {
  float rho, ux, uy;
  moments_exact(g, rho, ux, uy);
  const float jx = g[1] + g[5] + g[8] - (g[3] + g[6] + g[7]);
  const float jy = g[2] + g[5] + g[6] - (g[4] + g[7] + g[8]);
  const float usq = (ux * ux) + (uy * uy);
  bits = __float_as_uint(jx);
  const bool finite = lbm_exact::exact_sum_finite(__float_as_uint(rho)) && lbm_exact::exact_sum_finite(bits) &&
                      lbm_exact::exact_sum_finite(__float_as_uint(jy)) && lbm_exact::exact_sum_finite(__float_as_uint(usq));
  s = (fluid && finite) ? 1 : 0;
  bad = (fluid && !finite) ? 1 : 0;
}

// is the candidate (v, cell) in front of (best, best_cell)?  sign < 0: the smaller value (the minimum), else the larger;
// equal values (+0.0 == -0.0): the smaller cell (lbm_psi::psi_in_front is the host's)
__device__ __forceinline__ bool psi_in_front(double v, unsigned cell, double best, unsigned best_cell, int sign) {
  if (cell == kPsiNoCell) return false;
  if (best_cell == kPsiNoCell) return true;
  if (v != best) return sign < 0 ? v < best : v > best;
  return cell < best_cell;
}

__device__ __forceinline__ void psi_band_totals_lines(const LatticeArgs& a, const float* src, const unsigned char* mask, int rows, int band_rows,
                                                      long long* totals) {
  constexpr int L = lbm_exact::kExactLimbs;
  const int x = (int)blockIdx.x * kPsiColumns + (int)threadIdx.x;
  if (x >= a.nx) return;
  const int r0 = (int)blockIdx.y * band_rows, r1 = (r0 + band_rows < rows) ? r0 + band_rows : rows;
  long long acc[L];
#pragma unroll
  for (int i = 0; i < L; i++) acc[i] = 0;
  for (int r = r0; r < r1; r++) {
    const float* p = src + (long)r * a.row_pitch + x;
    float f[kQ];
#pragma unroll
    for (int k = 0; k < kQ; k++) f[k] = p[k * a.plane_stride];
    unsigned bits;
    int s, bad;
    psi_term(f, mask[(long)r * a.pitch + x] == 0, bits, s, bad);
    lbm_exact::exact_sum_add(acc, bits, s);
  }
  long long* out = totals + ((size_t)blockIdx.y * a.nx + x) * L;
#pragma unroll
  for (int i = 0; i < L; i++) out[i] = acc[i];
}

// a slab's owned rows into totals[bands][nx][kExactLimbs]; grid: (ceil(nx / kPsiColumns), bands)
__global__ __launch_bounds__(kBlock) void psi_band_totals(const LatticeArgs a, int rows, int band_rows, long long* totals) {
  psi_band_totals_lines(a, a.src, a.mask, rows, band_rows, totals);
}
// its twin for a batch: workgroup (g, b, member) on the member's current lattice and mask, into the member's totals
__global__ __launch_bounds__(kBlock) void psi_band_totals_batch(const LatticeArgs a, const ResidentMember* members, int rows, int band_rows,
                                                                long long* totals) {
  const int member = blockIdx.z;
  psi_band_totals_lines(a, members[member].src, members[member].mask, rows, band_rows,
                        totals + (size_t)member * gridDim.y * a.nx * lbm_exact::kExactLimbs);
}

// totals[bands][nx][kExactLimbs] -> in place, the limbs of everything below each band.  Limbs do not carry into each other
// (lbm_exact_sum.h), so a lane owns one WORD of a band, (column, limb) = (word / kExactLimbs, word % kExactLimbs) --
// consecutive lanes, consecutive addresses -- and walks the bands, kPsiAhead loads in flight at a time: the walk is serial in
// the bands and a grid of a few thousand columns has few lanes to hide it behind.  grid: (ceil(nx * kExactLimbs / kBlock),
// 1, members), member m on totals + m * bands * nx * kExactLimbs (incoming and outgoing belong to a single slab: members == 1)
constexpr int kPsiAhead = 8;
__global__ __launch_bounds__(kBlock) void psi_band_bases(int nx, int bands, long long* totals, const long long* incoming, long long* outgoing) {
  const size_t n_words = (size_t)nx * lbm_exact::kExactLimbs;
  const size_t word = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (word >= n_words) return;
  totals += (size_t)blockIdx.z * bands * n_words + word;
  long long base = incoming ? incoming[word] : 0;
  for (int b0 = 0; b0 < bands; b0 += kPsiAhead) {
    long long t[kPsiAhead];
#pragma unroll
    for (int j = 0; j < kPsiAhead; j++) t[j] = (b0 + j < bands) ? totals[(size_t)(b0 + j) * n_words] : 0;
#pragma unroll
    for (int j = 0; j < kPsiAhead; j++) {
      if (b0 + j < bands) totals[(size_t)(b0 + j) * n_words] = base;
      base += t[j];
    }
  }
  if (outgoing) outgoing[word] = base;
}

// the bands [band_first, band_first + gridDim.y) of a slab's `rows` owned rows from their bases.  FIELD: psi of their cells
// into `field` (dense, the first row of band band_first first, nx doubles per row); else the workgroup's candidate into
// cand[blockIdx.y * gridDim.x + blockIdx.x].  cell_first: the GLOBAL index of the slab's first owned cell.
template <bool FIELD>
__device__ __forceinline__ void psi_scan_cells(const LatticeArgs& a, const float* src, const unsigned char* mask, int rows, int band_rows,
                                               int band_first, const long long* bases, unsigned cell_first, double* field, PsiCandidate* cand) {
  constexpr int L = lbm_exact::kExactLimbs;
  constexpr int kWaves = kBlock / 64;
  const int band = band_first + (int)blockIdx.y;
  const int x = (int)blockIdx.x * kPsiColumns + (int)threadIdx.x;
  const int r0 = band * band_rows, r1 = (r0 + band_rows < rows) ? r0 + band_rows : rows;
  double lo = 0.0, hi = 0.0;
  unsigned lo_cell = kPsiNoCell, hi_cell = kPsiNoCell;
  int n_fluid = 0, n_bad = 0;
  if (x < a.nx) {
    long long acc[L];
    const long long* base = bases + ((size_t)band * a.nx + x) * L;
#pragma unroll
    for (int i = 0; i < L; i++) acc[i] = base[i];
    for (int r = r0; r < r1; r++) {
      const float* p = src + (long)r * a.row_pitch + x;
      float f[kQ];
#pragma unroll
      for (int k = 0; k < kQ; k++) f[k] = p[k * a.plane_stride];
      unsigned bits;
      int s, bad;
      psi_term(f, mask[(long)r * a.pitch + x] == 0, bits, s, bad);
      lbm_exact::exact_sum_add(acc, bits, s);
      const double psi = lbm_exact::exact_sum_round_hd(acc);  // (never -0.0)
      if constexpr (FIELD) {
        field[(size_t)(r - band_first * band_rows) * a.nx + x] = psi;
      } else {
        // rows ascend, so among a lane's equal values the first (the smallest cell) stays
        const unsigned cell = s ? cell_first + (unsigned)r * (unsigned)a.nx + (unsigned)x : kPsiNoCell;
        if (psi_in_front(psi, cell, lo, lo_cell, -1)) { lo = psi; lo_cell = cell; }
        if (psi_in_front(psi, cell, hi, hi_cell, +1)) { hi = psi; hi_cell = cell; }
        n_fluid += s;
        n_bad += bad;
      }
    }
  }
  if constexpr (!FIELD) {
    __shared__ double sh_v[2][kWaves];
    __shared__ unsigned sh_c[2][kWaves];
    __shared__ int sh_n[2][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 32; off > 0; off >>= 1) {
      const double o_lo = __shfl_xor(lo, off, 64), o_hi = __shfl_xor(hi, off, 64);
      const unsigned o_lo_cell = __shfl_xor(lo_cell, off, 64), o_hi_cell = __shfl_xor(hi_cell, off, 64);
      if (psi_in_front(o_lo, o_lo_cell, lo, lo_cell, -1)) { lo = o_lo; lo_cell = o_lo_cell; }
      if (psi_in_front(o_hi, o_hi_cell, hi, hi_cell, +1)) { hi = o_hi; hi_cell = o_hi_cell; }
      n_fluid += __shfl_xor(n_fluid, off, 64);
      n_bad += __shfl_xor(n_bad, off, 64);
    }
    if (lane == 0) {
      sh_v[0][wave] = lo;  sh_v[1][wave] = hi;
      sh_c[0][wave] = lo_cell;  sh_c[1][wave] = hi_cell;
      sh_n[0][wave] = n_fluid;  sh_n[1][wave] = n_bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      PsiCandidate c = {0.0, 0.0, kPsiNoCell, kPsiNoCell, 0, 0};
      for (int w = 0; w < kWaves; w++) {
        if (psi_in_front(sh_v[0][w], sh_c[0][w], c.psi_min, c.min_cell, -1)) { c.psi_min = sh_v[0][w]; c.min_cell = sh_c[0][w]; }
        if (psi_in_front(sh_v[1][w], sh_c[1][w], c.psi_max, c.max_cell, +1)) { c.psi_max = sh_v[1][w]; c.max_cell = sh_c[1][w]; }
        c.fluid += sh_n[0][w];
        c.bad += sh_n[1][w];
      }
      cand[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = c;
    }
  }
}

// grid: (ceil(nx / kPsiColumns), bands of this launch)
template <bool FIELD>
__global__ __launch_bounds__(kBlock) void psi_scan(const LatticeArgs a, int rows, int band_rows, int band_first, const long long* bases,
                                                   unsigned cell_first, double* field, PsiCandidate* cand) {
  psi_scan_cells<FIELD>(a, a.src, a.mask, rows, band_rows, band_first, bases, cell_first, field, cand);
}
// the recorder's form for a batch: workgroup (g, b, member), every member a grid of its own (cell_first 0), its bases and
// candidates behind the members' before it
__global__ __launch_bounds__(kBlock) void psi_scan_batch(const LatticeArgs a, const ResidentMember* members, int rows, int band_rows,
                                                         const long long* bases, PsiCandidate* cand) {
  const int member = blockIdx.z;
  psi_scan_cells<false>(a, members[member].src, members[member].mask, rows, band_rows, 0,
                        bases + (size_t)member * gridDim.y * a.nx * lbm_exact::kExactLimbs, 0u, nullptr,
                        cand + (size_t)member * gridDim.y * gridDim.x);
}

// the n candidates of a slab (or of member blockIdx.x, n apart) into its kPsiWords words of the row; grid: (members), one
// wave each.  Every word the readers use is stored: the row needs no zeroing.
__global__ __launch_bounds__(64) void psi_extrema(const PsiCandidate* cand, int n, long long* words) {
  cand += (size_t)blockIdx.x * n;
  words += (size_t)blockIdx.x * lbm_psi::kPsiWords;
  double lo = 0.0, hi = 0.0;
  unsigned lo_cell = kPsiNoCell, hi_cell = kPsiNoCell;
  long long n_fluid = 0, n_bad = 0;
  for (int i = threadIdx.x; i < n; i += 64) {
    const PsiCandidate c = cand[i];
    if (psi_in_front(c.psi_min, c.min_cell, lo, lo_cell, -1)) { lo = c.psi_min; lo_cell = c.min_cell; }
    if (psi_in_front(c.psi_max, c.max_cell, hi, hi_cell, +1)) { hi = c.psi_max; hi_cell = c.max_cell; }
    n_fluid += c.fluid;
    n_bad += c.bad;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double o_lo = __shfl_xor(lo, off, 64), o_hi = __shfl_xor(hi, off, 64);
    const unsigned o_lo_cell = __shfl_xor(lo_cell, off, 64), o_hi_cell = __shfl_xor(hi_cell, off, 64);
    if (psi_in_front(o_lo, o_lo_cell, lo, lo_cell, -1)) { lo = o_lo; lo_cell = o_lo_cell; }
    if (psi_in_front(o_hi, o_hi_cell, hi, hi_cell, +1)) { hi = o_hi; hi_cell = o_hi_cell; }
    n_fluid += __shfl_xor(n_fluid, off, 64);
    n_bad += __shfl_xor(n_bad, off, 64);
  }
  if (threadIdx.x == 0) {
    words[lbm_psi::kPsiMinWord] = lo_cell == kPsiNoCell ? 0ll : (long long)__double_as_longlong(lo + 0.0);  // (+ 0.0: never -0.0)
    words[lbm_psi::kPsiMaxWord] = hi_cell == kPsiNoCell ? 0ll : (long long)__double_as_longlong(hi + 0.0);
    words[lbm_psi::kPsiMinCellWord] = lo_cell == kPsiNoCell ? -1ll : (long long)lo_cell;
    words[lbm_psi::kPsiMaxCellWord] = hi_cell == kPsiNoCell ? -1ll : (long long)hi_cell;
    words[lbm_psi::kPsiFluidWord] = n_fluid;
    words[lbm_psi::kPsiBadWord] = n_bad;
  }
}

// ---------------------------------------------------------------------------------------------
// tracer particles (lbm_set_tracers): positions advected through the velocity field of a stored lattice
// ---------------------------------------------------------------------------------------------
// The one gather whose reads depend on data: a lane owns a tracer, reads its position, and per stage of the midpoint
// step (lbm_tracer_step.h: tracer_advance, the function the CPU check runs) gathers the 4 cells around a position -- 36
// populations through gather_cell's addressing and 4 mask bytes, all issued before the first moment is formed: the
// callable below has no branch, a blocked cell's populations are loaded like any other and its velocity selected to 0, 0
// behind moments_exact -- then forms the four velocities as final_state does and interpolates in doubles.  Two dependent
// stages, so two round trips to memory per sample; neighbouring tracers share cache lines only where the caller seeded
// them in row-major order.  The lane is the only writer of its tracer: the state is updated in place and the same 16
// bytes go to the ring row (null: armed without a ring).  No atomics, no LDS.  A lost tracer is written through.
// grid: (ceil(n / kBlock), 1, members)
__device__ __forceinline__ void tracer_lane(const LatticeArgs& a, const float* __restrict__ src, const unsigned char* __restrict__ mask, int ny,
                                            int n, int span, double2* state, double2* row) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double2 p = state[i];
  const auto u = [&](int x, int y) -> lbm_tracers::Vec {
    const long c = (long)y * a.row_pitch + x;
    float f[kQ];
#pragma unroll
    for (int k = 0; k < kQ; k++) f[k] = src[k * a.plane_stride + c];
    const bool blocked = mask[(long)y * a.pitch + x] != 0;
    float rho, ux, uy;
    moments_exact(f, rho, ux, uy);
    return {blocked ? 0.0 : (double)ux, blocked ? 0.0 : (double)uy};
  };
  const lbm_tracers::Vec q = lbm_tracers::tracer_advance(lbm_tracers::Vec{p.x, p.y}, a.nx, ny, span, u);
  const double2 out = make_double2(q.x, q.y);
  state[i] = out;
  if (row) row[i] = out;
}

// one sample of a context's n tracers over `span` timesteps in the field of a.src, the whole grid of ny rows
__global__ __launch_bounds__(kBlock) void tracer_advance(const LatticeArgs a, int ny, int n, int span, double2* state, double2* row) {
  tracer_lane(a, a.src, a.mask, ny, n, span, state, row);
}

// tracer_advance's twin for a batch: one launch for all members' tracers, workgroup (g, 0, member) in the member's current
// lattice and mask; state and row are [members][n]
__global__ __launch_bounds__(kBlock) void tracer_advance_batch(const LatticeArgs a, const ResidentMember* members, int ny, int n, int span,
                                                               double2* state, double2* row) {
  const size_t member = blockIdx.z;
  tracer_lane(a, members[member].src, members[member].mask, ny, n, span, state + member * (size_t)n, row ? row + member * (size_t)n : nullptr);
}

}  // namespace lbm
