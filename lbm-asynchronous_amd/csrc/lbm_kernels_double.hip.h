// lbm_kernels_double.hip.h -- the double-precision twins of the one-step kernels (lbm_kernels.hip.h), for the
// lbm_double_* entry points of include/lbm_hip.h.
//
// The reference's programs are `float`, but its golden results (the .dat files of check/) are the same algorithm evaluated in IEEE
// double: SerialCode/d2q9-bgk.c:207-458 with every float read as double, sqrtf as sqrt, `1.f` as 1.0, reproduces them
// to the last printed digit ("Double precision").  These kernels are that reading: every
// expression tree of the reference is kept, every divide is an IEEE divide (the multiply-by-reciprocal forms of the
// fp32 kernels were verified exhaustively over fp32, which cannot be done over doubles), sqrt is IEEE, and nothing is
// contracted (the library is built with -ffp-contract=off).
//
// Layout: that of the fp32 engine with doubles -- value (k, y, x) at base + (y*9 + k)*pitch + x, pitch a multiple of 64
// elements -- without halo rows: a double context is one periodic slab, and rows wrap inside the kernels.  The obstacle
// mask is the fp32 engine's (uint8 rows of `pitch` bytes, built by lbm::mask_from_int).
//
// step_double: one timestep per pass, two cells per lane, nine aligned 16-byte loads and stores per lane: 144 bytes per
// lattice update, twice step_vec4's, and like it bound by memory traffic.  step_double_scalar: one cell per lane, any nx.
#pragma once
#include "lbm_kernels.hip.h"

namespace lbm {

constexpr double kCsqD = 1.0 / 3.0;                 // SerialCode/d2q9-bgk.c:308 read as double
constexpr double kTwoCsqD = 2.0 * kCsqD;            // "2.f * c_sq" (:367)
constexpr double kTwoCsqSqD = 2.0 * kCsqD * kCsqD;  // "2.f * c_sq * c_sq" (:370)
constexpr double kW0D = 4.0 / 9.0;
constexpr double kW1D = 1.0 / 9.0;
constexpr double kW2D = 1.0 / 36.0;

// where a double lattice lies: LatticeArgs with double planes (a type of its own: LatticeArgs does not change)
struct LatticeArgsD {
  const double* src;
  double* dst;
  const unsigned char* mask;  // rows x pitch bytes, 1 = blocked
  long plane_stride;          // doubles between planes
  long row_pitch;             // doubles between lattice rows of one plane
  int pitch;                  // bytes between rows of the mask
  int nx;
};

struct StepArgsD : LatticeArgsD {
  int rows;          // ny: rows wrap periodically
  int accel_row;     // row that receives the next step's acceleration, or kNoRow
  double omega;
  double a1, a2;     // density*accel/9.0, density*accel/36.0 (SerialCode/d2q9-bgk.c:219-220)
  double* partials;  // one partial sum of |u| per workgroup of this launch
};

__device__ __forceinline__ void gather_cell_d(const LatticeArgsD& a, int row, int x, double (&f)[kQ]) {
  const long c = (long)row * a.row_pitch + x;
#pragma unroll
  for (int k = 0; k < kQ; k++) f[k] = a.src[k * a.plane_stride + c];
}
__device__ __forceinline__ bool cell_blocked_d(const LatticeArgsD& a, int row, int x) {
  return a.mask[(long)row * a.pitch + x] != 0;
}

// local density and velocity (SerialCode/d2q9-bgk.c:325-347).  The sum starts from 0.0 as the reference's does: 0.0 + f[0]
// is f[0] except for f[0] = -0.0, and nine -0.0 must sum to +0.0 (the sign of a zero pressure; without fast-math flags
// the compiler keeps the add)
__device__ __forceinline__ void moments_d(const double (&f)[kQ], double& rho, double& ux, double& uy) {
  double d = 0.0 + f[0];
#pragma unroll
  for (int k = 1; k < kQ; k++) d += f[k];
  rho = d;
  ux = (f[1] + f[5] + f[8] - (f[3] + f[6] + f[7])) / d;
  uy = (f[2] + f[5] + f[6] - (f[4] + f[7] + f[8])) / d;
}

__device__ __forceinline__ double speed_d(const double (&f)[kQ]) {
  double rho, ux, uy;
  moments_d(f, rho, ux, uy);
  return sqrt((ux * ux) + (uy * uy));  // IEEE: OCML's f64 sqrt is correctly rounded
}

// collision() of one fluid cell (SerialCode/d2q9-bgk.c:325-401).  u[3] = -u[1], u[4] = -u[2], u[7] = -u[5] and
// u[8] = -u[6] are exact negations (rounding is symmetric), so the quotients of the four opposite directions are the
// negated / identical quotients of the first four: eleven divides per cell, every one an IEEE divide.
__device__ __forceinline__ void collide_d(const double (&t)[kQ], double omega, double (&r)[kQ]) {
  double rho, ux, uy;
  moments_d(t, rho, ux, uy);
  const double u_sq = ux * ux + uy * uy;
  const double usq_term = u_sq / kTwoCsqD;
  const double w1r = kW1D * rho, w2r = kW2D * rho;
  const double us = ux + uy, ud = -ux + uy;
  const double x1 = ux / kCsqD, x2 = (ux * ux) / kTwoCsqSqD;
  const double y1 = uy / kCsqD, y2 = (uy * uy) / kTwoCsqSqD;
  const double s1 = us / kCsqD, s2 = (us * us) / kTwoCsqSqD;
  const double d1 = ud / kCsqD, d2 = (ud * ud) / kTwoCsqSqD;
  double eq[kQ];
  eq[0] = kW0D * rho * (1.0 - usq_term);
  eq[1] = w1r * (1.0 + x1 + x2 - usq_term);
  eq[2] = w1r * (1.0 + y1 + y2 - usq_term);
  eq[3] = w1r * (1.0 + -x1 + x2 - usq_term);
  eq[4] = w1r * (1.0 + -y1 + y2 - usq_term);
  eq[5] = w2r * (1.0 + s1 + s2 - usq_term);
  eq[6] = w2r * (1.0 + d1 + d2 - usq_term);
  eq[7] = w2r * (1.0 + -s1 + s2 - usq_term);
  eq[8] = w2r * (1.0 + -d1 + d2 - usq_term);
#pragma unroll
  for (int k = 0; k < kQ; k++) r[k] = t[k] + omega * (eq[k] - t[k]);
}

// accelerate_flow() on one cell (SerialCode/d2q9-bgk.c:229-242)
__device__ __forceinline__ void accelerate_d(double (&f)[kQ], double a1, double a2) {
  if ((f[3] - a1) > 0.0 && (f[6] - a2) > 0.0 && (f[7] - a2) > 0.0) {
    f[1] += a1;  f[5] += a2;  f[8] += a2;
    f[3] -= a1;  f[6] -= a2;  f[7] -= a2;
  }
}

// rebound(): mirrored copy, speed 0 kept (SerialCode/d2q9-bgk.c:291-298)
__device__ __forceinline__ void bounce_d(const double (&t)[kQ], double (&r)[kQ]) {
  r[0] = t[0];
  r[1] = t[3];  r[2] = t[4];  r[3] = t[1];  r[4] = t[2];
  r[5] = t[7];  r[6] = t[8];  r[7] = t[5];  r[8] = t[6];
}

// one cell of one timestep after the pull: rebound or collision, |u| of the relaxed cell as av_velocity() sees it
// (:426-450), then the NEXT step's accelerate_flow on the lid row
__device__ __forceinline__ double relax_cell_d(const double (&t)[kQ], bool blocked, bool lid, const StepArgsD& a,
                                               double (&r)[kQ]) {
  if (blocked) {
    bounce_d(t, r);
    return 0.0;
  }
  collide_d(t, a.omega, r);
  const double speed = speed_d(r);
  if (lid) accelerate_d(r, a.a1, a.a2);
  return speed;
}

// workgroup sum in a fixed order: wave64 shuffles, then one LDS hop across the four waves; valid in thread 0
__device__ __forceinline__ double block_sum_d(double v) {
  __shared__ double wave_part[kBlock / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = v;
  __syncthreads();
  double total = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kBlock / 64; w++) total += wave_part[w];
  }
  return total;
}

// a double from the adjacent lane: two DPP moves (wave_shr:1 / wave_shl:1), one per half, as lane_from_west<2> moves a float
__device__ __forceinline__ double lane_from_west_d(double v) {  // lane i <- lane i-1
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, 0x138, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), 0x138, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double lane_from_east_d(double v) {  // lane i <- lane i+1
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, 0x130, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), 0x130, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

template <bool NTS>
__device__ __forceinline__ void store2_d(double* p, double a, double b) {
  typedef double v2 __attribute__((ext_vector_type(2)));
  const v2 v = {a, b};
  if constexpr (NTS) __builtin_nontemporal_store(v, reinterpret_cast<v2*>(p));
  else *reinterpret_cast<v2*>(p) = v;
}

// ---------------------------------------------------------------------------------------------
// fused step, 2 cells per lane (nx % 2 == 0; pitch % 2 == 0): the fp64 twin of step_vec4<0, 2, NTS>
// ---------------------------------------------------------------------------------------------
template <bool NTS>
__global__ __launch_bounds__(kBlock) void step_double(const StepArgsD a) {
  const int pairs_x = a.nx >> 1;
  const long n_pairs = (long)pairs_x * a.rows;
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  const long ps = a.plane_stride;
  double my_sum = 0.0;

  if (q < n_pairs) {
    const int row = (int)(q / pairs_x);
    const int x0 = (int)(q - (long)row * pairs_x) << 1;
    // neighbour columns and rows with periodic wrap (SerialCode/d2q9-bgk.c:257-260)
    const int xw = (x0 == 0) ? a.nx - 1 : x0 - 1;
    const int xe = (x0 + 2 == a.nx) ? 0 : x0 + 2;
    const int rs = (row == 0) ? a.rows - 1 : row - 1;
    const int rn = (row == a.rows - 1) ? 0 : row + 1;
    const double* c_row = a.src + (long)row * a.row_pitch;
    const double* sb = a.src + (long)rs * a.row_pitch;
    const double* nb = a.src + (long)rn * a.row_pitch;
    const double *s2 = sb + 2 * ps, *s5 = sb + 5 * ps, *s6 = sb + 6 * ps;
    const double *n4 = nb + 4 * ps, *n7 = nb + 7 * ps, *n8 = nb + 8 * ps;

    // 9 aligned 16-byte loads
    const double2 v0 = *reinterpret_cast<const double2*>(c_row + x0);
    const double2 v1 = *reinterpret_cast<const double2*>(c_row + 1 * ps + x0);
    const double2 v3 = *reinterpret_cast<const double2*>(c_row + 3 * ps + x0);
    const double2 v2 = *reinterpret_cast<const double2*>(s2 + x0);
    const double2 v5 = *reinterpret_cast<const double2*>(s5 + x0);
    const double2 v6 = *reinterpret_cast<const double2*>(s6 + x0);
    const double2 v4 = *reinterpret_cast<const double2*>(n4 + x0);
    const double2 v7 = *reinterpret_cast<const double2*>(n7 + x0);
    const double2 v8 = *reinterpret_cast<const double2*>(n8 + x0);
    // the cell just west of the pair (speeds 1, 5, 8) and just east of it (3, 6, 7): the adjacent lane's
    const int lane = threadIdx.x & 63;
    double e1 = lane_from_west_d(v1.y), e5 = lane_from_west_d(v5.y), e8 = lane_from_west_d(v8.y);
    double e3 = lane_from_east_d(v3.x), e6 = lane_from_east_d(v6.x), e7 = lane_from_east_d(v7.x);
    // the wave's first / last lane and the row ends have no such lane: 8 bytes each
    if (lane == 0 || x0 == 0) {
      e1 = c_row[1 * ps + xw];  e5 = s5[xw];  e8 = n8[xw];
    }
    if (lane == 63 || x0 + 2 == a.nx || q + 1 == n_pairs) {
      e3 = c_row[3 * ps + xe];  e6 = s6[xe];  e7 = n7[xe];
    }
    const uchar2 m = *reinterpret_cast<const uchar2*>(a.mask + (long)row * a.pitch + x0);

    const double t0[kQ] = {v0.x, e1, v2.x, v3.y, v4.x, e5, v6.y, v7.y, e8};
    const double t1[kQ] = {v0.y, v1.x, v2.y, e3, v4.y, v5.x, e6, e7, v8.x};
    const bool lid = (row == a.accel_row);
    double r0[kQ], r1[kQ];
    my_sum = relax_cell_d(t0, m.x != 0, lid, a, r0);
    my_sum += relax_cell_d(t1, m.y != 0, lid, a, r1);

    double* d_row = a.dst + (long)row * a.row_pitch + x0;
#pragma unroll
    for (int k = 0; k < kQ; k++) store2_d<NTS>(d_row + k * ps, r0[k], r1[k]);
  }

  const double total = block_sum_d(my_sum);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------------------------
// fused step, 1 cell per lane: any nx
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void step_double_scalar(const StepArgsD a) {
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  const long n_cells = (long)a.nx * a.rows;
  const long ps = a.plane_stride;
  double my_sum = 0.0;
  if (q < n_cells) {
    const int row = (int)(q / a.nx);
    const int x = (int)(q - (long)row * a.nx);
    const int xw = (x == 0) ? a.nx - 1 : x - 1;
    const int xe = (x + 1 == a.nx) ? 0 : x + 1;
    const int rs = (row == 0) ? a.rows - 1 : row - 1;
    const int rn = (row == a.rows - 1) ? 0 : row + 1;
    const double* c_row = a.src + (long)row * a.row_pitch;
    const double* sb = a.src + (long)rs * a.row_pitch;
    const double* nb = a.src + (long)rn * a.row_pitch;
    const double t[kQ] = {c_row[x],        c_row[1 * ps + xw], sb[2 * ps + x],  c_row[3 * ps + xe], nb[4 * ps + x],
                          sb[5 * ps + xw], sb[6 * ps + xe],    nb[7 * ps + xe], nb[8 * ps + xw]};
    double r[kQ];
    my_sum = relax_cell_d(t, cell_blocked_d(a, row, x), row == a.accel_row, a, r);
    double* d = a.dst + (long)row * a.row_pitch + x;
#pragma unroll
    for (int k = 0; k < kQ; k++) d[k * ps] = r[k];
  }
  const double total = block_sum_d(my_sum);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------------------------
// small kernels around the step
// ---------------------------------------------------------------------------------------------

// accelerate_flow() as its own pass (SerialCode/d2q9-bgk.c:216-246): before the first step of a call; later steps get
// it from the epilogue of the step kernel
__global__ void accelerate_row_d(const LatticeArgsD a, int row, double a1, double a2) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= a.nx) return;
  if (cell_blocked_d(a, row, x)) return;
  const long ps = a.plane_stride;
  double* lat = a.dst + (long)row * a.row_pitch + x;
  double f[kQ];
#pragma unroll
  for (int k = 0; k < kQ; k++) f[k] = lat[k * ps];
  accelerate_d(f, a1, a2);
  lat[1 * ps] = f[1];  lat[3 * ps] = f[3];  lat[5 * ps] = f[5];
  lat[6 * ps] = f[6];  lat[7 * ps] = f[7];  lat[8 * ps] = f[8];
}

// the per-workgroup partials of up to gridDim.x steps -> tot_u: block s adds partials[s][0..n_part) in a fixed order
// (lane i takes i, i + 256, ... in turn, then a tree over the 256 lanes).  Deterministic, no atomics.
__global__ __launch_bounds__(kBlock) void reduce_partials_d(const double* partials, int n_part, long slot_stride,
                                                            double* tot_u, int step_base) {
  __shared__ double sh[kBlock];
  const double* p = partials + (long)blockIdx.x * slot_stride;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_part; i += kBlock) acc += p[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) tot_u[step_base + blockIdx.x] = sh[0];
}

// uniform equilibrium start (SerialCode/d2q9-bgk.c:546-567)
__global__ void init_equilibrium_d(const LatticeArgsD a, int rows, double r0, double r1, double r2) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (long)a.nx * rows) return;
  const long row = j / a.nx;
  const long ps = a.plane_stride;
  double* lat = a.dst + row * a.row_pitch + (j - row * a.nx);
  lat[0] = r0;
  lat[1 * ps] = r1;  lat[2 * ps] = r1;  lat[3 * ps] = r1;  lat[4 * ps] = r1;
  lat[5 * ps] = r2;  lat[6 * ps] = r2;  lat[7 * ps] = r2;  lat[8 * ps] = r2;
}

// AoS (reference host layout, 9 doubles per cell) <-> SoA planes, rows [row0, row0+nrows)
__global__ void aos_to_soa_d(const double* aos, const LatticeArgsD a, int row0, int nrows) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)a.nx * nrows * kQ) return;
  const long cell = i / kQ;
  const int k = (int)(i - cell * kQ);
  const int r = (int)(cell / a.nx), x = (int)(cell - (long)r * a.nx);
  a.dst[k * a.plane_stride + (long)(row0 + r) * a.row_pitch + x] = aos[i];
}
__global__ void soa_to_aos_d(const LatticeArgsD a, double* aos, int row0, int nrows) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)a.nx * nrows * kQ) return;
  const long cell = i / kQ;
  const int k = (int)(i - cell * kQ);
  const int r = (int)(cell / a.nx), x = (int)(cell - (long)r * a.nx);
  aos[i] = a.src[k * a.plane_stride + (long)(row0 + r) * a.row_pitch + x];
}

// write_values() quantities (SerialCode/d2q9-bgk.c:684-719)
__global__ void final_state_d(const LatticeArgsD a, int row0, int nrows, double density, double* ux_o, double* uy_o,
                              double* um_o, double* pr_o) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)a.nx * nrows) return;
  const int r = (int)(i / a.nx), x = (int)(i - (long)r * a.nx);
  if (cell_blocked_d(a, row0 + r, x)) {
    ux_o[i] = 0.0;  uy_o[i] = 0.0;  um_o[i] = 0.0;
    pr_o[i] = density * kCsqD;
  } else {
    double f[kQ];
    gather_cell_d(a, row0 + r, x, f);
    double rho, ux, uy;
    moments_d(f, rho, ux, uy);
    ux_o[i] = ux;  uy_o[i] = uy;
    um_o[i] = sqrt((ux * ux) + (uy * uy));
    pr_o[i] = rho * kCsqD;
  }
}

// av_velocity() (SerialCode/d2q9-bgk.c:409-458) and total_density() (:644-660) of a stored lattice: per-workgroup
// partials, grid-stride, tree-summed
__global__ __launch_bounds__(kBlock) void lattice_sums_d(const LatticeArgsD a, int rows, double* speed_part, double* mass_part) {
  __shared__ double sh_s[kBlock], sh_m[kBlock];
  double s = 0.0, m = 0.0;
  const long n = (long)a.nx * rows;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long)gridDim.x * kBlock) {
    const int r = (int)(i / a.nx), x = (int)(i - (long)r * a.nx);
    double f[kQ];
    gather_cell_d(a, r, x, f);
    double rho, ux, uy;
    moments_d(f, rho, ux, uy);
    m += rho;
    if (!cell_blocked_d(a, r, x)) s += sqrt((ux * ux) + (uy * uy));
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

}  // namespace lbm
