// lbm_tracer_step.h -- one advance of a tracer particle (lbm_set_tracers, include/lbm_hip.h states the definition): the
// wrap W, a position's two cells and weight along an axis, the bilinear velocity V over a callable that yields a cell's
// (u_x, u_y), and the midpoint step over a span of timesteps.  The kernels (tracer_advance, tracer_advance_batch in
// lbm_kernels.hip.h) call tracer_advance on the device with a callable that reads the stored lattice; the CPU check
// (tests/tracer_step_check.cpp) calls the same function over a plane of floats.  Every +, -, * below is one IEEE double
// operation: whoever includes this builds with -ffp-contract=off.
// No HIP, no allocation: any C++17 compiler builds it; under hipcc the functions are also device functions.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "lbm_exact_round.h"  // LBM_EXACT_HD

namespace lbm_tracers {

// a position, or a velocity widened to doubles
struct Vec {
  double x, y;
};
static_assert(sizeof(Vec) == 16, "a tracer is two doubles: lbm_tracer of include/lbm_hip.h");

// a position's cells along one axis: i0 = floor(z), i1 its periodic successor, f = z - i0
struct Cell {
  int i0, i1;
  double f;
};

LBM_EXACT_HD bool tracer_finite(double z) {
  uint64_t b;
  memcpy(&b, &z, sizeof(b));
  return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
LBM_EXACT_HD double tracer_nan() {
  const uint64_t b = 0x7ff8000000000000ull;
  double z;
  memcpy(&z, &b, sizeof(z));
  return z;
}
LBM_EXACT_HD Vec tracer_lost() { return {tracer_nan(), tracer_nan()}; }

// W(z, n) = z - n * floor(z / n), and 0.0 where rounding has carried that out of [0, n) (z = -ulp gives n): total on the
// finite doubles, the identity on [0, n).  A z that is not finite gives NaN: the tracer is lost.
LBM_EXACT_HD double tracer_wrap(double z, int n) {
  if (!tracer_finite(z)) return tracer_nan();
  const double N = (double)n;
  const double q = floor(z / N);
  const double w = z - N * q;
  return (w >= 0.0 && w < N) ? w : 0.0;
}

// the cells of z along an axis of n cells.  z in [0, n) is the caller's promise (tracer_wrap keeps it); whatever else
// arrives, a NaN included, is read as 0.0, so that i0 and i1 lie in 0 .. n - 1 for every double
LBM_EXACT_HD Cell tracer_cell(double z, int n) {
  const bool inside = z >= 0.0 && z < (double)n;
  const int i0 = inside ? (int)z : 0;  // (truncation is floor: z >= 0)
  const int i1 = (i0 + 1 == n) ? 0 : i0 + 1;
  return {i0, i1, inside ? z - (double)i0 : 0.0};
}

// one component of V: along x in the rows j0 and j1, then along y; three operations each, in this order
LBM_EXACT_HD double tracer_lerp2(double u00, double u10, double u01, double u11, double fx, double fy) {
  const double a = u00 + fx * (u10 - u00);
  const double b = u01 + fx * (u11 - u01);
  return a + fy * (b - a);
}
// V(x, y): u(i, j) is cell (i, j)'s velocity as a Vec.  The four cells are fetched before the first operation on any
template <class U>
LBM_EXACT_HD Vec tracer_interp(double x, double y, int nx, int ny, const U& u) {
  const Cell cx = tracer_cell(x, nx), cy = tracer_cell(y, ny);
  const Vec u00 = u(cx.i0, cy.i0), u10 = u(cx.i1, cy.i0), u01 = u(cx.i0, cy.i1), u11 = u(cx.i1, cy.i1);
  return {tracer_lerp2(u00.x, u10.x, u01.x, u11.x, cx.f, cy.f), tracer_lerp2(u00.y, u10.y, u01.y, u11.y, cx.f, cy.f)};
}

// one advance of the tracer at p over a span of h timesteps in the field u: the midpoint rule.  A lost tracer (NaN, NaN)
// stays lost; no index is formed from a position that is not finite
template <class U>
LBM_EXACT_HD Vec tracer_advance(Vec p, int nx, int ny, int h, const U& u) {
  if (!tracer_finite(p.x) || !tracer_finite(p.y)) return tracer_lost();
  const double H = (double)h;
  const Vec v1 = tracer_interp(p.x, p.y, nx, ny, u);
  if (!tracer_finite(v1.x) || !tracer_finite(v1.y)) return tracer_lost();
  const double xm = tracer_wrap(p.x + (0.5 * H) * v1.x, nx);
  const double ym = tracer_wrap(p.y + (0.5 * H) * v1.y, ny);
  if (!tracer_finite(xm) || !tracer_finite(ym)) return tracer_lost();
  const Vec v2 = tracer_interp(xm, ym, nx, ny, u);
  if (!tracer_finite(v2.x) || !tracer_finite(v2.y)) return tracer_lost();
  const double x1 = tracer_wrap(p.x + H * v2.x, nx);
  const double y1 = tracer_wrap(p.y + H * v2.y, ny);
  if (!tracer_finite(x1) || !tracer_finite(y1)) return tracer_lost();
  return {x1, y1};
}

}  // namespace lbm_tracers
