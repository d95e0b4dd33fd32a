// CPU check of csrc/lbm_tracer_step.h, the header the tracer kernels run on the device: a stand-alone program, built by
// tests/test_tracer_step.py with -ffp-contract=off under AddressSanitizer and UBSan; nothing is loaded into Python.
// 1. tracer_wrap over adversarial doubles for n in {2, 3, 13, 1024, 8192}: a finite z gives a value in [0, n), never
//    "lost"; a z that is not finite gives NaN (lost); on [0, n) it is the identity, bit for bit.
// 2. tracer_cell of every double tried, NaN, infinities and values outside the grid included: i0 and i1 inside the grid,
//    f in [0, 1); inside the grid i0 = floor(z), f = z - i0, i1 the periodic successor.
//    Prints "<cases> cases, <failed> failed".
// 3. Standard input holds cases: "<nx> <ny> <h> <n>", then ny * nx pairs "<u_x bits> <u_y bits>" (float, hex, row-major),
//    then n pairs "<x bits> <y bits>" (double, hex).  For each tracer one line "<x' bits> <y' bits>" of tracer_advance over
//    the plane; the test compares them with tests/tracer_model.py, which is written from include/lbm_hip.h.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../lbm-asynchronous_amd/csrc/lbm_tracer_step.h"

using namespace lbm_tracers;

static uint64_t bits_of(double z) {
  uint64_t b;
  std::memcpy(&b, &z, sizeof(b));
  return b;
}
static double double_of(uint64_t b) {
  double z;
  std::memcpy(&z, &b, sizeof(z));
  return z;
}
static float float_of(uint32_t b) {
  float z;
  std::memcpy(&z, &b, sizeof(z));
  return z;
}

static long cases = 0, failed = 0;
static void expect(bool ok, const char* what, double z, int n) {
  cases++;
  if (ok) return;
  failed++;
  std::printf("FAILED %s: z = %a (%.17g), n = %d\n", what, z, z, n);
}

static void check_cell(double z, int n) {
  const Cell c = tracer_cell(z, n);
  expect(c.i0 >= 0 && c.i0 < n && c.i1 >= 0 && c.i1 < n && c.f >= 0.0 && c.f < 1.0, "tracer_cell leaves the grid", z, n);
  if (z >= 0.0 && z < (double)n)
    expect((double)c.i0 == std::floor(z) && bits_of(c.f) == bits_of(z - (double)(long long)std::floor(z)) && c.i1 == (c.i0 + 1) % n,
           "tracer_cell inside the grid", z, n);  // (i0 is an integer: of z = -0.0 it is 0, not -0.0, and f = -0.0)
}

static void check_wrap(double z, int n) {
  const double w = tracer_wrap(z, n);
  if (std::isfinite(z))
    expect(w >= 0.0 && w < (double)n, "tracer_wrap of a finite z is not in [0, n)", z, n);
  else
    expect(std::isnan(w), "tracer_wrap of a z that is not finite does not report lost", z, n);
  if (z >= 0.0 && z < (double)n) expect(bits_of(w) == bits_of(z + 0.0), "tracer_wrap is not the identity on [0, n)", z, n);
  check_cell(z, n);
  check_cell(w, n);
}

int main() {
  const double inf = HUGE_VAL, nan = std::nan("");
  const double denorm = double_of(1), big = 9007199254740992.0;  // 2^-1074, 2^53
  uint64_t rng = 0x9e3779b97f4a7c15ull;
  for (int n : {2, 3, 13, 1024, 8192}) {
    const double N = (double)n, below = std::nextafter(N, 0.0), ulp = N - below;
    const double list[] = {0.0, -0.0, denorm, -denorm, DBL_MIN, -DBL_MIN, DBL_MIN / 2, -DBL_MIN / 2, DBL_EPSILON, -DBL_EPSILON, below, -ulp,
                           -below, N, -N, std::nextafter(N, inf), N + 0.5, -0.5, 1e-300, -1e-300, big, -big, big + 2.0, -(big + 2.0), 1e300, -1e300,
                           DBL_MAX, -DBL_MAX, 2147483648.0, -2147483649.0, 4294967296.5, inf, -inf, nan, -nan};
    for (double z : list) check_wrap(z, n);
    for (int i = 0; i <= n; i++)  // every cell centre and its neighbours on both sides
      for (double z : {(double)i, std::nextafter((double)i, -inf), std::nextafter((double)i, inf), i + 0.5}) {
        check_wrap(z, n);
        check_wrap(-z, n);
        check_wrap(z + N, n);
        check_wrap(z - 3.0 * N, n);
      }
    for (int i = 0; i < 20000; i++) {  // any bits at all, and values spread over [0, n)
      rng = rng * 6364136223846793005ull + 1442695040888963407ull;
      check_wrap(double_of(rng), n);
      check_wrap(N * ((double)(rng >> 11) * 0x1p-53), n);
    }
  }
  std::printf("%ld cases, %ld failed\n", cases, failed);

  int nx, ny, h, n;
  while (std::scanf("%d %d %d %d", &nx, &ny, &h, &n) == 4) {
    if (nx < 1 || ny < 1 || n < 0) return 2;
    std::vector<float> ux((size_t)nx * ny), uy((size_t)nx * ny);
    for (size_t i = 0; i < ux.size(); i++) {
      unsigned bx, by;
      if (std::scanf("%x %x", &bx, &by) != 2) return 2;
      ux[i] = float_of(bx);
      uy[i] = float_of(by);
    }
    const auto u = [&](int i, int j) -> Vec {
      if (i < 0 || i >= nx || j < 0 || j >= ny) std::abort();  // (the vectors are heap blocks: ASan watches them too)
      return {(double)ux[(size_t)j * nx + i], (double)uy[(size_t)j * nx + i]};
    };
    for (int t = 0; t < n; t++) {
      unsigned long long bx, by;
      if (std::scanf("%llx %llx", &bx, &by) != 2) return 2;
      const Vec q = tracer_advance(Vec{double_of(bx), double_of(by)}, nx, ny, h, u);
      std::printf("%016llx %016llx\n", (unsigned long long)bits_of(q.x), (unsigned long long)bits_of(q.y));
    }
  }
  return failed ? 1 : 0;
}
