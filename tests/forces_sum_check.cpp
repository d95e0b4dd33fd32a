// forces_sum_check.cpp -- checks lbm-asynchronous_amd/csrc/lbm_exact_sum.h without a GPU (tests/test_forces_abi.py builds
// and feeds it).  Standard input holds cases: "n" then n lines "<float bits, hex> <sign: -1, 0 or 1>" then one line
// "<expected double bits, hex>", the correctly rounded sum of sign * float.  The terms are dealt to four accumulators in
// turn, which are then added limb by limb -- as lanes, workgroups and slabs are -- and rounded once.  Exit status 0 when
// every case gives the expected bits.
#include <cstdio>
#include <cstring>

#include "../lbm-asynchronous_amd/csrc/lbm_exact_sum.h"

int main() {
  using namespace lbm_exact;
  int n, cases = 0, failed = 0;
  while (std::scanf("%d", &n) == 1) {
    long long part[4][kExactLimbs] = {};
    for (int i = 0; i < n; i++) {
      unsigned bits;
      int sign;
      if (std::scanf("%x %d", &bits, &sign) != 2) return 2;
      if (!exact_sum_finite(bits)) return 3;
      exact_sum_add(part[i & 3], bits, sign);
    }
    long long acc[kExactLimbs] = {};
    for (int w = 3; w >= 0; w--)
      for (int j = 0; j < kExactLimbs; j++) acc[j] += part[w][j];
    unsigned long long want;
    if (std::scanf("%llx", &want) != 1) return 2;
    const double got = exact_sum_round(acc);
    unsigned long long got_bits;
    std::memcpy(&got_bits, &got, sizeof(got));
    if (got_bits != want) {
      std::printf("case %d (%d terms): got %016llx, expected %016llx\n", cases, n, got_bits, want);
      failed++;
    }
    cases++;
  }
  std::printf("%d cases, %d failed\n", cases, failed);
  return (failed || cases == 0) ? 1 : 0;
}
