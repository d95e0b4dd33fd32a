// stats_row_check.cpp -- checks lbm-asynchronous_amd/csrc/lbm_stats_row.h ("words -> lbm_stats_row") without a GPU
// (tests/test_stats_abi.py builds and feeds it).  Standard input holds cases: "<slabs> <nx>", then per slab four sums --
// each "m" and m float bits in hex: the terms of rho, jx, jy, usq -- then "<non-finite cells>", then "k" and k pairs
// "<umag bits, hex> <global cell>", the slab's finite fluid cells that compete for the maximum; then one line
// "<mass> <mom_x> <mom_y> <sum_u_sq> (double bits, hex) <nonfinite> <max_u bits, hex> <max_x> <max_y>", what the row must be.
// A slab's words are filled as stats_gather fills them: exact_sum_add per term, the largest stats_key.  Exit status 0 when
// every case gives the expected row.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lbm-asynchronous_amd/csrc/lbm_stats_row.h"

static_assert(sizeof(lbm_stats_row) == 56, "lbm_stats_row is 56 bytes");

int main() {
  using namespace lbm_stats;
  constexpr int L = lbm_exact::kExactLimbs;
  int slabs, nx, cases = 0, failed = 0;
  while (std::scanf("%d %d", &slabs, &nx) == 2) {
    std::vector<long long> words((size_t)slabs * kStatsWords, 0);
    for (int s = 0; s < slabs; s++) {
      long long* w = words.data() + (size_t)s * kStatsWords;
      for (int j = 0; j < kStatsSums; j++) {
        int m;
        if (std::scanf("%d", &m) != 1) return 2;
        long long acc[L] = {};
        for (int i = 0; i < m; i++) {
          unsigned bits;
          if (std::scanf("%x", &bits) != 1) return 2;
          if (!lbm_exact::exact_sum_finite(bits)) return 3;
          lbm_exact::exact_sum_add(acc, bits, 1);
        }
        for (int i = 0; i < L; i++) w[j * L + i] = acc[i];
      }
      int k;
      if (std::scanf("%lld %d", &w[kStatsBadWord], &k) != 2) return 2;
      unsigned long long key = 0;
      for (int i = 0; i < k; i++) {
        unsigned bits, cell;
        if (std::scanf("%x %u", &bits, &cell) != 2) return 2;
        const unsigned long long c = stats_key(bits, cell);
        if (c > key) key = c;
      }
      w[kStatsKeyWord] = (long long)key;
    }
    unsigned long long want[4];
    long long want_bad;
    unsigned want_u;
    int want_x, want_y;
    if (std::scanf("%llx %llx %llx %llx %lld %x %d %d", &want[0], &want[1], &want[2], &want[3], &want_bad, &want_u, &want_x, &want_y) != 8) return 2;
    const lbm_stats_row row = stats_row_from_words(words.data(), slabs, nx);
    const double sums[4] = {row.mass, row.mom_x, row.mom_y, row.sum_u_sq};
    unsigned long long got[4];
    unsigned got_u;
    std::memcpy(got, sums, sizeof(got));
    std::memcpy(&got_u, &row.max_u, sizeof(got_u));
    if (std::memcmp(got, want, sizeof(got)) != 0 || row.nonfinite != want_bad || got_u != want_u || row.max_x != want_x || row.max_y != want_y ||
        row.reserved != 0) {
      std::printf("case %d: got %016llx %016llx %016llx %016llx %lld %08x %d %d, expected %016llx %016llx %016llx %016llx %lld %08x %d %d\n", cases,
                  got[0], got[1], got[2], got[3], row.nonfinite, got_u, row.max_x, row.max_y, want[0], want[1], want[2], want[3], want_bad,
                  want_u, want_x, want_y);
      failed++;
    }
    cases++;
  }
  std::printf("%d cases, %d failed\n", cases, failed);
  return (failed || cases == 0) ? 1 : 0;
}
