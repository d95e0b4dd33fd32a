// residual_row_check.cpp -- checks lbm-asynchronous_amd/csrc/lbm_residual_row.h ("words -> lbm_residual_row") without a
// GPU (tests/test_residual_abi.py builds and feeds it).  Standard input holds cases: "<slabs> <nx> <span>", then per slab
// two sums -- each "m" and m float bits in hex: the terms of dsq and of usq -- then "<non-finite cells>", then "k" and k
// pairs "<dmag bits, hex> <global cell>", the slab's finite fluid cells that compete for the maximum; then one line
// "<sum_du_sq> <sum_u_sq> (double bits, hex) <nonfinite> <max_du bits, hex> <max_x> <max_y> <span>", what the row must be.
// A slab's words are filled as residual_gather fills them: exact_sum_add per term, the largest stats_key.  Exit status 0
// when every case gives the expected row.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lbm-asynchronous_amd/csrc/lbm_residual_row.h"

static_assert(sizeof(lbm_residual_row) == 40, "lbm_residual_row is 40 bytes");
static_assert(offsetof(lbm_residual_row, span) == 36, "span is the last word");

int main() {
  using namespace lbm_residual;
  constexpr int L = lbm_exact::kExactLimbs;
  int slabs, nx, span, cases = 0, failed = 0;
  while (std::scanf("%d %d %d", &slabs, &nx, &span) == 3) {
    std::vector<long long> words((size_t)slabs * kResidualWords, 0);
    for (int s = 0; s < slabs; s++) {
      long long* w = words.data() + (size_t)s * kResidualWords;
      for (int j = 0; j < kResidualSums; j++) {
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
      if (std::scanf("%lld %d", &w[kResidualBadWord], &k) != 2) return 2;
      unsigned long long key = 0;
      for (int i = 0; i < k; i++) {
        unsigned bits, cell;
        if (std::scanf("%x %u", &bits, &cell) != 2) return 2;
        const unsigned long long c = lbm_stats::stats_key(bits, cell);
        if (c > key) key = c;
      }
      w[kResidualKeyWord] = (long long)key;
    }
    unsigned long long want[2];
    long long want_bad;
    unsigned want_du;
    int want_x, want_y, want_span;
    if (std::scanf("%llx %llx %lld %x %d %d %d", &want[0], &want[1], &want_bad, &want_du, &want_x, &want_y, &want_span) != 7) return 2;
    const lbm_residual_row row = residual_row_from_words(words.data(), slabs, nx, span);
    const double sums[2] = {row.sum_du_sq, row.sum_u_sq};
    unsigned long long got[2];
    unsigned got_du;
    std::memcpy(got, sums, sizeof(got));
    std::memcpy(&got_du, &row.max_du, sizeof(got_du));
    if (std::memcmp(got, want, sizeof(got)) != 0 || row.nonfinite != want_bad || got_du != want_du || row.max_x != want_x || row.max_y != want_y ||
        row.span != want_span) {
      std::printf("case %d: got %016llx %016llx %lld %08x %d %d %d, expected %016llx %016llx %lld %08x %d %d %d\n", cases, got[0], got[1],
                  row.nonfinite, got_du, row.max_x, row.max_y, row.span, want[0], want[1], want_bad, want_du, want_x, want_y, want_span);
      failed++;
    }
    cases++;
  }
  std::printf("%d cases, %d failed\n", cases, failed);
  return (failed || cases == 0) ? 1 : 0;
}
