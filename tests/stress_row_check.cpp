// stress_row_check.cpp -- checks lbm-asynchronous_amd/csrc/lbm_stress_row.h ("words -> lbm_stress_row") without a GPU
// (tests/test_stress_abi.py builds and feeds it).  Standard input holds cases: "<slabs> <nx>", then per slab two sums --
// each "m" and m float bits in hex: the terms of q and of txy -- then "<non-finite cells> <finite fluid cells>", then "k"
// and k pairs "<q bits, hex> <global cell>", the slab's finite fluid cells that compete for the maximum; then one line
// "<sum_q> <sum_txy> (double bits, hex) <nonfinite> <max_q bits, hex> <max_x> <max_y> <fluid>", what the row must be.  A
// slab's words are filled as stress_gather fills them: exact_sum_add per term, the largest stats_key.  Exit status 0 when
// every case gives the expected row.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lbm-asynchronous_amd/csrc/lbm_enstrophy_row.h"
#include "../lbm-asynchronous_amd/csrc/lbm_stress_row.h"

static_assert(sizeof(lbm_stress_row) == 40, "lbm_stress_row is 40 bytes");
static_assert(offsetof(lbm_stress_row, sum_q) == 0 && offsetof(lbm_stress_row, sum_txy) == 8 && offsetof(lbm_stress_row, nonfinite) == 16 &&
                  offsetof(lbm_stress_row, max_q) == 24 && offsetof(lbm_stress_row, max_x) == 28 && offsetof(lbm_stress_row, max_y) == 32 &&
                  offsetof(lbm_stress_row, fluid) == 36,
              "the row's layout is lbm_enstrophy_row's");
static_assert(lbm_stress::kStressWords * sizeof(long long) == 192, "a slab's share of a row is 192 bytes");
static_assert(lbm_stress::kStressWords == lbm_enstrophy::kEnstrophyWords && lbm_stress::kStressKeyWord == lbm_enstrophy::kEnstrophyKeyWord,
              "the slot is laid out and padded as the enstrophy's is");

int main() {
  using namespace lbm_stress;
  constexpr int L = lbm_exact::kExactLimbs;
  int slabs, nx, cases = 0, failed = 0;
  while (std::scanf("%d %d", &slabs, &nx) == 2) {
    std::vector<long long> words((size_t)slabs * kStressWords, 0);
    for (int s = 0; s < slabs; s++) {
      long long* w = words.data() + (size_t)s * kStressWords;
      for (int j = 0; j < kStressSums; j++) {
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
      if (std::scanf("%lld %lld %d", &w[kStressBadWord], &w[kStressFluidWord], &k) != 3) return 2;
      unsigned long long key = 0;
      for (int i = 0; i < k; i++) {
        unsigned bits, cell;
        if (std::scanf("%x %u", &bits, &cell) != 2) return 2;
        const unsigned long long c = lbm_stats::stats_key(bits, cell);
        if (c > key) key = c;
      }
      w[kStressKeyWord] = (long long)key;
    }
    unsigned long long want[2];
    long long want_bad;
    unsigned want_q;
    int want_x, want_y, want_fluid;
    if (std::scanf("%llx %llx %lld %x %d %d %d", &want[0], &want[1], &want_bad, &want_q, &want_x, &want_y, &want_fluid) != 7) return 2;
    const lbm_stress_row row = stress_row_from_words(words.data(), slabs, nx);
    const double sums[2] = {row.sum_q, row.sum_txy};
    unsigned long long got[2];
    unsigned got_q;
    std::memcpy(got, sums, sizeof(got));
    std::memcpy(&got_q, &row.max_q, sizeof(got_q));
    if (std::memcmp(got, want, sizeof(got)) != 0 || row.nonfinite != want_bad || got_q != want_q || row.max_x != want_x || row.max_y != want_y ||
        row.fluid != want_fluid) {
      std::printf("case %d: got %016llx %016llx %lld %08x %d %d %d, expected %016llx %016llx %lld %08x %d %d %d\n", cases, got[0], got[1],
                  row.nonfinite, got_q, row.max_x, row.max_y, row.fluid, want[0], want[1], want_bad, want_q, want_x, want_y, want_fluid);
      failed++;
    }
    cases++;
  }
  std::printf("%d cases, %d failed\n", cases, failed);
  return (failed || cases == 0) ? 1 : 0;
}
