// profile_row_check.cpp -- checks lbm-asynchronous_amd/csrc/lbm_profile_row.h ("words -> lbm_profile_line") without a GPU
// (tests/test_profile_abi.py builds and feeds it).  Standard input holds cases: "<slabs> <nx> <ny> <axes>", then per slab
// "<row_first> <row_count>", then that slab's lines in the order of its share of a record -- its row lines if axes & 1,
// then nx column lines (its rows' share) if axes & 2 -- each line as five sums, a sum being "m" and m float bits in hex
// (the terms of rho, jx, jy, ux, uy), then "<fluid> <nonfinite>".  A line's words are filled as the kernels fill them:
// exact_sum_add per term, the two counts, the spare word left 0.  Standard output: per case "case <i>", then per line of
// the record "<sum_rho> <sum_jx> <sum_jy> <sum_ux> <sum_uy> (double bits, hex) <fluid> <nonfinite>".
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lbm-asynchronous_amd/csrc/lbm_profile_row.h"

static_assert(sizeof(lbm_profile_line) == 48, "lbm_profile_line is 48 bytes");

int main() {
  using namespace lbm_profile;
  constexpr int L = lbm_exact::kExactLimbs;
  int slabs, nx, ny, axes, cases = 0;
  while (std::scanf("%d %d %d %d", &slabs, &nx, &ny, &axes) == 4) {
    if (slabs < 1 || nx < 1 || ny < 1 || axes < 1 || axes > 3) return 2;
    std::vector<int> row_first((size_t)slabs), row_count((size_t)slabs);
    std::vector<long long> words;
    for (int s = 0; s < slabs; s++) {
      if (std::scanf("%d %d", &row_first[(size_t)s], &row_count[(size_t)s]) != 2) return 2;
      if (row_first[(size_t)s] < 0 || row_count[(size_t)s] < 1 || row_first[(size_t)s] + row_count[(size_t)s] > ny) return 2;
      const size_t lines = profile_slab_lines(row_count[(size_t)s], nx, axes);
      for (size_t l = 0; l < lines; l++) {
        long long w[kProfileWords] = {};
        for (int j = 0; j < kProfileSums; j++) {
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
        if (std::scanf("%lld %lld", &w[kProfileFluidWord], &w[kProfileBadWord]) != 2) return 2;
        words.insert(words.end(), w, w + kProfileWords);
      }
    }
    const size_t lines = profile_slab_lines(ny, nx, axes);
    std::vector<lbm_profile_line> out(lines);
    std::memset(out.data(), 0xff, lines * sizeof(lbm_profile_line));
    profile_lines_from_words(words.data(), slabs, row_first.data(), row_count.data(), nx, ny, axes, out.data());
    std::printf("case %d\n", cases);
    for (const lbm_profile_line& line : out) {
      const double sums[kProfileSums] = {line.sum_rho, line.sum_jx, line.sum_jy, line.sum_ux, line.sum_uy};
      unsigned long long bits[kProfileSums];
      std::memcpy(bits, sums, sizeof(bits));
      std::printf("%016llx %016llx %016llx %016llx %016llx %d %d\n", bits[0], bits[1], bits[2], bits[3], bits[4], line.fluid, line.nonfinite);
    }
    cases++;
  }
  return cases == 0 ? 1 : 0;
}
