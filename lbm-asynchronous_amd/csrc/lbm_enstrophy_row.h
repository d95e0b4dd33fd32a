// lbm_enstrophy_row.h -- from the words vorticity_gather leaves in a ring row to the lbm_enstrophy_row the readers hand
// out (lbm_read_enstrophy, lbm_batch_read_enstrophy).  A slab (or a batch member) owns kEnstrophyWords int64 words of a
// row, 24 words = 192 bytes:
//   [0, 9)   the fixed-point limbs (lbm_exact_sum.h) of the sum of wsq = w * w over its finite fluid cells,
//   [9, 18)  of w over the same cells,
//   18       its fluid cells that are not finite,
//   19       its finite fluid cells,
//   20       its max key, unsigned: lbm_stats::stats_key(bits of fabsf(w), GLOBAL cell index y * nx + x) -- |w| >= +0, so
//            unsigned order is value order and, among equal values, the smaller index wins; 0: the slab has no finite
//            fluid cell (lbm_stats_row.h),
//   21 .. 23 unused.
// The slabs' limbs are added as integers -- the order of the slabs does not matter -- and each sum is rounded once.
// No HIP, no allocation: any C++17 compiler builds it (tests/enstrophy_row_check.cpp checks it without a GPU).
#pragma once

#include <cstdint>
#include <cstring>

#include "lbm_exact_sum.h"
#include "lbm_stats_row.h"
#include "../../include/lbm_hip.h"

namespace lbm_enstrophy {

constexpr int kEnstrophySums = 2;  // wsq, w
constexpr int kEnstrophyBadWord = kEnstrophySums * lbm_exact::kExactLimbs;  // 18
constexpr int kEnstrophyFluidWord = kEnstrophyBadWord + 1;                  // 19
constexpr int kEnstrophyKeyWord = kEnstrophyFluidWord + 1;                  // 20
constexpr int kEnstrophyWords = 24;                                         // 192 bytes
static_assert(kEnstrophyKeyWord < kEnstrophyWords, "a slab's words hold the two accumulators, the two counts and the key");

// words[n_slabs][kEnstrophyWords] of one row (the slabs of a context; one "slab" for a batch member) -> the row; nx:
// cells per row of the whole grid
inline lbm_enstrophy_row enstrophy_row_from_words(const long long* words, int n_slabs, int nx) {
  constexpr int L = lbm_exact::kExactLimbs;
  long long sum[kEnstrophySums][L] = {};
  long long bad = 0, fluid = 0;
  unsigned long long key = 0;
  for (int s = 0; s < n_slabs; s++) {
    const long long* w = words + (size_t)s * kEnstrophyWords;
    for (int j = 0; j < kEnstrophySums; j++)
      for (int i = 0; i < L; i++) sum[j][i] += w[j * L + i];
    bad += w[kEnstrophyBadWord];
    fluid += w[kEnstrophyFluidWord];
    const unsigned long long k = (unsigned long long)w[kEnstrophyKeyWord];
    if (k > key) key = k;
  }
  lbm_enstrophy_row row;
  std::memset(&row, 0, sizeof(row));
  row.enstrophy = lbm_exact::exact_sum_round(sum[0]);
  row.circulation = lbm_exact::exact_sum_round(sum[1]);
  row.nonfinite = bad;
  row.fluid = (int)fluid;
  row.max_x = row.max_y = -1;
  if (key != 0) {
    const uint32_t bits = (uint32_t)(key >> 32);
    const uint32_t cell = 0xffffffffu - (uint32_t)(key & 0xffffffffull);
    std::memcpy(&row.max_abs_w, &bits, sizeof(bits));
    row.max_x = (int)(cell % (uint32_t)nx);
    row.max_y = (int)(cell / (uint32_t)nx);
  }
  return row;
}

}  // namespace lbm_enstrophy
