// lbm_stress_row.h -- from the words stress_gather leaves in a ring row to the lbm_stress_row the readers hand out
// (lbm_read_stress_rows, lbm_batch_read_stress_rows).  A slab (or a batch member) owns kStressWords int64 words of a
// row, 24 words = 192 bytes, laid out as the enstrophy's are:
//   [0, 9)   the fixed-point limbs (lbm_exact_sum.h) of the sum of q = t:t over its finite fluid cells,
//   [9, 18)  of txy over the same cells,
//   18       its fluid cells that are not finite,
//   19       its finite fluid cells,
//   20       its max key, unsigned: lbm_stats::stats_key(bits of q, GLOBAL cell index y * nx + x) -- q >= +0, so unsigned
//            order is value order and, among equal values, the smaller index wins; 0: the slab has no finite fluid cell
//            (lbm_stats_row.h),
//   21 .. 23 unused.
// The slabs' limbs are added as integers -- the order of the slabs does not matter -- and each sum is rounded once.
// No HIP, no allocation: any C++17 compiler builds it (tests/stress_row_check.cpp checks it without a GPU).
#pragma once

#include <cstdint>
#include <cstring>

#include "lbm_exact_sum.h"
#include "lbm_stats_row.h"
#include "../../include/lbm_hip.h"

namespace lbm_stress {

constexpr int kStressSums = 2;  // q, txy
constexpr int kStressBadWord = kStressSums * lbm_exact::kExactLimbs;  // 18
constexpr int kStressFluidWord = kStressBadWord + 1;                  // 19
constexpr int kStressKeyWord = kStressFluidWord + 1;                  // 20
constexpr int kStressWords = 24;                                      // 192 bytes
static_assert(kStressKeyWord < kStressWords, "a slab's words hold the two accumulators, the two counts and the key");

// words[n_slabs][kStressWords] of one row (the slabs of a context; one "slab" for a batch member) -> the row; nx: cells
// per row of the whole grid
inline lbm_stress_row stress_row_from_words(const long long* words, int n_slabs, int nx) {
  constexpr int L = lbm_exact::kExactLimbs;
  long long sum[kStressSums][L] = {};
  long long bad = 0, fluid = 0;
  unsigned long long key = 0;
  for (int s = 0; s < n_slabs; s++) {
    const long long* w = words + (size_t)s * kStressWords;
    for (int j = 0; j < kStressSums; j++)
      for (int i = 0; i < L; i++) sum[j][i] += w[j * L + i];
    bad += w[kStressBadWord];
    fluid += w[kStressFluidWord];
    const unsigned long long k = (unsigned long long)w[kStressKeyWord];
    if (k > key) key = k;
  }
  lbm_stress_row row;
  std::memset(&row, 0, sizeof(row));
  row.sum_q = lbm_exact::exact_sum_round(sum[0]);
  row.sum_txy = lbm_exact::exact_sum_round(sum[1]);
  row.nonfinite = bad;
  row.fluid = (int)fluid;
  row.max_x = row.max_y = -1;
  if (key != 0) {
    const uint32_t bits = (uint32_t)(key >> 32);
    const uint32_t cell = 0xffffffffu - (uint32_t)(key & 0xffffffffull);
    std::memcpy(&row.max_q, &bits, sizeof(bits));
    row.max_x = (int)(cell % (uint32_t)nx);
    row.max_y = (int)(cell / (uint32_t)nx);
  }
  return row;
}

}  // namespace lbm_stress
