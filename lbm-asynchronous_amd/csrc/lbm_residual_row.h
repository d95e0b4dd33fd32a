// lbm_residual_row.h -- from the words residual_gather leaves in a ring row to the lbm_residual_row the readers hand out
// (lbm_read_residual, lbm_batch_read_residual).  A slab (or a batch member) owns kResidualWords int64 words of a row:
//   [0, 9)   the fixed-point limbs (lbm_exact_sum.h) of the sum of dsq = |u - u_remembered|^2 over its finite fluid cells,
//   [9, 18)  of usq over the same cells,
//   18       its fluid cells that are not finite,
//   19       its max key, unsigned, built as the statistics build theirs (lbm_stats_row.h: stats_key): the bits of dmag in
//            the high word, 0xffffffff - GLOBAL cell index (y * nx + x) in the low word; dmag >= +0, so unsigned order is
//            value order and, among equal values, the smaller index wins.  0: the slab has no finite fluid cell.
// The slabs' limbs are added as integers -- the order of the slabs does not matter -- and each sum is rounded once.
// No HIP, no allocation: any C++17 compiler builds it (tests/residual_row_check.cpp checks it without a GPU).
#pragma once

#include <cstdint>
#include <cstring>

#include "lbm_exact_sum.h"
#include "lbm_stats_row.h"
#include "../../include/lbm_hip.h"

namespace lbm_residual {

constexpr int kResidualSums = 2;  // dsq, usq
constexpr int kResidualBadWord = kResidualSums * lbm_exact::kExactLimbs;  // 18
constexpr int kResidualKeyWord = kResidualBadWord + 1;                    // 19
constexpr int kResidualWords = 20;                                        // 160 bytes
static_assert(kResidualKeyWord < kResidualWords, "a slab's words hold the two accumulators, the count and the key");

// words[n_slabs][kResidualWords] of one row (the slabs of a context; one "slab" for a batch member) -> the row; nx: cells
// per row of the whole grid; span: timesteps between the remembered field and the sample (the host knows it)
inline lbm_residual_row residual_row_from_words(const long long* words, int n_slabs, int nx, int span) {
  constexpr int L = lbm_exact::kExactLimbs;
  long long sum[kResidualSums][L] = {};
  long long bad = 0;
  unsigned long long key = 0;
  for (int s = 0; s < n_slabs; s++) {
    const long long* w = words + (size_t)s * kResidualWords;
    for (int j = 0; j < kResidualSums; j++)
      for (int i = 0; i < L; i++) sum[j][i] += w[j * L + i];
    bad += w[kResidualBadWord];
    const unsigned long long k = (unsigned long long)w[kResidualKeyWord];
    if (k > key) key = k;
  }
  lbm_residual_row row;
  std::memset(&row, 0, sizeof(row));
  row.sum_du_sq = lbm_exact::exact_sum_round(sum[0]);
  row.sum_u_sq = lbm_exact::exact_sum_round(sum[1]);
  row.nonfinite = bad;
  row.max_x = row.max_y = -1;
  row.span = span;
  if (key != 0) {
    const uint32_t bits = (uint32_t)(key >> 32);
    const uint32_t cell = 0xffffffffu - (uint32_t)(key & 0xffffffffull);
    std::memcpy(&row.max_du, &bits, sizeof(bits));
    row.max_x = (int)(cell % (uint32_t)nx);
    row.max_y = (int)(cell / (uint32_t)nx);
  }
  return row;
}

}  // namespace lbm_residual
