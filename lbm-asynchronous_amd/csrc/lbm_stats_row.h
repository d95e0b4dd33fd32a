// lbm_stats_row.h -- from the words stats_gather leaves in a ring row to the lbm_stats_row the readers hand out
// (lbm_read_stats, lbm_batch_read_stats).  A slab (or a batch member) owns kStatsWords int64 words of a row:
//   [0, 9)   the fixed-point limbs (lbm_exact_sum.h) of the sum of rho over its finite cells,
//   [9, 18)  of jx, [18, 27) of jy, [27, 36) of usq over its finite fluid cells,
//   36       its cells that are not finite,
//   37       its max key, unsigned: the bits of umag in the high word, 0xffffffff - GLOBAL cell index (y * nx + x) in the
//            low word; umag >= +0, so unsigned order is value order and, among equal values, the smaller index wins.
//            0: the slab has no finite fluid cell (a cell's key has a low word of at least 1: a grid has at most
//            2^32 - 1 cells, so its indices end below 0xffffffff),
//   38, 39   unused.
// The slabs' limbs are added as integers -- the order of the slabs does not matter -- and each sum is rounded once.
// No HIP, no allocation: any C++17 compiler builds it (tests/stats_row_check.cpp checks it without a GPU).
#pragma once

#include <cstdint>
#include <cstring>

#include "lbm_exact_sum.h"
#include "../../include/lbm_hip.h"

namespace lbm_stats {

constexpr int kStatsSums = 4;  // rho, jx, jy, usq
constexpr int kStatsBadWord = kStatsSums * lbm_exact::kExactLimbs;  // 36
constexpr int kStatsKeyWord = kStatsBadWord + 1;                    // 37
constexpr int kStatsWords = 40;                                     // 320 bytes
static_assert(kStatsKeyWord < kStatsWords, "a slab's words hold the four accumulators, the count and the key");

// the key of a finite fluid cell
LBM_EXACT_HD unsigned long long stats_key(unsigned umag_bits, unsigned global_cell) {
  return ((unsigned long long)umag_bits << 32) | (unsigned long long)(0xffffffffu - global_cell);
}

// words[n_slabs][kStatsWords] of one row (the slabs of a context; one "slab" for a batch member) -> the row; nx: cells
// per row of the whole grid
inline lbm_stats_row stats_row_from_words(const long long* words, int n_slabs, int nx) {
  constexpr int L = lbm_exact::kExactLimbs;
  long long sum[kStatsSums][L] = {};
  long long bad = 0;
  unsigned long long key = 0;
  for (int s = 0; s < n_slabs; s++) {
    const long long* w = words + (size_t)s * kStatsWords;
    for (int j = 0; j < kStatsSums; j++)
      for (int i = 0; i < L; i++) sum[j][i] += w[j * L + i];
    bad += w[kStatsBadWord];
    const unsigned long long k = (unsigned long long)w[kStatsKeyWord];
    if (k > key) key = k;
  }
  lbm_stats_row row;
  std::memset(&row, 0, sizeof(row));
  row.mass = lbm_exact::exact_sum_round(sum[0]);
  row.mom_x = lbm_exact::exact_sum_round(sum[1]);
  row.mom_y = lbm_exact::exact_sum_round(sum[2]);
  row.sum_u_sq = lbm_exact::exact_sum_round(sum[3]);
  row.nonfinite = bad;
  row.max_x = row.max_y = -1;
  if (key != 0) {
    const uint32_t bits = (uint32_t)(key >> 32);
    const uint32_t cell = 0xffffffffu - (uint32_t)(key & 0xffffffffull);
    std::memcpy(&row.max_u, &bits, sizeof(bits));
    row.max_x = (int)(cell % (uint32_t)nx);
    row.max_y = (int)(cell / (uint32_t)nx);
  }
  return row;
}

}  // namespace lbm_stats
