// lbm_psi_row.h -- from the words psi_extrema leaves in a ring row to the lbm_psi_row the readers hand out
// (lbm_read_psi_rows, lbm_batch_read_psi_rows).  A slab (or a batch member) owns kPsiWords int64 words of a row,
// 8 words = 64 bytes:
//   0   the bits of the smallest psi (a double, already rounded) among its finite fluid cells,
//   1   the bits of the largest,
//   2   the GLOBAL cell index y * nx + x of the smallest -- of several cells with that psi the smallest index; -1: the slab
//       has no finite fluid cell (words 0 and 1 are then 0),
//   3   likewise of the largest,
//   4   its finite fluid cells,
//   5   its fluid cells that are not finite,
//   6, 7 unused.
// The slabs' candidates are compared as the kernels compare them: by value as doubles (+0.0 and -0.0 are equal; the exact
// sum never yields -0.0 and no candidate is a NaN), then by the smaller cell index -- the order of the slabs does not
// matter.  The counts are added.
// No HIP, no allocation: any C++17 compiler builds it (tests/psi_row_check.cpp checks it without a GPU).
#pragma once

#include <cstdint>
#include <cstring>

#include "../../include/lbm_hip.h"

namespace lbm_psi {

constexpr int kPsiMinWord = 0, kPsiMaxWord = 1, kPsiMinCellWord = 2, kPsiMaxCellWord = 3, kPsiFluidWord = 4, kPsiBadWord = 5;
constexpr int kPsiWords = 8;  // 64 bytes
static_assert(kPsiBadWord < kPsiWords, "a slab's words hold the two candidates and the two counts");

// is the candidate (v, cell) in front of (best, best_cell)?  sign = -1: the smaller value wins (the minimum), +1: the
// larger; equal values: the smaller cell.  best_cell < 0: there is no candidate yet.
inline bool psi_in_front(double v, long long cell, double best, long long best_cell, int sign) {
  if (best_cell < 0) return true;
  if (v != best) return sign < 0 ? v < best : v > best;
  return cell < best_cell;
}

// words[n_slabs][kPsiWords] of one row (the slabs of a context; one "slab" for a batch member) -> the row; nx: cells per
// row of the whole grid
inline lbm_psi_row psi_row_from_words(const long long* words, int n_slabs, int nx) {
  double best[2] = {0.0, 0.0};
  long long best_cell[2] = {-1, -1};
  long long fluid = 0, bad = 0;
  for (int s = 0; s < n_slabs; s++) {
    const long long* w = words + (size_t)s * kPsiWords;
    fluid += w[kPsiFluidWord];
    bad += w[kPsiBadWord];
    for (int j = 0; j < 2; j++) {
      const long long cell = w[kPsiMinCellWord + j];
      if (cell < 0) continue;
      double v;
      std::memcpy(&v, &w[kPsiMinWord + j], sizeof(v));
      if (psi_in_front(v, cell, best[j], best_cell[j], j == 0 ? -1 : +1)) {
        best[j] = v;
        best_cell[j] = cell;
      }
    }
  }
  lbm_psi_row row;
  std::memset(&row, 0, sizeof(row));
  row.psi_min = best_cell[0] < 0 ? 0.0 : best[0] + 0.0;  // (+ 0.0: a -0.0, which the exact sum never yields, would be stored as +0.0)
  row.psi_max = best_cell[1] < 0 ? 0.0 : best[1] + 0.0;
  row.nonfinite = bad;
  row.min_x = best_cell[0] < 0 ? -1 : (int)(best_cell[0] % nx);
  row.min_y = best_cell[0] < 0 ? -1 : (int)(best_cell[0] / nx);
  row.max_x = best_cell[1] < 0 ? -1 : (int)(best_cell[1] % nx);
  row.max_y = best_cell[1] < 0 ? -1 : (int)(best_cell[1] / nx);
  row.fluid = (int)fluid;
  row.reserved = 0;
  return row;
}

}  // namespace lbm_psi
