// lbm_profile_row.h -- from the words profile_rows and profile_columns leave in a ring record to the lbm_profile_line
// array the readers hand out (lbm_read_profiles, lbm_batch_read_profiles).  A line owns kProfileWords int64 words:
//   [0, 9)    the fixed-point limbs (lbm_exact_sum.h) of the sum of rho over the line's finite fluid cells,
//   [9, 18)   of jx, [18, 27) of jy, [27, 36) of ux, [36, 45) of uy over the same cells,
//   45        the line's finite fluid cells,
//   46        its fluid cells that are not finite,
//   47        unused.
// A slab (or a batch member) owns, per record, the row lines of its owned rows (if LBM_PROFILE_ROWS is selected), then nx
// column lines (if LBM_PROFILE_COLUMNS is) that hold its own rows' share of every column.  A row line comes from the slab
// that owns the row; a column's limbs and counts are added over the slabs as integers -- the order of the slabs does not
// matter -- and each sum is rounded once.
// No HIP, no allocation: any C++17 compiler builds it (tests/profile_row_check.cpp checks it without a GPU).
#pragma once

#include <cstddef>
#include <cstring>

#include "lbm_exact_sum.h"
#include "../../include/lbm_hip.h"

namespace lbm_profile {

constexpr int kProfileSums = 5;  // rho, jx, jy, ux, uy
constexpr int kProfileFluidWord = kProfileSums * lbm_exact::kExactLimbs;  // 45
constexpr int kProfileBadWord = kProfileFluidWord + 1;                    // 46
constexpr int kProfileWords = 48;                                         // 384 bytes
static_assert(kProfileBadWord < kProfileWords, "a line's words hold the five accumulators and the two counts");

// lines of one slab's (or member's) share of a record, and of a whole record
constexpr size_t profile_slab_lines(int rows, int nx, int axes) {
  return (size_t)((axes & LBM_PROFILE_ROWS) ? rows : 0) + (size_t)((axes & LBM_PROFILE_COLUMNS) ? nx : 0);
}

// limbs and counts -> the line (limbs: kProfileSums accumulators)
inline lbm_profile_line profile_line_from_sums(const long long (&sum)[kProfileSums][lbm_exact::kExactLimbs], long long fluid, long long bad) {
  lbm_profile_line line;
  std::memset(&line, 0, sizeof(line));
  line.sum_rho = lbm_exact::exact_sum_round(sum[0]);
  line.sum_jx = lbm_exact::exact_sum_round(sum[1]);
  line.sum_jy = lbm_exact::exact_sum_round(sum[2]);
  line.sum_ux = lbm_exact::exact_sum_round(sum[3]);
  line.sum_uy = lbm_exact::exact_sum_round(sum[4]);
  line.fluid = (int)fluid;
  line.nonfinite = (int)bad;
  return line;
}

// One record.  words: the slabs' shares one after the other, slab s with profile_slab_lines(row_count[s], nx, axes) lines;
// row_first[s], row_count[s]: the GLOBAL rows slab s owns (together the rows 0 .. ny - 1, each once).  out: ny row lines
// (if selected), then nx column lines (if selected).
inline void profile_lines_from_words(const long long* words, int n_slabs, const int* row_first, const int* row_count, int nx, int ny, int axes,
                                     lbm_profile_line* out) {
  constexpr int L = lbm_exact::kExactLimbs;
  const bool rows = (axes & LBM_PROFILE_ROWS) != 0, columns = (axes & LBM_PROFILE_COLUMNS) != 0;
  lbm_profile_line* const out_columns = out + (rows ? ny : 0);
  auto add = [](long long (&sum)[kProfileSums][L], const long long* w) {
    for (int j = 0; j < kProfileSums; j++)
      for (int i = 0; i < L; i++) sum[j][i] += w[j * L + i];
  };
  if (rows) {
    const long long* share = words;
    for (int s = 0; s < n_slabs; s++) {
      for (int r = 0; r < row_count[s]; r++) {
        const long long* w = share + (size_t)r * kProfileWords;
        long long sum[kProfileSums][L] = {};
        add(sum, w);
        out[row_first[s] + r] = profile_line_from_sums(sum, w[kProfileFluidWord], w[kProfileBadWord]);
      }
      share += profile_slab_lines(row_count[s], nx, axes) * kProfileWords;
    }
  }
  if (columns) {
    for (int x = 0; x < nx; x++) {
      long long sum[kProfileSums][L] = {};
      long long fluid = 0, bad = 0;
      const long long* share = words;
      for (int s = 0; s < n_slabs; s++) {
        const long long* w = share + ((size_t)(rows ? row_count[s] : 0) + (size_t)x) * kProfileWords;
        add(sum, w);
        fluid += w[kProfileFluidWord];
        bad += w[kProfileBadWord];
        share += profile_slab_lines(row_count[s], nx, axes) * kProfileWords;
      }
      out_columns[x] = profile_line_from_sums(sum, fluid, bad);
    }
  }
}

}  // namespace lbm_profile
