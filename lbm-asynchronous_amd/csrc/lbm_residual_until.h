// lbm_residual_until.h -- the whole decision of a residual-steady run (lbm_run_until_residual and its batch twin): from
// the kResidualWords words residual_gather left for one lattice (lbm_residual_row.h) to the two exactly rounded sums,
// r_j = sqrt(sum_du_sq / sum_u_sq), the streak, the stop word and the words of the last check.  The check kernels
// (residual_check, residual_check_batch in lbm_kernels.hip.h) call until_check on the device; the host only forms rows
// from the words afterwards (residual_row_from_words).  One lattice is one "slab": nothing is merged.
// The sums are rounded by exact_sum_round_hd (lbm_exact_round.h), lbm_exact::exact_sum_round's twin for device code.
// No HIP, no allocation: any C++17 compiler builds it (tests/residual_until_check.cpp checks it without a GPU, against
// exact_sum_round and math.fsum); under hipcc the functions are also device functions.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "lbm_exact_sum.h"
#include "lbm_exact_round.h"
#include "lbm_residual_row.h"

namespace lbm_residual {

using lbm_exact::exact_sum_round_hd;  // (lbm_exact_round.h)

// the stop word of a run: what travels back to the host after a check
constexpr int kUntilGoOn = 0, kUntilSteady = 1, kUntilDiverged = 2;

// what the checks of one lattice have found so far; reset at the start of every call
struct UntilState {
  double last_rel;             // r_j of the last check (+inf before the first)
  int streak;                  // consecutive checks met
  int checks;                  // checks made
  int stop;                    // kUntilGoOn, or how the run ended: later checks change nothing
  int steady_step;             // steps of the call after which it became steady (-1: not)
  long long last[kResidualWords];  // the words of the last check (zeros before the first)
};
static_assert(sizeof(UntilState) == 24 + 8 * kResidualWords, "UntilState is copied between device and host as it is");

LBM_EXACT_HD void until_reset(UntilState& st) {
  st.last_rel = HUGE_VAL;
  st.streak = st.checks = 0;
  st.stop = kUntilGoOn;
  st.steady_step = -1;
  for (int i = 0; i < kResidualWords; i++) st.last[i] = 0;
}

// sqrt(sum_du_sq / sum_u_sq), both operations IEEE double; the corners are residual_l2's
LBM_EXACT_HD double until_rel(double sum_du_sq, double sum_u_sq) {
  if (sum_u_sq == 0.0) return sum_du_sq == 0.0 ? 0.0 : HUGE_VAL;
  return std::sqrt(sum_du_sq / sum_u_sq);
}

// One check, the sums already rounded (the kernels let two lanes round them): `words` are the kResidualWords words of the
// sample.  Returns the stop word this check set (kUntilGoOn when it set none, or when the run had stopped before).
LBM_EXACT_HD int until_verdict(UntilState& st, const long long* words, double sum_du_sq, double sum_u_sq, double tol, int patience,
                               int steps_after) {
  if (st.stop != kUntilGoOn) return kUntilGoOn;  // the verdict stands: the check of a look-ahead segment changes nothing
  st.checks += 1;
  st.last_rel = until_rel(sum_du_sq, sum_u_sq);
  for (int i = 0; i < kResidualWords; i++) st.last[i] = words[i];
  if (words[kResidualBadWord] > 0) {  // a fluid cell is not finite: the run has blown up
    st.streak = 0;
    st.stop = kUntilDiverged;
    return kUntilDiverged;
  }
  st.streak = (st.last_rel <= tol) ? st.streak + 1 : 0;
  if (st.streak >= patience) {
    st.stop = kUntilSteady;
    st.steady_step = steps_after;
    return kUntilSteady;
  }
  return kUntilGoOn;
}

// the same from the words alone
LBM_EXACT_HD int until_check(UntilState& st, const long long* words, double tol, int patience, int steps_after) {
  if (st.stop != kUntilGoOn) return kUntilGoOn;
  return until_verdict(st, words, exact_sum_round_hd(words), exact_sum_round_hd(words + lbm_exact::kExactLimbs), tol, patience,
                       steps_after);
}

}  // namespace lbm_residual
