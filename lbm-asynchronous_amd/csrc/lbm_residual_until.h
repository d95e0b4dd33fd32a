// lbm_residual_until.h -- the whole decision of a residual-steady run (lbm_run_until_residual and its batch twin): from
// the kResidualWords words residual_gather left for one lattice (lbm_residual_row.h) to the two exactly rounded sums,
// r_j = sqrt(sum_du_sq / sum_u_sq), the streak, the stop word and the words of the last check.  The check kernels
// (residual_check, residual_check_batch in lbm_kernels.hip.h) call until_check on the device; the host only forms rows
// from the words afterwards (residual_row_from_words).  One lattice is one "slab": nothing is merged.
// exact_sum_round_hd is lbm_exact::exact_sum_round's twin for device code: the same integer steps with the top bit found
// by count-leading-zeros and the kept bits cut out of three digits, instead of loops over single bits; the same bits.
// No HIP, no allocation: any C++17 compiler builds it (tests/residual_until_check.cpp checks it without a GPU, against
// exact_sum_round and math.fsum); under hipcc the functions are also device functions.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "lbm_exact_sum.h"
#include "lbm_residual_row.h"

namespace lbm_residual {

// the value of an accumulator (lbm_exact_sum.h: kExactLimbs int64 limbs, limb j in units of 2^(32 j - 149)) rounded to
// the nearest double, ties to even
LBM_EXACT_HD double exact_sum_round_hd(const long long* acc) {
  constexpr int L = lbm_exact::kExactLimbs;
  // carries: d[i] in [0, 2^32) for i < L, the rest on top (d[L], non-negative after the sign is taken out); two zero
  // digits above, so that a window of three digits can start anywhere
  uint32_t d[L + 3];
  bool negative = false;
  for (int pass = 0; pass < 2; pass++) {
    long long carry = 0;
    for (int i = 0; i < L; i++) {
      const long long t = (negative ? -acc[i] : acc[i]) + carry;
      d[i] = (uint32_t)(t & 0xffffffffLL);
      carry = t >> 32;
    }
    if (carry >= 0) {
      d[L] = (uint32_t)carry;  // (|carry| < 2^32 by the 2^31-term bound of the limbs)
      break;
    }
    negative = true;  // the value is negative: convert its magnitude
  }
  d[L + 1] = d[L + 2] = 0u;
  int hi = L;
  while (hi >= 0 && d[hi] == 0u) hi--;
  if (hi < 0) return 0.0;
  const int top = 32 * hi + 31 - __builtin_clz(d[hi]);  // highest set bit
  const int low = top > 52 ? top - 52 : 0;              // lowest bit kept
  const int w = low >> 5, s = low & 31;
  const uint64_t lo64 = (uint64_t)d[w] | ((uint64_t)d[w + 1] << 32);
  const uint64_t window = s ? (lo64 >> s) | ((uint64_t)d[w + 2] << (64 - s)) : lo64;  // bits low .. low + 63
  uint64_t mant = window & ((1ull << (top - low + 1)) - 1ull);                        // bits low .. top, at most 53
  if (low > 0) {
    const int g = low - 1, gw = g >> 5, gs = g & 31;
    const unsigned guard = (d[gw] >> gs) & 1u;
    bool sticky = (d[gw] & ((1u << gs) - 1u)) != 0u;
    for (int i = 0; i < gw; i++) sticky = sticky || d[i] != 0u;
    if (guard && (sticky || (mant & 1ull))) mant++;  // (2^53 is exact in a double as well)
  }
  // mant * 2^(low - 149): both factors are doubles without rounding, and so is the product (exponents -149 .. 171)
  const uint64_t scale_bits = (uint64_t)(low - 149 + 1023) << 52;
  double scale;
  std::memcpy(&scale, &scale_bits, sizeof(scale));
  const double r = (double)mant * scale;
  return negative ? -r : r;
}

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
