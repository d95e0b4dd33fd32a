// lbm_exact_round.h -- exact_sum_round_hd, lbm_exact::exact_sum_round's twin for device code: the same integer steps with
// the top bit found by count-leading-zeros and the kept bits cut out of three digits, instead of loops over single bits;
// the same bits.  Two users: the check kernels of a residual-steady run (lbm_residual_until.h), which round two sums per
// sample, and the stream function's scan (psi_scan in lbm_kernels.hip.h), which rounds a column's running sum once per cell.
// No HIP, no allocation: any C++17 compiler builds it (tests/residual_until_check.cpp and tests/psi_row_check.cpp check it
// without a GPU, against exact_sum_round); under hipcc the function is also a device function.
#pragma once

#include <cstdint>
#include <cstring>

#include "lbm_exact_sum.h"

namespace lbm_exact {

// the value of an accumulator (lbm_exact_sum.h: kExactLimbs int64 limbs, limb j in units of 2^(32 j - 149)) rounded to
// the nearest double, ties to even
LBM_EXACT_HD double exact_sum_round_hd(const long long* acc) {
  constexpr int L = kExactLimbs;
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

}  // namespace lbm_exact
