// lbm_exact_sum.h -- the exact sum of signed floats, as the obstacle forces (lbm_set_forces) take it: a fixed-point
// accumulator wide enough for every finite float, so that the sum has no rounding until it is converted to a double,
// once, to nearest-even.  Integer additions commute: the result does not depend on the order of the terms, on how they
// were dealt to lanes, workgroups or slabs, or on which partial accumulators were added first.
//
// A finite float is m * 2^(q - 149) with an integer |m| < 2^24 and q in 0..253 (q = max(biased exponent, 1) - 1).
// Limb j of an accumulator counts units of 2^(32 j - 149): a term adds the low 32 bits of m << (q % 32) to limb q / 32
// and the (signed) rest to limb q / 32 + 1.  One term moves a limb by less than 2^32, so an int64 limb takes 2^31 terms
// without carries; carries are resolved once, by exact_sum_round.  kExactLimbs = 9 limbs reach 2^(32*8 + 55 - 149).
// No HIP, no allocation: any C++17 compiler builds it (tests/forces_sum_check.cpp checks it without a GPU); under hipcc
// the functions are also device functions, and force_gather (lbm_kernels.hip.h) accumulates with exact_sum_add.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LBM_EXACT_HD __host__ __device__ __forceinline__
#else
#define LBM_EXACT_HD inline
#endif

namespace lbm_exact {

constexpr int kExactLimbs = 9;

// acc += sign * f for a finite f given by its bits; sign in {-1, 0, +1}.  The limb is selected by compares over a
// constant trip count, so an accumulator held in registers stays there.
LBM_EXACT_HD void exact_sum_add(long long (&acc)[kExactLimbs], unsigned bits, int sign) {
  const unsigned e = (bits >> 23) & 0xffu;
  const int mant = (int)(bits & 0x7fffffu) | (e ? 0x800000 : 0);
  const int q = e ? (int)e - 1 : 0;
  const int m = ((bits >> 31) ? -mant : mant) * sign;
  const long long v = (long long)m * (1LL << (q & 31));  // |v| < 2^55
  const long long lo = v & 0xffffffffLL, hi = v >> 32;   // v = hi * 2^32 + lo, 0 <= lo < 2^32
  const int j = q >> 5;                                  // 0..7
#pragma unroll
  for (int i = 0; i < kExactLimbs; i++) acc[i] += (i == j ? lo : 0LL) + (i == j + 1 ? hi : 0LL);
}

LBM_EXACT_HD bool exact_sum_finite(unsigned bits) { return ((bits >> 23) & 0xffu) != 0xffu; }

// the accumulated value rounded to the nearest double, ties to even (what math.fsum gives for the same terms)
inline double exact_sum_round(const long long (&acc)[kExactLimbs]) {
  // carries: digits[i] in [0, 2^32) for i < kExactLimbs, the rest (signed) on top
  uint64_t d[kExactLimbs + 1];
  bool negative = false;
  for (int pass = 0; pass < 2; pass++) {
    long long carry = 0;
    for (int i = 0; i < kExactLimbs; i++) {
      // (limb and carry are far from the int64 range: |limb| < 2^63 / 2 by the 2^31-term bound, |carry| < 2^32)
      const long long t = (negative ? -acc[i] : acc[i]) + carry;
      d[i] = (uint64_t)(t & 0xffffffffLL);
      carry = t >> 32;
    }
    if (carry >= 0) {
      d[kExactLimbs] = (uint64_t)carry;
      break;
    }
    negative = true;  // the value is negative: convert its magnitude
  }
  auto bit = [&](int i) -> unsigned { return (unsigned)((d[i >> 5] >> (i & 31)) & 1u); };  // i < 32 * kExactLimbs
  int top = -1;  // highest set bit
  const int n_bits = 32 * kExactLimbs + 32;
  auto bit_any = [&](int i) -> unsigned {
    return i < 32 * kExactLimbs ? bit(i) : (unsigned)((d[kExactLimbs] >> (i - 32 * kExactLimbs)) & 1u);
  };
  for (int i = n_bits - 1; i >= 0; i--)
    if (bit_any(i)) {
      top = i;
      break;
    }
  if (top < 0) return 0.0;
  const int low = top > 52 ? top - 52 : 0;  // lowest bit kept
  uint64_t mant = 0;
  for (int i = top; i >= low; i--) mant = (mant << 1) | bit_any(i);
  if (low > 0) {
    const unsigned guard = bit_any(low - 1);
    unsigned sticky = 0;
    for (int i = low - 2; i >= 0 && !sticky; i--) sticky = bit_any(i);
    if (guard && (sticky || (mant & 1u))) mant++;  // (2^53 is exact in a double as well)
  }
  const double r = std::ldexp((double)mant, low - 149);
  return negative ? -r : r;
}

}  // namespace lbm_exact
