// psi_row_check.cpp -- checks lbm-asynchronous_amd/csrc/lbm_psi_row.h (the words psi_extrema leaves -> the lbm_psi_row of the
// readers) and lbm-asynchronous_amd/csrc/lbm_exact_round.h (exact_sum_round_hd, which psi_scan calls once per cell) on a
// machine without a GPU.  A program of its own: built plain and with -fsanitize=address,undefined, run directly.
//   rounding: exact_sum_round_hd must give the bits of lbm_exact::exact_sum_round for accumulators filled as the kernels
//     fill them (exact_sum_add of floats over the whole exponent range, running prefixes included), for totals that turn
//     negative, for limbs whose sum carries, for total cancellation, and for random limbs set directly.
//   rows: psi_row_from_words against a reference that sorts all candidates, for 1, 2, 3 and 8 slabs, random values, ties
//     between slabs, slabs without a finite fluid cell, no cell at all, a -0.0 candidate, cell indices near 2^32.
// Prints "<n> checks, <m> failed"; the exit status is 0 only when m == 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../lbm-asynchronous_amd/csrc/lbm_exact_round.h"
#include "../lbm-asynchronous_amd/csrc/lbm_psi_row.h"

namespace {

constexpr int L = lbm_exact::kExactLimbs;
long checks = 0, failed = 0;

uint64_t bits_of(double v) {
  uint64_t b;
  std::memcpy(&b, &v, sizeof(b));
  return b;
}
unsigned fbits(float v) {
  unsigned b;
  std::memcpy(&b, &v, sizeof(b));
  return b;
}

void same_rounding(const long long (&acc)[L], const char* what) {
  checks++;
  const uint64_t got = bits_of(lbm_exact::exact_sum_round_hd(acc)), want = bits_of(lbm_exact::exact_sum_round(acc));
  if (got != want) {
    failed++;
    std::printf("rounding (%s): exact_sum_round_hd %016llx, exact_sum_round %016llx\n", what, (unsigned long long)got, (unsigned long long)want);
  }
}

// a finite float with a random sign, mantissa and an exponent from the whole range (subnormals included)
float any_float(std::mt19937_64& rng) {
  const unsigned e = (unsigned)(rng() % 255u);  // 0 .. 254: never inf / nan
  const unsigned b = ((unsigned)(rng() & 1u) << 31) | (e << 23) | (unsigned)(rng() & 0x7fffffu);
  float v;
  std::memcpy(&v, &b, sizeof(v));
  return v;
}

void check_rounding() {
  std::mt19937_64 rng(20261020);
  // running prefixes of random terms, as a lane of psi_scan sees them
  for (int run = 0; run < 200; run++) {
    long long acc[L] = {};
    const int narrow = run % 4;  // 0: the whole exponent range; else a window of exponents, where the terms cancel and carry
    for (int i = 0; i < 200; i++) {
      float v = any_float(rng);
      if (narrow) {
        const unsigned e = 100u + (unsigned)(rng() % (unsigned)(8 * narrow));
        const unsigned b = (fbits(v) & 0x807fffffu) | (e << 23);
        std::memcpy(&v, &b, sizeof(v));
      }
      lbm_exact::exact_sum_add(acc, fbits(v), (rng() % 16u) ? 1 : 0);  // (sign 0: a cell that adds nothing)
      same_rounding(acc, "prefix");
    }
  }
  // the cancellation lattice's column: 2^60, 2^-60, -2^60
  {
    long long acc[L] = {};
    const float terms[3] = {0x1p60f, 0x1p-60f, -0x1p60f};
    const double want[3] = {0x1p60, 0x1p60, 0x1p-60};
    for (int i = 0; i < 3; i++) {
      lbm_exact::exact_sum_add(acc, fbits(terms[i]), 1);
      same_rounding(acc, "cancellation");
      checks++;
      if (bits_of(lbm_exact::exact_sum_round_hd(acc)) != bits_of(want[i])) {
        failed++;
        std::printf("cancellation: prefix %d is not %a\n", i, want[i]);
      }
    }
    lbm_exact::exact_sum_add(acc, fbits(-0x1p-60f), 1);
    same_rounding(acc, "total cancellation");
    checks++;
    if (bits_of(lbm_exact::exact_sum_round_hd(acc)) != 0u) {  // +0.0, never -0.0
      failed++;
      std::printf("total cancellation: not +0.0\n");
    }
  }
  // carries: many equal terms with 24 one-bits across two limbs; then the sum turns negative
  {
    long long acc[L] = {};
    const float v = 4.0f - 0x1p-22f;
    for (int i = 0; i < 5000; i++) {
      lbm_exact::exact_sum_add(acc, fbits(v), 1);
      if (i % 50 == 0) same_rounding(acc, "carries");
    }
    for (int i = 0; i < 10000; i++) {
      lbm_exact::exact_sum_add(acc, fbits(-v), 1);
      if (i % 50 == 0) same_rounding(acc, "negative total");
    }
  }
  // ties to even at every bit position: 2^k + 2^(k-53) (down to even) and 2^k + 2^(k-52) + 2^(k-53) (up to even)
  for (int k = 60; k < 250; k += 7) {
    for (int odd = 0; odd < 2; odd++) {
      long long acc[L] = {};
      auto set_bit = [&](int bit) { acc[bit >> 5] += 1LL << (bit & 31); };
      set_bit(k);
      set_bit(k - 53);
      if (odd) set_bit(k - 52);
      same_rounding(acc, "tie");
      for (int i = 0; i < L; i++) acc[i] = -acc[i];
      same_rounding(acc, "negative tie");
    }
  }
  // random limbs set directly, within the 2^31-term bound, mixed signs
  for (int run = 0; run < 20000; run++) {
    long long acc[L];
    const int top = (int)(rng() % (unsigned)L);
    for (int i = 0; i < L; i++) {
      const long long v = (long long)(rng() >> (2 + rng() % 60u));
      acc[i] = i > top ? 0 : ((rng() & 1u) ? -v : v);
    }
    same_rounding(acc, "random limbs");
  }
}

struct Cand {
  double v;
  long long cell;
};

// the row the definition asks for: all candidates in one list
lbm_psi_row reference_row(const std::vector<Cand>& lo, const std::vector<Cand>& hi, long long fluid, long long bad, int nx) {
  lbm_psi_row row;
  std::memset(&row, 0, sizeof(row));
  row.min_x = row.min_y = row.max_x = row.max_y = -1;
  row.fluid = (int)fluid;
  row.nonfinite = bad;
  if (!lo.empty()) {
    const Cand m = *std::min_element(lo.begin(), lo.end(), [](const Cand& a, const Cand& b) { return a.v < b.v || (a.v == b.v && a.cell < b.cell); });
    row.psi_min = m.v == 0.0 ? 0.0 : m.v;
    row.min_x = (int)(m.cell % nx);
    row.min_y = (int)(m.cell / nx);
  }
  if (!hi.empty()) {
    const Cand m = *std::min_element(hi.begin(), hi.end(), [](const Cand& a, const Cand& b) { return a.v > b.v || (a.v == b.v && a.cell < b.cell); });
    row.psi_max = m.v == 0.0 ? 0.0 : m.v;
    row.max_x = (int)(m.cell % nx);
    row.max_y = (int)(m.cell / nx);
  }
  return row;
}

void same_row(const lbm_psi_row& got, const lbm_psi_row& want, const char* what) {
  checks++;
  const bool ok = bits_of(got.psi_min) == bits_of(want.psi_min) && bits_of(got.psi_max) == bits_of(want.psi_max) &&
                  got.nonfinite == want.nonfinite && got.min_x == want.min_x && got.min_y == want.min_y && got.max_x == want.max_x &&
                  got.max_y == want.max_y && got.fluid == want.fluid && got.reserved == 0;
  if (!ok) {
    failed++;
    std::printf("row (%s): got %a %a %lld (%d,%d) (%d,%d) %d, want %a %a %lld (%d,%d) (%d,%d) %d\n", what, got.psi_min, got.psi_max, got.nonfinite,
                got.min_x, got.min_y, got.max_x, got.max_y, got.fluid, want.psi_min, want.psi_max, want.nonfinite, want.min_x, want.min_y,
                want.max_x, want.max_y, want.fluid);
  }
}

void put(long long* w, double lo, long long lo_cell, double hi, long long hi_cell, long long fluid, long long bad) {
  std::memset(w, 0, lbm_psi::kPsiWords * sizeof(long long));
  if (lo_cell >= 0) std::memcpy(&w[lbm_psi::kPsiMinWord], &lo, sizeof(lo));
  if (hi_cell >= 0) std::memcpy(&w[lbm_psi::kPsiMaxWord], &hi, sizeof(hi));
  w[lbm_psi::kPsiMinCellWord] = lo_cell;
  w[lbm_psi::kPsiMaxCellWord] = hi_cell;
  w[lbm_psi::kPsiFluidWord] = fluid;
  w[lbm_psi::kPsiBadWord] = bad;
}

void check_rows() {
  static_assert(sizeof(lbm_psi_row) == 48, "lbm_psi_row is 48 bytes");
  std::mt19937_64 rng(7);
  const int slab_counts[4] = {1, 2, 3, 8};
  const double values[6] = {-0.25, 0.0, 0x1p-60, 3.5, -0x1p60, 0.125};  // few values: ties between slabs are common
  for (int run = 0; run < 4000; run++) {
    const int n_slabs = slab_counts[run % 4], nx = 1 + (int)(rng() % 300u);
    std::vector<long long> words((size_t)n_slabs * lbm_psi::kPsiWords);
    std::vector<Cand> lo, hi;
    long long fluid = 0, bad = 0;
    for (int s = 0; s < n_slabs; s++) {
      const bool none = rng() % 4u == 0;
      const Cand a = {values[rng() % 6u], (long long)(rng() % 5000u)}, b = {values[rng() % 6u], (long long)(rng() % 5000u)};
      const long long f = none ? 0 : 1 + (long long)(rng() % 1000u), n = (long long)(rng() % 3u);
      put(&words[(size_t)s * lbm_psi::kPsiWords], a.v, none ? -1 : a.cell, b.v, none ? -1 : b.cell, f, n);
      if (!none) {
        lo.push_back(a);
        hi.push_back(b);
      }
      fluid += f;
      bad += n;
    }
    same_row(lbm_psi::psi_row_from_words(words.data(), n_slabs, nx), reference_row(lo, hi, fluid, bad, nx), "random");
  }
  long long w[3 * lbm_psi::kPsiWords];
  // no finite fluid cell anywhere: 0 at -1, -1
  for (int s = 0; s < 3; s++) put(w + s * lbm_psi::kPsiWords, 0.0, -1, 0.0, -1, 0, 5 + s);
  same_row(lbm_psi::psi_row_from_words(w, 3, 64), reference_row({}, {}, 0, 18, 64), "nothing finite");
  // a tie between slabs, given in descending order of the cells: the smallest cell, 130
  put(w, 0.5, 700, 0.5, 700, 2, 0);
  put(w + lbm_psi::kPsiWords, 0.5, 130, 0.5, 131, 2, 0);
  put(w + 2 * lbm_psi::kPsiWords, 0.5, 4000, 0.5, 130, 1, 0);
  {
    const lbm_psi_row r = lbm_psi::psi_row_from_words(w, 3, 64);
    same_row(r, reference_row({{0.5, 700}, {0.5, 130}, {0.5, 4000}}, {{0.5, 700}, {0.5, 131}, {0.5, 130}}, 5, 0, 64), "tie");
    checks++;
    if (r.min_x != 2 || r.min_y != 2 || r.max_x != 2 || r.max_y != 2) {
      failed++;
      std::printf("tie: not cell 130\n");
    }
  }
  // +0.0 and -0.0 are equal: the smaller cell wins, and the row holds +0.0
  put(w, -0.0, 9, -0.0, 9, 1, 0);
  put(w + lbm_psi::kPsiWords, 0.0, 3, 0.0, 3, 1, 0);
  same_row(lbm_psi::psi_row_from_words(w, 2, 4), reference_row({{-0.0, 9}, {0.0, 3}}, {{-0.0, 9}, {0.0, 3}}, 2, 0, 4), "signed zeros");
  put(w, -0.0, 1, -0.0, 1, 1, 0);
  same_row(lbm_psi::psi_row_from_words(w, 1, 4), reference_row({{0.0, 1}}, {{0.0, 1}}, 1, 0, 4), "a -0.0 is stored as +0.0");
  // cell indices near 2^32
  put(w, -1.0, 4294967294LL, 2.0, 4294967295LL, 7, 1);
  same_row(lbm_psi::psi_row_from_words(w, 1, 65536), reference_row({{-1.0, 4294967294LL}}, {{2.0, 4294967295LL}}, 7, 1, 65536), "large cells");
}

}  // namespace

int main() {
  check_rounding();
  check_rows();
  std::printf("%ld checks, %ld failed\n", checks, failed);
  return failed == 0 ? 0 : 1;
}
