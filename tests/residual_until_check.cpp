// residual_until_check.cpp -- checks lbm-asynchronous_amd/csrc/lbm_residual_until.h (the verdict of a residual-steady run,
// as the check kernels take it) without a GPU (tests/test_residual_until_abi.py builds and feeds it).  Standard input holds
// runs: "<tol, double bits in hex> <patience> <check_every> <checks>", then per check two sums -- each "m" and m float bits
// in hex: the terms of dsq and of usq -- and "<non-finite cells> <key, hex>", then one line of what must hold after the
// check: "<sum_du_sq> <sum_u_sq> <last_rel> (double bits, hex) <stop word returned> <streak> <checks> <stop> <steady_step>".
// The words are filled as residual_gather fills them (exact_sum_add per term).  exact_sum_round_hd must give the bits of
// exact_sum_round and of the expected sums; until_check must return the expected word and leave the expected state, with
// the words of the check in `last` when the state moved and `last` untouched when it did not.  Exit status 0 when every
// check of every run does.
#include <cstdio>
#include <cstring>

#include "../lbm-asynchronous_amd/csrc/lbm_residual_until.h"

static_assert(sizeof(lbm_residual_steady_result) == 72, "lbm_residual_steady_result is 72 bytes");

static unsigned long long bits_of(double v) {
  unsigned long long b;
  std::memcpy(&b, &v, sizeof(b));
  return b;
}

int main() {
  using namespace lbm_residual;
  constexpr int L = lbm_exact::kExactLimbs;
  unsigned long long tol_bits;
  int patience, every, n_checks, runs = 0, checks = 0, failed = 0;
  while (std::scanf("%llx %d %d %d", &tol_bits, &patience, &every, &n_checks) == 4) {
    double tol;
    std::memcpy(&tol, &tol_bits, sizeof(tol));
    UntilState st;
    until_reset(st);
    for (int j = 1; j <= n_checks; j++, checks++) {
      long long words[kResidualWords] = {};
      for (int s = 0; s < kResidualSums; s++) {
        int m;
        if (std::scanf("%d", &m) != 1) return 2;
        long long acc[L] = {};
        for (int i = 0; i < m; i++) {
          unsigned bits;
          if (std::scanf("%x", &bits) != 1) return 2;
          if (!lbm_exact::exact_sum_finite(bits)) return 3;
          lbm_exact::exact_sum_add(acc, bits, 1);
        }
        for (int i = 0; i < L; i++) words[s * L + i] = acc[i];
      }
      unsigned long long key, want_du, want_u, want_rel;
      int want_code, want_streak, want_checks, want_stop, want_step;
      if (std::scanf("%lld %llx", &words[kResidualBadWord], &key) != 2) return 2;
      words[kResidualKeyWord] = (long long)key;
      if (std::scanf("%llx %llx %llx %d %d %d %d %d", &want_du, &want_u, &want_rel, &want_code, &want_streak, &want_checks, &want_stop,
                     &want_step) != 8)
        return 2;
      bool ok = true;
      for (int s = 0; s < kResidualSums; s++) {
        long long acc[L];
        for (int i = 0; i < L; i++) acc[i] = words[s * L + i];
        const unsigned long long got = bits_of(exact_sum_round_hd(words + s * L));
        ok = ok && got == bits_of(lbm_exact::exact_sum_round(acc)) && got == (s ? want_u : want_du);
        for (int i = 0; i < L; i++) acc[i] = -acc[i];  // and of the negated accumulator
        ok = ok && bits_of(exact_sum_round_hd(acc)) == bits_of(lbm_exact::exact_sum_round(acc));
      }
      const UntilState before = st;
      const int code = until_check(st, words, tol, patience, j * every);
      ok = ok && code == want_code && st.streak == want_streak && st.checks == want_checks && st.stop == want_stop &&
           st.steady_step == want_step && bits_of(st.last_rel) == want_rel;
      if (st.checks != before.checks)
        ok = ok && std::memcmp(st.last, words, sizeof(words)) == 0;
      else
        ok = ok && std::memcmp(&st, &before, sizeof(st)) == 0;
      if (!ok) {
        std::printf("run %d check %d: got %016llx %016llx rel %016llx word %d streak %d checks %d stop %d step %d, expected %016llx %016llx rel "
                    "%016llx word %d streak %d checks %d stop %d step %d\n",
                    runs, j, bits_of(exact_sum_round_hd(words)), bits_of(exact_sum_round_hd(words + L)), bits_of(st.last_rel), code, st.streak,
                    st.checks, st.stop, st.steady_step, want_du, want_u, want_rel, want_code, want_streak, want_checks, want_stop, want_step);
        failed++;
      }
    }
    runs++;
  }
  std::printf("%d runs, %d checks, %d failed\n", runs, checks, failed);
  return (failed || runs == 0) ? 1 : 0;
}
