// ring_check.cpp -- checks lbm-asynchronous_amd/csrc/lbm_ring.h ("the n oldest waiting records lie in at most two runs of
// the ring") without a GPU (tests/test_ring_abi.py builds and runs it).  Against the brute-force list (read + i) % slots,
// i = 0 .. n - 1: exhaustively for rings of 1 .. 5 slots, every read % slots and every n from 0 to slots, with `read`
// small, a multiple of the ring further on and beyond 2^31 (the counters are 64-bit); every case with records of 0 .. 3
// words, copied run by run as the readers copy them.  Exit status 0 when every case holds.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lbm-asynchronous_amd/csrc/lbm_ring.h"

static int check(long long read, int slots, int n, size_t words) {
  const lbm_ring::Runs runs = lbm_ring::oldest_runs(read, slots, n);
  if (runs.n < 0 || runs.n > 2) return 1;                    // never more than two runs
  if ((n == 0) != (runs.n == 0)) return 2;                   // no record, no run
  if (runs.n == 2 && runs.run[1].first != 0) return 3;       // the second run starts at slot 0
  // the runs cover exactly the n oldest slots, in order
  std::vector<size_t> want, got;
  for (int i = 0; i < n; i++) want.push_back((size_t)((read + i) % slots));
  for (int j = 0; j < runs.n; j++) {
    const lbm_ring::Run& run = runs.run[j];
    if (run.count < 1 || run.at != (int)got.size() || run.first + (size_t)run.count > (size_t)slots) return 4;
    for (int i = 0; i < run.count; i++) got.push_back(run.first + (size_t)i);
  }
  if (got != want) return 5;
  // the copy the readers make: slot s of the ring holds `words` words s * 8 + w (none: a record of zero words is harmless)
  std::vector<long long> ring((size_t)slots * words), dst((size_t)n * words, -1);
  for (size_t s = 0; s < (size_t)slots; s++)
    for (size_t w = 0; w < words; w++) ring[s * words + w] = (long long)(s * 8 + w);
  for (int j = 0; j < runs.n; j++) {
    const lbm_ring::Run& run = runs.run[j];
    const size_t bytes = (size_t)run.count * words * sizeof(long long);
    if (bytes) std::memcpy(dst.data() + (size_t)run.at * words, ring.data() + run.first * words, bytes);
  }
  for (int i = 0; i < n; i++)
    for (size_t w = 0; w < words; w++)
      if (dst[(size_t)i * words + w] != (long long)(want[(size_t)i] * 8 + w)) return 6;
  return 0;
}

int main() {
  int cases = 0, failed = 0;
  for (int slots = 1; slots <= 5; slots++)
    for (int first = 0; first < slots; first++)
      for (int n = 0; n <= slots; n++)
        for (size_t words = 0; words <= 3; words++) {
          const long long reads[] = {first, first + 7LL * slots, first + (1LL << 31) / slots * slots + (long long)slots,
                                     first + (1LL << 62) / slots * slots};
          for (long long read : reads) {
            if (read % slots != first) return 2;  // the case list itself
            const int why = check(read, slots, n, words);
            if (why) {
              std::printf("read %lld, %d slots, n %d, %zu words: check %d failed\n", read, slots, n, words, why);
              failed++;
            }
            cases++;
          }
        }
  // once well beyond 2^31 on a ring no power of two divides, with the slot worked out by hand: 3000000000 % 7 == 4
  {
    const lbm_ring::Runs runs = lbm_ring::oldest_runs(3000000000LL, 7, 6);
    const bool ok = runs.n == 2 && runs.run[0].first == 4 && runs.run[0].at == 0 && runs.run[0].count == 3 && runs.run[1].first == 0 &&
                    runs.run[1].at == 3 && runs.run[1].count == 3 && check(3000000000LL, 7, 6, 2) == 0;
    if (!ok) {
      std::printf("read 3000000000, 7 slots, n 6: wrong runs\n");
      failed++;
    }
    cases++;
  }
  std::printf("%d cases, %d failed\n", cases, failed);
  return (failed || cases == 0) ? 1 : 0;
}
