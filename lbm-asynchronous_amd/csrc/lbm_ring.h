// lbm_ring.h -- where the oldest records of a recorder's ring wait.  A ring has `slots` slots of one record each; record
// number k since arming (k = 0, 1, ...) lies in slot k % slots, `read` records have been drained, and a reader asks for
// the n oldest of those that wait (n <= written - read <= slots).  They lie in at most two runs of consecutive slots: from
// slot read % slots towards the ring's end, then on from slot 0.  The counters are 64-bit (a long run outlives 2^31
// records); slot numbers and counts fit an int, as `slots` does.
// No HIP, no allocation: any C++17 compiler builds it (tests/ring_check.cpp checks it without a GPU).
#pragma once

#include <cstddef>

namespace lbm_ring {

struct Run {
  size_t first;  // the run's first slot
  int at;        // which of the n records lies there (0: the oldest)
  int count;     // records in the run, one slot after the other
};
struct Runs {
  int n;  // 0 (no record asked for), 1 or 2
  Run run[2];
};

inline Runs oldest_runs(long long read, int slots, int n) {
  Runs r = {0, {{0, 0, 0}, {0, 0, 0}}};
  if (n <= 0 || slots <= 0) return r;
  const int first = (int)(read % slots);
  const int head = (n < slots - first) ? n : slots - first;  // up to the ring's end
  r.run[r.n++] = {(size_t)first, 0, head};
  if (head < n) r.run[r.n++] = {0, head, n - head};  // the rest, from slot 0 on
  return r;
}

}  // namespace lbm_ring
