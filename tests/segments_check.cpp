// segments_check.cpp -- checks lbm-asynchronous_amd/csrc/lbm_segments.h (the segment loop of a checked run: issue up to
// `depth` segments ahead, judge the oldest, end at the first stop, break or failed issue) without a GPU
// (tests/test_segments.py builds and runs it).  Exhaustively for n_seg 0 .. 6, depth 1 and 2, a stop at each index or
// never, a break at each index or never, a failing issue at each index or never: the calls the loop makes are recorded
// and compared with a brute-force list -- judge k stands behind issue min(k + depth - 1, n_seg - 1), cut at the first
// event that ends the run -- and the properties the engine relies on are checked on the record itself.  Exit status 0
// when every case holds.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../lbm-asynchronous_amd/csrc/lbm_segments.h"

struct Event {
  bool issue;  // else a judge
  int index;
  bool operator==(const Event& o) const { return issue == o.issue && index == o.index; }
};

// -1: never
static int check(int n_seg, int depth, int stop_at, int break_at, int fail_at) {
  const auto ends = [&](const Event& e) { return e.issue ? e.index == fail_at : (e.index == stop_at || e.index == break_at); };
  // the brute-force list: every issue and judge of a run that nothing ends, then the cut
  std::vector<Event> want;
  for (int k = 0, next = 0; k < n_seg; k++) {
    for (; next <= std::min(k + depth - 1, n_seg - 1); next++) want.push_back({true, next});
    want.push_back({false, k});
  }
  const auto cut = std::find_if(want.begin(), want.end(), ends);
  if (cut != want.end()) want.erase(cut + 1, want.end());

  std::vector<Event> got;
  bool over = false, late = false, crowded = false;
  int in_flight = 0;
  const lbm_segments::Outcome o = lbm_segments::run(
      n_seg, depth,
      [&](int index) {
        late |= over;
        crowded |= in_flight >= depth;  // with this issue more than `depth` would be in flight
        got.push_back({true, index});
        over = index == fail_at;
        if (!over) in_flight++;
        return !over;
      },
      [&](int index) {
        late |= over;
        got.push_back({false, index});
        in_flight--;
        over = ends(got.back());
        return index == stop_at ? lbm_segments::kStop : index == break_at ? lbm_segments::kBreak : lbm_segments::kGoOn;
      });
  if (late) return 1;     // nothing is issued or judged after the first stop, break or failure
  if (crowded) return 2;  // issued - judged never exceeds depth
  if (got != want) return 3;
  // issues and judges each come in index order, from 0, without gaps; the outcome counts them
  int issues = 0, judges = 0;
  for (const Event& e : got) {
    if (e.index != (e.issue ? issues : judges)) return 4;
    (e.issue ? issues : judges)++;
  }
  const bool failed = !got.empty() && got.back().issue && got.back().index == fail_at;
  if (o.failed != failed || o.issued != issues - (failed ? 1 : 0) || o.judged != judges) return 5;
  if (o.stopped != (!got.empty() && !got.back().issue && got.back().index == stop_at)) return 6;
  // what is left in flight for the caller to drop: nothing at depth 1, at most one segment at depth 2
  if (o.issued - o.judged < 0 || o.issued - o.judged > depth - 1) return 7;
  if (n_seg == 0 && !got.empty()) return 8;
  // a run that nothing ended judged every segment
  if (cut == want.end() && (o.issued != n_seg || o.judged != n_seg || o.stopped || o.failed)) return 9;
  return 0;
}

int main() {
  int cases = 0, failed = 0;
  for (int n_seg = 0; n_seg <= 6; n_seg++)
    for (int depth = 1; depth <= 2; depth++)
      for (int stop_at = -1; stop_at < n_seg; stop_at++)
        for (int break_at = -1; break_at < n_seg; break_at++)
          for (int fail_at = -1; fail_at < n_seg; fail_at++) {
            const int why = check(n_seg, depth, stop_at, break_at, fail_at);
            if (why) {
              std::printf("n_seg %d, depth %d, stop at %d, break at %d, failing issue %d: check %d failed\n", n_seg, depth, stop_at, break_at,
                          fail_at, why);
              failed++;
            }
            cases++;
          }
  std::printf("%d cases, %d failed\n", cases, failed);
  return (failed || cases == 0) ? 1 : 0;
}
