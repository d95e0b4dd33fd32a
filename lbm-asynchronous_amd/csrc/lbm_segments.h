// lbm_segments.h -- the segment loop of a checked run.  A run has n_seg segments, each followed by a check whose verdict
// the host reads later: issue(index) enqueues segment `index` with its check and returns false when that failed;
// judge(index) waits for the verdict of segment `index`.  Up to `depth` segments are in flight: at depth 1 the host knows
// every verdict before it issues the next segment; at depth 2 one segment of look-ahead is enqueued behind the one being
// judged, and the caller drops it (issued > judged) when the verdict ends the run.
// No HIP, no allocation: any C++17 compiler builds it (tests/segments_check.cpp checks it without a GPU).
#pragma once

namespace lbm_segments {

enum Verdict { kGoOn, kStop /* the check has decided */, kBreak /* the work gave up, or the wait failed: nothing is decided */ };

struct Outcome {
  int issued;    // segments enqueued: 0 .. issued - 1, in order
  int judged;    // verdicts read: 0 .. judged - 1, in order; issued - judged is 0, or 1 at depth 2
  bool stopped;  // the last verdict was kStop
  bool failed;   // an issue failed: segment `issued` is not wholly enqueued, and nothing was judged after that
};

template <class Issue, class Judge>
Outcome run(int n_seg, int depth, Issue&& issue, Judge&& judge) {
  Outcome o = {0, 0, false, false};
  while (o.judged < n_seg && !o.stopped) {
    for (; o.issued < n_seg && o.issued - o.judged < depth; o.issued++) {
      o.failed = !issue(o.issued);
      if (o.failed) return o;
    }
    const Verdict v = judge(o.judged++);
    o.stopped = v == kStop;
    if (v == kBreak) break;
  }
  return o;
}

}  // namespace lbm_segments
