// lbm_coarse_row.h -- the geometry of the coarse frames (lbm_set_coarse_frames, lbm_read_coarse) and the way from the
// words coarse_gather leaves in a slab's slot to the lbm_profile_line[cy][cx] frame the readers hand out.
// Boxes of bx x by cells tile the GLOBAL grid from cell (0, 0): cx = ceil(nx / bx) by cy = ceil(ny / by) boxes, box row Y
// covers the rows [Y * by, min(ny, (Y + 1) * by)); the last box of an axis may be ragged, nothing wraps.
// A slab (or a batch member) owns the rows [row_first, row_first + rows).  A box row that lies in them completely is a
// WHOLE box row of the slab: the kernel rounds its boxes on the device and stores each as its 48-byte lbm_profile_line
// (kCoarseLineWords = 6 words: the five doubles, then fluid in the low and nonfinite in the high half of the sixth).  A
// box row the slab shares with its neighbours is a PARTIAL box row: only the slab's first and / or last box row can be
// one (the two are the same row where by exceeds the slab's rows), and there the slab stores the box's kProfileWords
// limb words of lbm_profile_row.h; the reader adds the slabs' limbs as integers -- in any order -- before the one rounding.
// A slab's slot: [whole box rows][cx] lines of 6 words, then [0, 1 or 2 partial box rows][cx] of 48 words.
// No HIP: any C++17 compiler builds it (tests/coarse_row_check.cpp checks it without a GPU); under hipcc the geometry's
// functions are also device functions, and the launch code and the reader both use them.  Only the reader's
// coarse_frame_from_words allocates: the slabs' geometry, once per frame.
#pragma once

#include <cstddef>
#include <cstring>
#include <vector>

#include "lbm_exact_round.h"
#include "lbm_profile_row.h"

namespace lbm_coarse {

constexpr int kCoarseLineWords = 6;  // sizeof(lbm_profile_line) / 8
static_assert(sizeof(lbm_profile_line) == kCoarseLineWords * sizeof(long long), "a rounded box is its line, word for word");

constexpr int coarse_boxes(int n, int b) { return (n + b - 1) / b; }  // cx of (nx, bx), cy of (ny, by)

// what a slab holds of the coarse grid
struct SlabBoxRows {
  int bx, by, cx;
  int ny;                    // rows of the global grid
  int row_first, rows;       // the slab's GLOBAL rows
  int first, count;          // the box rows that touch the slab: first .. first + count - 1
  int whole_first, whole_n;  // ... those it owns completely (whole_n may be 0)
  int partial[2];            // ... and the partial ones in slot order, -1: none (partial[1] >= 0 only if partial[0] >= 0)
};

// the first and the one-past-last GLOBAL row of box row Y
LBM_EXACT_HD int box_row_begin(const SlabBoxRows& g, int Y) { return Y * g.by; }
LBM_EXACT_HD int box_row_end(const SlabBoxRows& g, int Y) { return (Y + 1) * g.by < g.ny ? (Y + 1) * g.by : g.ny; }

inline SlabBoxRows slab_box_rows(int nx, int ny, int bx, int by, int row_first, int rows) {
  SlabBoxRows g;
  g.bx = bx;
  g.by = by;
  g.cx = coarse_boxes(nx, bx);
  g.ny = ny;
  g.row_first = row_first;
  g.rows = rows;
  g.first = row_first / by;
  const int last = (row_first + rows - 1) / by;
  g.count = last - g.first + 1;
  const bool first_partial = box_row_begin(g, g.first) < row_first || box_row_end(g, g.first) > row_first + rows;
  const bool last_partial = last != g.first && box_row_end(g, last) > row_first + rows;
  g.whole_first = g.first + (first_partial ? 1 : 0);
  g.whole_n = g.count - (first_partial ? 1 : 0) - (last_partial ? 1 : 0);
  g.partial[0] = first_partial ? g.first : (last_partial ? last : -1);
  g.partial[1] = (first_partial && last_partial) ? last : -1;
  return g;
}

LBM_EXACT_HD int partial_rows(const SlabBoxRows& g) { return (g.partial[0] >= 0 ? 1 : 0) + (g.partial[1] >= 0 ? 1 : 0); }

// words of the slab's slot, and where its partial box rows start
LBM_EXACT_HD size_t seam_offset(const SlabBoxRows& g) { return (size_t)g.whole_n * (size_t)g.cx * kCoarseLineWords; }
LBM_EXACT_HD size_t slot_words(const SlabBoxRows& g) {
  return seam_offset(g) + (size_t)partial_rows(g) * (size_t)g.cx * lbm_profile::kProfileWords;
}

// Where box (X, Y) of a box row that touches the slab goes in its slot; *whole says which form: 6 words of a line, or
// kProfileWords limb words.
LBM_EXACT_HD size_t box_offset(const SlabBoxRows& g, int X, int Y, bool* whole) {
  if (Y >= g.whole_first && Y < g.whole_first + g.whole_n) {
    *whole = true;
    return ((size_t)(Y - g.whole_first) * (size_t)g.cx + (size_t)X) * kCoarseLineWords;
  }
  *whole = false;
  const int p = (Y == g.partial[0]) ? 0 : 1;
  return seam_offset(g) + ((size_t)p * (size_t)g.cx + (size_t)X) * lbm_profile::kProfileWords;
}

// limbs and counts -> the six words of the box's line, the bits of lbm_profile::profile_line_from_sums (exact_sum_round_hd
// gives exact_sum_round's bits): what the head lane of coarse_gather stores of a whole box
LBM_EXACT_HD void line_words_from_sums(const long long (&sum)[lbm_profile::kProfileSums][lbm_exact::kExactLimbs], int fluid, int bad,
                                       long long (&line)[kCoarseLineWords]) {
  for (int j = 0; j < lbm_profile::kProfileSums; j++) {
    const double v = lbm_exact::exact_sum_round_hd(sum[j]);
    std::memcpy(&line[j], &v, sizeof(v));
  }
  line[lbm_profile::kProfileSums] = (long long)(((unsigned long long)(unsigned)bad << 32) | (unsigned long long)(unsigned)fluid);
}

// One frame.  words: the slabs' slots one after the other; row_first[s], row_count[s]: the GLOBAL rows slab s owns
// (together the rows 0 .. ny - 1, each once).  out: cy * cx lines, row-major.
inline void coarse_frame_from_words(const long long* words, int n_slabs, const int* row_first, const int* row_count, int nx, int ny, int bx,
                                    int by, lbm_profile_line* out) {
  constexpr int L = lbm_exact::kExactLimbs, S = lbm_profile::kProfileSums;
  const int cx = coarse_boxes(nx, bx), cy = coarse_boxes(ny, by);
  std::vector<SlabBoxRows> geometry((size_t)n_slabs);  // every slab's, and where its slot starts, once
  std::vector<size_t> slot_at((size_t)n_slabs);
  size_t at = 0;
  for (int s = 0; s < n_slabs; s++) {
    geometry[(size_t)s] = slab_box_rows(nx, ny, bx, by, row_first[s], row_count[s]);
    slot_at[(size_t)s] = at;
    at += slot_words(geometry[(size_t)s]);
  }
  for (int Y = 0; Y < cy; Y++) {
    for (int X = 0; X < cx; X++) {
      long long sum[S][L] = {};
      long long fluid = 0, bad = 0;
      bool rounded = false;
      for (int s = 0; s < n_slabs && !rounded; s++) {
        const SlabBoxRows& g = geometry[(size_t)s];
        if (Y >= g.first && Y < g.first + g.count) {
          bool whole;
          const long long* w = words + slot_at[(size_t)s] + box_offset(g, X, Y, &whole);
          if (whole) {  // the one slab that owns the box row: its line as it is
            std::memcpy(&out[(size_t)Y * cx + X], w, sizeof(lbm_profile_line));
            rounded = true;
          } else {
            for (int j = 0; j < S; j++)
              for (int i = 0; i < L; i++) sum[j][i] += w[j * L + i];
            fluid += w[lbm_profile::kProfileFluidWord];
            bad += w[lbm_profile::kProfileBadWord];
          }
        }
      }
      if (!rounded) out[(size_t)Y * cx + X] = lbm_profile::profile_line_from_sums(sum, fluid, bad);
    }
  }
}

}  // namespace lbm_coarse
