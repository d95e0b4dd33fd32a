// coarse_row_check.cpp -- checks lbm-asynchronous_amd/csrc/lbm_coarse_row.h (the coarse frames' geometry and "words ->
// frame") without a GPU (tests/test_coarse_abi.py builds and feeds it).  Standard input holds cases: "<slabs> <nx> <ny>
// <bx> <by>", then per slab "<row_first> <row_count>", then that slab's boxes in the order of its slot -- its whole box
// rows, then its partial ones, cx boxes each -- a box as five sums, a sum being "m" and m float bits in hex (the terms of
// rho, jx, jy, ux, uy of the slab's cells of the box), then "<fluid> <nonfinite>".  A slot is filled as coarse_gather
// fills it: exact_sum_add per term; a whole box rounded by line_words_from_sums into 6 words, a partial one as its limb
// and count words with the spare word left 0; every word at box_offset.  Standard output: per case "case <i>", per slab
// "slab <s> <first> <count> <whole_first> <whole_n> <partial 0> <partial 1> <slot words>", then per box of the frame,
// row-major, "<sum_rho> <sum_jx> <sum_jy> <sum_ux> <sum_uy> (double bits, hex) <fluid> <nonfinite>".
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lbm-asynchronous_amd/csrc/lbm_coarse_row.h"

static_assert(sizeof(lbm_profile_line) == 48, "lbm_profile_line is 48 bytes");

int main() {
  using namespace lbm_coarse;
  constexpr int L = lbm_exact::kExactLimbs, S = lbm_profile::kProfileSums, W = lbm_profile::kProfileWords;
  int slabs, nx, ny, bx, by, cases = 0;
  while (std::scanf("%d %d %d %d %d", &slabs, &nx, &ny, &bx, &by) == 5) {
    if (slabs < 1 || nx < 1 || ny < 1 || bx < 1 || by < 1 || bx > nx || by > ny) return 2;
    std::vector<int> row_first((size_t)slabs), row_count((size_t)slabs);
    std::vector<long long> words;
    std::printf("case %d\n", cases);
    for (int s = 0; s < slabs; s++) {
      if (std::scanf("%d %d", &row_first[(size_t)s], &row_count[(size_t)s]) != 2) return 2;
      if (row_first[(size_t)s] < 0 || row_count[(size_t)s] < 1 || row_first[(size_t)s] + row_count[(size_t)s] > ny) return 2;
      const SlabBoxRows g = slab_box_rows(nx, ny, bx, by, row_first[(size_t)s], row_count[(size_t)s]);
      std::printf("slab %d %d %d %d %d %d %d %zu\n", s, g.first, g.count, g.whole_first, g.whole_n, g.partial[0], g.partial[1], slot_words(g));
      if (g.whole_n + partial_rows(g) != g.count) return 4;
      std::vector<long long> slot(slot_words(g), -1);
      std::vector<char> written(slot.size(), 0);
      std::vector<int> order;  // the slab's box rows in slot order
      for (int i = 0; i < g.whole_n; i++) order.push_back(g.whole_first + i);
      for (int p = 0; p < partial_rows(g); p++) order.push_back(g.partial[p]);
      for (int Y : order)
        for (int X = 0; X < g.cx; X++) {
          long long acc[S][L] = {};
          for (int j = 0; j < S; j++) {
            int m;
            if (std::scanf("%d", &m) != 1) return 2;
            for (int i = 0; i < m; i++) {
              unsigned bits;
              if (std::scanf("%x", &bits) != 1) return 2;
              if (!lbm_exact::exact_sum_finite(bits)) return 3;
              lbm_exact::exact_sum_add(acc[j], bits, 1);
            }
          }
          long long fluid, bad;
          if (std::scanf("%lld %lld", &fluid, &bad) != 2) return 2;
          bool whole;
          const size_t at = box_offset(g, X, Y, &whole);
          const int n = whole ? kCoarseLineWords : W;
          if (at + (size_t)n > slot.size()) return 5;  // the layout keeps every box inside the slot ...
          for (int i = 0; i < n; i++) {
            if (written[at + (size_t)i]) return 6;  // ... and no two boxes share a word
            written[at + (size_t)i] = 1;
          }
          if (whole) {
            long long line[kCoarseLineWords];
            line_words_from_sums(acc, (int)fluid, (int)bad, line);
            std::memcpy(&slot[at], line, sizeof(line));
          } else {
            for (int j = 0; j < S; j++)
              for (int i = 0; i < L; i++) slot[at + (size_t)(j * L + i)] = acc[j][i];
            slot[at + lbm_profile::kProfileFluidWord] = fluid;
            slot[at + lbm_profile::kProfileBadWord] = bad;
            slot[at + W - 1] = 0;
          }
        }
      for (char w : written)
        if (!w) return 7;  // ... and the boxes fill it
      words.insert(words.end(), slot.begin(), slot.end());
    }
    const size_t boxes = (size_t)coarse_boxes(nx, bx) * (size_t)coarse_boxes(ny, by);
    std::vector<lbm_profile_line> out(boxes);
    std::memset(out.data(), 0xff, boxes * sizeof(lbm_profile_line));
    coarse_frame_from_words(words.data(), slabs, row_first.data(), row_count.data(), nx, ny, bx, by, out.data());
    for (const lbm_profile_line& line : out) {
      const double sums[S] = {line.sum_rho, line.sum_jx, line.sum_jy, line.sum_ux, line.sum_uy};
      unsigned long long bits[S];
      std::memcpy(bits, sums, sizeof(bits));
      std::printf("%016llx %016llx %016llx %016llx %016llx %d %d\n", bits[0], bits[1], bits[2], bits[3], bits[4], line.fluid, line.nonfinite);
    }
    cases++;
  }
  return cases == 0 ? 1 : 0;
}
