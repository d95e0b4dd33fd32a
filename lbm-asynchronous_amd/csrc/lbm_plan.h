// lbm_plan.h -- which kernels advance a context and with what launch geometry: pure host arithmetic on the grid, the
// decomposition, the device's CU count and the LBM_* environment.  No HIP, no allocation, no output: any C++17 compiler
// builds it, and tests/plan_dump.cpp pins its answers against tests/golden/kernel_plans.json on a machine without a GPU.
// create_common (lbm_hip.hip) runs on plan_kernels' answer; the host-only query lbm_plan_halo_depth asks it too.
// All numbers in the comments were measured on MI355X (profiles/r01_tuning.md, r02_tuning.md, r03_tuning.md).
#pragma once

#include <cstdlib>

namespace lbm_plan {

constexpr int kMaxSlabs = 8;
constexpr int kMaxBandGroups = 3;  // interior streams of the band-group path: with the seam stream four in all
constexpr int kHaloRows = 4;  // halo rows kept below and above every slab (a K-step pass reads K rows beyond the slab)
constexpr int kMaskHalo = 3;  // mask rows kept beyond the slab: a K-step pass relaxes K-1 halo rows redundantly
constexpr int kBlock = 256;   // threads of a one-step workgroup (lbm::kBlock)
constexpr int kNoRow = -1000000;  // "no such row in this slab" (lbm::kNoRow)

// how the halo rows of a slab travel
enum HaloKind { HALO_SELF = 0, HALO_MEMCPY = 1, HALO_RCCL = 2, HALO_HOST = 3 };

// step_tile instantiations: own cells per workgroup (tw x th), halo depth = most timesteps per launch, threads
struct TileDims { int tw, th, kmax, threads; };
constexpr TileDims kTileDims[] = {
    {16, 8, 4, 384},   // 0: tiny grids: one thread per staged cell (24 x 16)
    {16, 8, 8, 768},   // 1: same, halo of 8
    {32, 16, 2, 640},  // 2..: larger tiles, less redundant halo work
    {32, 16, 3, 768},
    {32, 16, 4, 896},
    {64, 16, 2, 640},
    {64, 8, 2, 704},
};
constexpr int kTileShapeCount = (int)(sizeof(kTileDims) / sizeof(kTileDims[0]));

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
inline long round_up(long a, long b) { return (a + b - 1) / b * b; }

// ---- the environment: one knob, read once; its value where it has one, and whether it is set at all ------------------
struct Knob {
  bool set = false;        // the variable exists (an empty one too)
  bool has_value = false;  // ... and is not empty
  int number = 0;
  int value(int dflt) const { return has_value ? number : dflt; }
};
inline Knob env_knob(const char* name) {
  const char* v = getenv(name);
  return {v != nullptr, v && *v, (v && *v) ? atoi(v) : 0};
}
inline int env_int(const char* name, int dflt) { return env_knob(name).value(dflt); }

// every knob plan_kernels reads
struct Knobs {
  Knob vec4 = env_knob("LBM_VEC4"), fuse2 = env_knob("LBM_FUSE2"), lane_cells = env_knob("LBM_LANE_CELLS"),
       packed = env_knob("LBM_PACKED"), pass_steps = env_knob("LBM_PASS_STEPS"), neigh = env_knob("LBM_NEIGH"),
       nts = env_knob("LBM_NTS"), snake = env_knob("LBM_SNAKE"), graph = env_knob("LBM_GRAPH"),
       lds_windows = env_knob("LBM_LDS_WINDOWS"), prefetch = env_knob("LBM_PREFETCH"), xcd_chunk = env_knob("LBM_XCD_CHUNK"),
       stepk = env_knob("LBM_STEPK"), band_groups = env_knob("LBM_BAND_GROUPS"), band_rows = env_knob("LBM_BAND_ROWS"),
       band_max = env_knob("LBM_BAND_MAX"), tile_steps = env_knob("LBM_TILE_STEPS"), tile_shape = env_knob("LBM_TILE_SHAPE"),
       threads = env_knob("LBM_THREADS"), resident = env_knob("LBM_RESIDENT"), resident_rows = env_knob("LBM_RESIDENT_ROWS"),
       resident_joint = env_knob("LBM_RESIDENT_JOINT"), resident_one_xcd = env_knob("LBM_RESIDENT_ONE_XCD"),
       resident_group = env_knob("LBM_RESIDENT_GROUP"), resident_min_steps = env_knob("LBM_RESIDENT_MIN_STEPS"),
       resident_timeout_ms = env_knob("LBM_RESIDENT_TIMEOUT_MS");
  // the selection knobs: asking for another kernel by any of them leaves the resident kernel off unless LBM_RESIDENT=1
  // says otherwise
  bool selects_a_kernel() const {
    return fuse2.set || vec4.set || tile_steps.set || tile_shape.set || lane_cells.set || pass_steps.set || packed.set ||
           band_rows.set || graph.set || stepk.set || lds_windows.set || prefetch.set || xcd_chunk.set || neigh.set ||
           snake.set || nts.set;
  }
};

// ---- what is planned for ------------------------------------------------------------------------------------------
struct PlanInput {
  int nx = 0, ny = 0;
  int world = 1, rank = 0;  // processes sharing the grid, and which of them this is (its rows: row_span(ny, world, rank))
  int n_slabs = 1;          // row slabs of this process
  int halo = HALO_SELF;     // HaloKind
  int cus = 0;              // CUs of slab 0's device (0: unknown -- no resident kernel)
  int n_devices = 1;
  bool distinct_devices = false;  // several slabs, each on a device of its own
};

struct KernelPlan {
  bool vec4 = false;
  int neigh = 0;  // step_vec4 NEIGH flavour (LBM_NEIGH overrides)
  int nts = 1;    // nontemporal stores (LBM_NTS overrides)
  int snake = 0;  // alternate the sweep direction every step (LBM_SNAKE overrides)
  int fuse2 = 0;  // several timesteps per pass over memory (the stream kernels) where the slabs allow it
  int pass_steps = 2;  // ... how many: 2 or 3 (LBM_PASS_STEPS)
  int lane_cells = 4;  // cells per lane in step2_stream (4 or 2; LBM_LANE_CELLS)
  int halo_lanes = 1;  // stream kernel: lanes at each end of a wave that only feed their neighbours
  int n_strips = 0;    // stream kernel geometry: waves across x
  int packed = 0;      // stream kernel: collision on pairs of cells, v_pk_* instructions (LBM_PACKED)
  int lds_windows = 0; // packed stream kernel: how many of the K-1 sliding windows live in LDS (LBM_LDS_WINDOWS, 0..2)
  int prefetch = 0;    // stream kernel: request the next row before relaxing the current one (LBM_PREFETCH)
  int xcd_chunk = 0;   // stream kernel: strips per XCD chunk (LBM_XCD_CHUNK; 0 = plain workgroup order)
  int use_stepk = 0;   // two-step passes through stepk_stream<K=2> instead of step2_stream (LBM_STEPK; experiments)
  int band_groups = 1; // single periodic slab: full-depth passes as this many band groups (LBM_BAND_GROUPS)
  int band_rows = 8;   // stream kernel geometry: band height
  int tile_steps = 0;  // > 0: single slab advanced by the LDS-tile kernel, this many steps per launch
  int tile_shape = 0;  // index into kTileDims
  long part_stride = 0;  // floats between the partial-sum slots of a slab: the most workgroups any launch has, rounded up
  int use_graph = 0;   // replay chunks of an even number of passes + their reduce as one hipGraph each
  int want_team = 0;   // one issuing host thread per slab
  int resident = 0;             // single periodic slab that fits the chip's registers: lbm_run calls of at least
  int resident_min_steps = 16;  // ... this many timesteps run as launches of the resident kernel (lbm::resident_band)
  int resident_bands = 0;       // its workgroups (bands of resident_rows rows)
  int resident_joint = 0;       // narrow grids: both pairs of a lane relaxed as one block behind the halo wait
  int resident_rows = 4;        // rows per band: 4, or 2 where the chip has CUs to spare (one pair per lane)
  int resident_group = 1;       // bands per workgroup
  int resident_one_xcd = 0;     // all workgroups on one XCD (8 x the workgroups launched, 7 of 8 leave at once)
  long long resident_timeout = 0;  // bound of one halo wait, wall-clock ticks
};

// two plans launch the resident kernel alike (the members of a batch must)
inline bool same_resident_launch(const KernelPlan& a, const KernelPlan& b) {
  return a.resident == b.resident && a.resident_bands == b.resident_bands && a.resident_group == b.resident_group &&
         a.resident_one_xcd == b.resident_one_xcd && a.resident_rows == b.resident_rows;
}
// the plan with its resident candidate withdrawn (the device's occupancy query refused it)
inline KernelPlan without_resident(KernelPlan pl) {
  const KernelPlan none;
  pl.resident = none.resident;
  pl.resident_min_steps = none.resident_min_steps;
  pl.resident_bands = none.resident_bands;
  pl.resident_joint = none.resident_joint;
  pl.resident_rows = none.resident_rows;
  pl.resident_group = none.resident_group;
  pl.resident_one_xcd = none.resident_one_xcd;
  pl.resident_timeout = none.resident_timeout;
  return pl;
}

// ---- rows ---------------------------------------------------------------------------------------------------------
// part `index` of `parts` of ny rows: balanced blocks, the first ny % parts parts get one row more (lbm_partition_rows
// checks the arguments)
struct RowSpan { int first, count; };
inline RowSpan row_span(int ny, int parts, int index) {
  const int base = ny / parts, rem = ny % parts;
  return {index * base + (index < rem ? index : rem), base + (index < rem ? 1 : 0)};
}

// workgroups of a one-step launch over n_rows rows
inline int blocks_for_rows(bool vec4, int nx, int n_rows) {
  if (n_rows <= 0) return 0;
  return vec4 ? ceil_div((long)(nx / 4) * n_rows, kBlock) : ceil_div((long)nx * n_rows, kBlock);
}
// workgroups of an LDS-tile launch over `rows` rows
inline int tile_count(int nx, int rows, int shape) {
  return ceil_div(nx, kTileDims[shape].tw) * ceil_div(rows, kTileDims[shape].th);
}
// band groups: rows [lo, hi) of group g of `groups` over a slab of `rows` rows; returns the group height H (the last
// group also takes the remainder)
inline int group_rows(int rows, int groups, int g, int* lo, int* hi) {
  const int h = rows / groups;
  *lo = g * h;
  *hi = (g == groups - 1) ? rows : *lo + h;
  return h;
}
// waves of a grouped pass of k steps: the interior bands of every group and G seam bands; partial slots in this order
inline int grouped_waves(int rows, int groups, int band_rows, int n_strips, int k) {
  int bands = groups;
  for (int g = 0; g < groups; g++) {
    int lo, hi;
    group_rows(rows, groups, g, &lo, &hi);
    bands += ceil_div(hi - lo - 2 * k, band_rows);
  }
  return n_strips * bands;
}

// the rows of slab s of this process and its one-step launch geometry
struct SlabRows {
  int row_first = 0;  // global row of slab row 0
  int rows = 0;       // owned rows
  int accel_row = kNoRow;   // slab row (may be a halo row) holding global row ny-2
  int accel_row2 = kNoRow;  // its second periodic image among the halo rows (a ring of ONE slab with 3-step passes)
  int blocks_main = 0;      // interior rows (or all rows in HALO_SELF)
  int blocks_boundary = 0;  // rows 0 and rows-1 (halo modes)
};
inline SlabRows slab_rows(const PlanInput& in, bool vec4, int s) {
  SlabRows sl;
  const RowSpan mine = row_span(in.ny, in.world, in.rank);
  const RowSpan span = in.n_slabs > 1 ? row_span(mine.count, in.n_slabs, s) : RowSpan{0, mine.count};
  sl.row_first = mine.first + span.first;
  sl.rows = span.count;
  const int lid = in.ny - 2;  // SerialCode/d2q9-bgk.c:223
  // slab-local index of the lid row; with several slabs it may be one of MY halo rows (-kMaskHalo..-1 or
  // rows..rows+kMaskHalo-1), which a multi-step pass relaxes redundantly and must accelerate like its owner does
  for (int shift = -1; shift <= 1; shift++) {
    const int local = lid + shift * in.ny - sl.row_first;
    const bool owned = (local >= 0 && local < sl.rows);
    const bool in_halo = (in.halo != HALO_SELF) && ((local < 0 && local >= -kMaskHalo) || (local >= sl.rows && local < sl.rows + kMaskHalo));
    if (owned || in_halo) {
      if (sl.accel_row == kNoRow || owned) { if (sl.accel_row != kNoRow) sl.accel_row2 = sl.accel_row; sl.accel_row = local; }
      else sl.accel_row2 = local;
    }
  }
  const int edge_rows = (in.halo == HALO_SELF) ? 0 : 2;
  sl.blocks_main = blocks_for_rows(vec4, in.nx, sl.rows - edge_rows);
  sl.blocks_boundary = blocks_for_rows(vec4, in.nx, edge_rows);
  return sl;
}

// ---- stage one: the stream kernel ----------------------------------------------------------------------------------
// Which step kernel advances a decomposition of the grid into `parts` row slabs (in one process or over ranks), and how
// many timesteps it takes per pass -- from global numbers only, so every rank of a multi-process run decides alike.
struct StreamPlan { bool vec4; int fuse2, lane_cells, pass_steps; };
inline StreamPlan plan_stream(int nx, int ny, int parts, bool halo_on, const Knobs& env) {
  // 4 cells per lane need nx % 4 == 0; tiny single-slab grids are latency-bound and run faster with one
  // cell per lane (4x the waves, a quarter of the dependent arithmetic per lane: 128^2 3.2 vs 5.0 us per
  // step, 256^2 3.8 vs 5.2; from 512^2 on the 4-cell kernel wins).  Asking for the stream kernel,
  // which exists in the 4- and 2-cell forms only, implies vec4; so do halos.
  const bool vec4 = (nx % 4 == 0) && env.vec4.value(((long)nx * ny >= 128L * 1024 || env.fuse2.value(0) == 1 || halo_on) ? 1 : 0);
  const int min_rows = ny / (parts > 0 ? parts : 1);  // the thinnest slab of a balanced partition
  const long min_cells = (long)nx * min_rows;
  // Across slabs / ranks a pass costs one exchange and ~10 runtime calls per slab whatever it computes, so
  // several timesteps per pass always pay there (1024^2 over 2/4/8 slabs on one device: 45/74/97 us per step
  // vs 70/113/125 one-step; 2048^2 over 8: 96 vs 261).
  // (across slabs the stream kernel needs slabs of at least 4 rows)
  const int fuse2 = (vec4 && env.fuse2.value((min_cells >= 300L * 1024 || halo_on) ? 1 : 0) && !(halo_on && min_rows < 4)) ? 1 : 0;
  const int lane_cells = env.lane_cells.value(min_cells >= 7L * 512 * 1024 ? 4 : 2) == 2 ? 2 : 4;  // from 3.5 Mi cells
  // Timesteps per pass of the stream kernel.  The two-step kernel at 8192^2 is bound by DRAM traffic (round-2 PMC:
  // 5.4-5.8 TB/s at the memory controllers whatever the band height or the arithmetic), so the 4-cell form runs more
  // steps per pass: K = 3 (stepk_stream, 2 waves per SIMD, next row prefetched) 0.345 vs 0.47-0.49 ms per step, at
  // which point it is bound by VALU issue again (K = 4 with scalar arithmetic: 0.36); with the collision on PAIRS of
  // cells (stepk_pk: v_pk_* instructions, 108 instead of 155 lane-instructions per update) K = 4 pays: 0.275-0.285.
  // The packed kernel exists for the exact arithmetic only; the 2-cell form for K = 2 only.
  // The two-cell form (one pair per lane, twice the waves: mid-size grids) takes two halo lanes per side beyond two
  // steps and runs K = 3 as the packed kernel (124 VGPRs, 4 waves per SIMD): 1024^2 9.4 vs 10.7 us (K = 2), 1280^2
  // 12.4 vs 15.2 (four-cell K = 4), 1536^2 15.2 vs 20.9, 1792^2 20.2 vs 22.3; from 2048^2 the four-cell form wins
  // (24.9 vs 25.6-27.5).
  // FAST math (reciprocal + FMA, scalar) is the faster arithmetic only in the one-step and LDS-tile kernels.  The
  // multi-step stream kernels run the packed EXACT collision in both modes: it is faster than the scalar fast form
  // (8192^2: 0.27 vs 0.345 ms per step) and at K = 4 it already sits at the DRAM bound of its access pattern (5.8 GB per
  // launch at 5.4-5.8 TB/s), so a packed fast form could not be faster -- and exact results meet the fast mode's
  // tolerance trivially.  LBM_PACKED=0 selects the scalar kernels (fast math: K = 3 / 2).
  const bool exact_packed = env.packed.value(1) != 0;
  const int asked = env.pass_steps.value(lane_cells == 4 ? (exact_packed ? 4 : 3) : (exact_packed ? 3 : 2));
  // two steps where the request is out of range; the scalar two-cell kernel (step2_stream) is two-step; across slabs a
  // K-step pass needs slabs of at least 2K rows, a periodic slab at least K
  const bool two_steps = asked < 2 || asked > kHaloRows || (lane_cells != 4 && !exact_packed) ||
                         (halo_on && min_rows < 2 * asked) || min_rows < asked;
  return {vec4, fuse2, lane_cells, two_steps ? 2 : asked};
}

// ---- the band height of the stream kernels -------------------------------------------------------------------------
// Band height.  A wave sweeps band_rows + 2 rows.
//   4-cell form (256 CUs x 12 waves resident): short bands, by row width -- measured optimum 7 rows at 8192 cells
//   per row (8192^2: 0.477-0.480 ms vs 0.481-0.484 at 6, 0.495 at 4; same in the halo pipeline), 4-5 rows for
//   narrower and for wider rows (7168^2: 0.384 at 4 vs 0.411 at 7; 6144^2: 0.277 at 5 vs 0.303 at 7; 4096^2
//   0.131-0.132 at 4-7; 12288: 5; 16384^2: 2.01 at 4 vs 2.23 at 6).  Fitting whole rounds of resident waves
//   does NOT pay here (4096^2: 0.146 with the round model's 23-row bands vs 0.131; 8192x2048: 0.139 vs 0.126).
//   2-cell form (mid-size grids, 256 x 20 waves resident): a slab that fits in a few rounds is quantised by
//   them -- pick the height that fills k rounds exactly (1536^2: 4 rows = 0.98 rounds 24.0 us, 8 rows 25.3 us).
// `groups`: the band groups asked for (their interiors are in flight together); row_count: this process's rows.
inline int pick_band_rows(const PlanInput& in, int row_count, int lane_cells, int pass_steps, int n_strips, int groups, int band_max) {
  const bool halo_on = in.halo != HALO_SELF;
  const bool cut = in.n_slabs > 1 || in.world > 1;
  const int by_width = (in.nx <= 7168) ? 5 : (in.nx <= 8192 ? 7 : (in.nx <= 12288 ? 5 : 4));
  const long slab_rows = cut ? (row_count / in.n_slabs) - 4 : row_count;
  const long rows_eff = slab_rows > 1 ? slab_rows : 1;
  if (lane_cells == 4 && pass_steps >= 3) {
    // K >= 3 (2 waves per SIMD, bound by instruction issue): the waves run in rounds of 2048 and every wave of a round
    // takes band + 2(K-1) row iterations, so the cost of a band height is rounds x iterations (8192^2, K = 4: 46 rows
    // = 6086 waves = 2.97 rounds 0.274 ms per step; 55 rows = 2.47 rounds 0.288; 58 rows 0.300; 64 rows 0.309;
    // 24 / 32 rows 0.293 / 0.296; K = 3: 44 rows = 3.10 rounds 0.389, 46 rows 0.350).  Round 3: heights up to 160
    // rows -- ONE round of 2040 waves at 8192^2 (137 rows: 6 warm-up rows per 137 instead of per 46) 0.2691 vs
    // 0.2757 at 46, 0.2736 at 69 (two rounds), 0.284 at 92, 0.334 at 119, 0.321 at 180 (same box).
    // band groups: the interiors of the G groups are in flight together, and their waves fill the rounds together
    const long interior = (cut || halo_on) ? rows_eff + 4 - 2 * pass_steps
                                           : (groups > 1 ? rows_eff / groups - 2 * pass_steps : rows_eff);
    const long r_int = interior > 1 ? interior : 1;
    const int warm = 2 * (pass_steps - 1);
    if (groups * (long)n_strips * ceil_div(r_int, 24) >= 16L * 1024)
      return 32;  // many rounds (XCD-chunked order): flat in the height, 16384^2 24 / 32 / model (48) = 1.078 / 1.077 / 1.098
    // rounds of 2048 resident waves; a last round that fills at most half of the slots leaves one wave per SIMD,
    // which then runs at nearly twice the speed
    double best = -1.0;
    int pick = by_width;
    for (int b = 8; b <= band_max; b++) {
      const long waves = groups * (long)n_strips * ceil_div(r_int, b);
      const long full = waves / 2048, rest = waves % 2048;
      double rounds = (double)full + (rest == 0 ? 0.0 : (rest > 1024 ? 1.0 : 0.6));
      if (rounds < 1.0) rounds = 1.0;  // a lone wave on a SIMD hides no latency
      const double cost = rounds * (b + warm);
      if (best < 0.0 || cost < best) { best = cost; pick = b; }
    }
    return pick;
  }
  if (lane_cells == 2 && pass_steps >= 3) {
    // two-cell packed kernel: these sizes are bound by latency, and the best height is the one that spreads the
    // slab over one round of two waves per SIMD (2048 waves): 768^2 3, 1024^2 5, 1152^2 6, 1280^2 7-8, 1536^2 10,
    // 1792^2 14-16 rows (profiles/r02_tuning.md)
    const long interior = (cut || halo_on) ? rows_eff + 4 - 2 * pass_steps : rows_eff;
    const long b = ((interior > 1 ? interior : 1) * n_strips + 2047) / 2048;
    return (int)(b < 3 ? 3 : (b > 64 ? 64 : b));
  }
  const long resident = 256L * 4 * 5;  // 2-cell waves resident at once
  if (lane_cells == 2 && (long)n_strips * ceil_div(rows_eff, 8) < 5 * resident) {
    const long lo = 3;
    long best_cost = -1;
    int pick = by_width;
    for (int k = 1; k <= 4; k++) {
      long b = (rows_eff * n_strips + k * resident - 1) / (k * resident);
      if (b < lo) b = lo;
      if (b > 32) b = 32;
      const long rounds = ((long)n_strips * ceil_div(rows_eff, b) + resident - 1) / resident;
      const long cost = rounds * (b + 2);
      if (best_cost < 0 || cost < best_cost) { best_cost = cost; pick = (int)b; }
    }
    return pick;
  }
  return by_width;
}

// ---- the plan -----------------------------------------------------------------------------------------------------
// ---- which kernel, and its geometry (all measured on MI355X; profiles/r01_tuning.md) --------
//   single periodic slab below 300 Ki cells (round 2: the packed two-cell stream kernel wins from 576^2 on: 6.0 vs 7.2 us,
//                        640^2 7.2 vs 8.9, 704^2 7.2 vs 9.1; 512^2 5.8 vs 5.4): LDS tiles, 4 or 3 timesteps per launch (step_tile; set further
//                        down).  With halos: always several timesteps per pass (fewer exchanges).
//   (one timestep per pass, step_vec4 / step_scalar: the odd last step of a run, widths that are not a multiple
//                        of 4, LBM_FUSE2=0; it was the default up to 1.5 Mi cells until the two-step kernel stopped
//                        computing |u| on its warm-up rows: 768^2 9.8 vs 11.3 us, 1024^2 12.35 vs 13.23, 1152^2 15.3 vs 18.1)
//   0.3 .. 3.5 Mi cells : THREE timesteps per pass, 2 cells per lane (one pair, two halo lanes per side: 124 VGPRs,
//                        4 waves/SIMD, twice the waves of the 4-cell form; 1024^2 9.4 us vs 10.7 two-step)
//   >= 3.5 Mi cells    : FOUR timesteps per pass on pairs of cells, 4 cells per lane (16-byte accesses; us per step,
//                        this form | 2-cell two-step: 1024^2 15.1 | 10.7, 1280^2 15.2 | 17.2, 1536^2 20.9 | 22.1,
//                        1792^2 22.1 | 28.2; three-step scalar | two-step: 2048^2 31.8 | 35.4, 3072^2 59.0 | 76.0,
//                        4096^2 93 | 129, 8192^2 340 | 492; four-step packed: 2048^2 24.9, 4096^2 75.3, 8192^2 277-285)
// LBM_FUSE2, LBM_LANE_CELLS, LBM_BAND_ROWS override.  Ranks decide from global numbers only, so
// every rank of a multi-process run takes the same path.
inline KernelPlan plan_kernels(const PlanInput& in) {
  const Knobs env;
  const int nx = in.nx, ny = in.ny, n_slabs = in.n_slabs;
  const long cells = (long)nx * ny;
  const bool halo_on = (in.halo != HALO_SELF);
  const int row_count = row_span(ny, in.world, in.rank).count;  // rows of this process
  KernelPlan pl;

  const StreamPlan stream = plan_stream(nx, ny, in.world * n_slabs, halo_on, env);
  pl.vec4 = stream.vec4;
  pl.fuse2 = stream.fuse2;
  pl.lane_cells = stream.lane_cells;
  pl.pass_steps = stream.pass_steps;
  const int neigh = env.neigh.value(0);
  pl.neigh = (neigh < 0 || neigh > 2) ? 0 : neigh;
  // nontemporal stores pay once the two lattices no longer fit the 256 MiB Infinity Cache
  // (measured: +4 % at 4096^2 and above, -2..-20 % at 2048^2 and below; profiles/r01_tuning.md)
  const double lattice_pair_bytes = 2.0 * 36.0 * (double)nx * (double)ny;
  pl.nts = env.nts.value(lattice_pair_bytes > 512.0 * 1024 * 1024 ? 1 : 0) ? 1 : 0;
  pl.snake = env.snake.value(0) ? 1 : 0;

  // One issuing thread per slab when one process drives several slabs on DISTINCT devices (LBM_GPUS=n on a multi-GPU
  // node): a pass enqueues ~10 runtime calls per slab, 25-30 us on one thread -- more than an 8-GPU pass of 8192^2
  // takes on the devices.  With several slabs on ONE device it is slower (the runtime serialises calls to a device:
  // 65 vs 53 us per step for 2 slabs), so there it stays opt-in.  LBM_THREADS=0/1 overrides.
  pl.want_team = (n_slabs > 1 && env.threads.value(in.distinct_devices ? 1 : 0)) ? 1 : 0;
  // hipGraph replay pays where the loop is bound by the host's launch rate (~3.5 us per launch): measured
  // 128^2 3.11 vs 3.52 us per step, 128x256 3.22 vs 3.53; no difference from 256^2 on.
  // hipGraph replay of the halo pipeline (both streams of every slab, RCCL send/recv or device copies inside the
  // capture) exists (capture_chunk) but is OFF unless LBM_GRAPH=1: measured on MI355X / ROCm 7.2 it buys nothing
  // (host issue 11.1 vs 11.6 us per step for a rank with RCCL self-exchange at 256^2: the runtime still enqueues every
  // node) and hipGraphInstantiate overflows its stack on the larger pipelines (3+ slabs with device-copy halos, a
  // rank's 20-pass chunk at 8192x1024) -- profiles/r02_tuning.md.  The device-copy transport never uses it.
  // Nor does a context with a slab team.
  const bool graph_over_halos = env.graph.set && in.halo != HALO_HOST;
  pl.use_graph = (env.graph.value(cells < 64L * 1024 ? 1 : 0) && (!halo_on || graph_over_halos) && !pl.want_team) ? 1 : 0;

  pl.halo_lanes = ceil_div(pl.pass_steps, pl.lane_cells);
  pl.n_strips = ceil_div(nx / pl.lane_cells > 0 ? nx / pl.lane_cells : 1, 64 - 2 * pl.halo_lanes);
  // Packed arithmetic (exact mode, 4 cells per lane): on.  With K = 4 two of the three sliding windows live in LDS
  // (18 KB per wave), which leaves registers to prefetch the next row (216 VGPRs): us per step, this form | packed
  // without prefetch / LDS | scalar K = 3: 16384^2 1091 | 1097 | 1355, 12288^2 640 | 652 | 838, 6144^2 180 | 187 | 233,
  // 4096^2 75.3 | 78.1 | 94.7, 3072^2 45.6 | 45.3 | 59.0, 2048^2 24.9 | 26.3 | 31.9; a rank's share through the halo
  // pipeline 8192x1024 45.1 | 46.7 | 55.3, 8192x2048 77.5 | 81.4 | 98.9, 8192x4096 149 | 152 | 187.
  pl.packed = env.packed.value(1) ? 1 : 0;  // both math modes (see plan_stream)
  const int lds_windows = env.lds_windows.value((pl.packed && pl.pass_steps == 4) ? 2 : 0);
  pl.lds_windows = (lds_windows < 0 || lds_windows > 2 || !pl.packed) ? 0 : lds_windows;
  // scalar K = 4 with prefetch spills (245 + 36 VGPRs); the packed K = 4 needs its LDS windows for it
  pl.prefetch = env.prefetch.value((pl.lane_cells == 4 && (pl.pass_steps == 3 || (pl.pass_steps == 4 && pl.lds_windows == 2))) ? 1 : 0) ? 1 : 0;
  // strips per XCD chunk: a whole band of strips, for slabs of many rounds of waves only (16384^2, K = 4: 1.033 ms per
  // step with 67-strip chunks, 1.088 with 34, 1.107 without; K = 3: 12288^2 0.793 vs 0.832).  Elsewhere the band height
  // packs the waves tightly into rounds (below) and the few empty workgroups of the chunked order spill into an
  // extra round (4096^2: 0.135 vs 0.093; 8192^2: 0.298 vs 0.288).
  const bool many_rounds = (long)pl.n_strips * ceil_div(row_count / n_slabs, 24) >= 16L * 1024;
  const int xcd_chunk = env.xcd_chunk.value((pl.pass_steps >= 3 && many_rounds) ? pl.n_strips : 0);
  pl.xcd_chunk = (xcd_chunk < 0 || xcd_chunk > pl.n_strips) ? 0 : xcd_chunk;
  pl.use_stepk = env.stepk.value(0) ? 1 : 0;

  // Band groups (issue_grouped_pass): a single periodic slab issues its full-depth passes as G row groups on their own
  // streams, so that the next pass of one group fills the end of the current pass of the others.  Default: two groups
  // where four-step passes run on four-cell lanes (the launches there are one round of waves each, whose last waves
  // leave most of the chip idle); LBM_BAND_GROUPS overrides (1 = one launch per pass; at most kMaxBandGroups).
  const bool may_group = !halo_on && n_slabs == 1 && pl.fuse2 && !pl.use_graph;
  const int groups_asked = env.band_groups.value((pl.lane_cells == 4 && pl.pass_steps == 4) ? 2 : 1);
  const int groups_wanted = !may_group ? 1 : (groups_asked < 1 ? 1 : (groups_asked > kMaxBandGroups ? kMaxBandGroups : groups_asked));
  const int band_rows = env.band_rows.value(
      pick_band_rows(in, row_count, pl.lane_cells, pl.pass_steps, pl.n_strips, groups_wanted, env.band_max.value(160)));
  pl.band_rows = band_rows < 1 ? 1 : band_rows;
  // every group keeps an interior: by default a couple of bands, at least one row when asked for
  const int group_interior = row_count / groups_wanted - 2 * pl.pass_steps;
  const int groups_fit = (groups_wanted > 1 && group_interior < (env.band_groups.set ? 1 : 2 * pl.band_rows)) ? 1 : groups_wanted;

  // LDS-tile kernel (several timesteps per launch) for small single-slab grids: LBM_TILE_STEPS overrides
  // measured (us per step; one-step kernels | 16x8 tiles, 4 steps per launch | 32x16 tiles, 3 steps per launch):
  //   128^2 3.14 | 2.09 | -      256^2 3.84 | 2.82 | 3.54    384^2 5.65 | 4.19 | 5.43    448^2 6.14 | 5.44 | 5.26
  //   512^2 6.56 | 6.02 | 5.34   640^2 9.38 | 8.34 | 8.89    768^2 11.28 | 11.22 | 10.14  896^2 12.70 | 14.7 | 13.8
  //   1024^2 13.34 | 18.8 | 15.1 -- from there the redundant halo work costs more than the launches it saves
  // (asking for one of the other kernels by LBM_FUSE2 / LBM_VEC4 takes the tile kernel out of the default)
  if (!halo_on) {
    const bool other_kernel_requested = env.fuse2.set || env.vec4.set;
    const int dflt_shape = (cells <= 200L * 1024) ? 0 : 3;
    const int dflt_steps = (other_kernel_requested || cells >= 300L * 1024) ? 0 : kTileDims[dflt_shape].kmax;
    const int steps = env.tile_steps.value(dflt_steps);
    const int shape = env.tile_shape.value(env.tile_steps.set ? (steps > 4 ? 1 : 0) : dflt_shape);
    pl.tile_shape = (shape < 0 || shape >= kTileShapeCount) ? 0 : shape;
    const int kmax = kTileDims[pl.tile_shape].kmax;
    pl.tile_steps = (steps < 0 || steps > kmax) ? kmax : steps;
  }
  pl.band_groups = pl.tile_steps ? 1 : groups_fit;  // (the tile kernel runs every pass)

  // the most workgroups any launch of any slab has: every one of them writes a partial sum per step
  int max_blocks = 0;
  for (int s = 0; s < n_slabs; s++) {
    const SlabRows sl = slab_rows(in, pl.vec4, s);
    const int one_step = sl.blocks_main + sl.blocks_boundary;
    const int waves = pl.fuse2 ? pl.n_strips * (ceil_div(sl.rows, pl.band_rows) + 2) : 0;
    max_blocks = one_step > max_blocks ? one_step : max_blocks;
    max_blocks = waves > max_blocks ? waves : max_blocks;
  }
  const int grouped = groups_fit > 1 ? grouped_waves(row_count, groups_fit, pl.band_rows, pl.n_strips, pl.pass_steps) : 0;
  const int tiles = pl.tile_steps ? tile_count(nx, ny, pl.tile_shape) : 0;
  max_blocks = grouped > max_blocks ? grouped : max_blocks;
  max_blocks = tiles > max_blocks ? tiles : max_blocks;
  pl.part_stride = round_up(max_blocks, 64);

  // Resident kernel (lbm::resident_band): one launch advances up to kResidentChunk timesteps with the lattice in
  // registers, bands of 4 rows x the full width per workgroup, seam rows through L2 granules.  For single periodic
  // slabs whose bands are all co-resident (at most one workgroup per CU of the device) and whose rows are one lane
  // per cell wide: the reference's own data sets (128x128 ... 1024x1024).  Both math modes run it (its arithmetic is
  // the exact one, which meets the fast mode's tolerance and is the faster kernel at these sizes).  Asking for
  // another kernel by any of the selection knobs leaves it off unless LBM_RESIDENT=1 says otherwise.
  // This is the CANDIDATE: create_common confirms it with the device's occupancy query.
  if (!halo_on && n_slabs == 1) {
    const int cus = in.cus;
    // rows per band: 2 (one pair per lane) where every band still gets a CU of its own, else 4 (us per step, 4 | 2 rows:
    // 128^2 1.88 | 1.54, 128x256 1.93 | 1.59, 256^2 2.03 | 1.62, 512^2 2.73 | 2.17, 1024x512 4.35 | 3.43)
    const int rows_asked = env.resident_rows.value(0);
    const int rows = (rows_asked == 2 || rows_asked == 4) ? rows_asked : ((ny % 2 == 0 && ny / 2 <= cus && ny >= 4) ? 2 : 4);
    const bool shape_ok = nx % 64 == 0 && nx >= 64 && nx <= 1024 && ny % rows == 0 && ny >= 2 * rows;
    if (shape_ok && env.resident.value(env.selects_a_kernel() ? 0 : 1) && cus > 0 && ny / rows <= cus) {
      pl.resident = 1;
      pl.resident_rows = rows;
      pl.resident_bands = ny / rows;
      pl.resident_joint = (rows == 4 && nx <= 512 && env.resident_joint.value(nx <= 256 ? 1 : 0)) ? 1 : 0;
      // Grids of at most 128 waves (two-row bands): everything on ONE XCD, one wave per SIMD -- workgroups of four
      // waves (1, 2 or 4 bands side by side), at most one per CU of the XCD; 8 x the workgroups are launched and
      // those not dealt to the first XCD leave at once.  Then no seam crosses the fabric (hand-off 0.29 instead of
      // 0.63 us, tools/hop_flavours.hip): 128^2 1.10 vs 1.36 us per step, 64x128 1.06 vs 1.34, 128x64 1.05 vs 1.42
      // (two bands per workgroup alone: no change; one XCD with two workgroups per CU: none either).
      const int waves_per_band = nx / 64, cus_per_xcd = cus / 8;
      int fit_group = 0;  // the smallest power of two of bands per workgroup that puts the grid on one XCD
      if (rows == 2)
        for (int g = 1; g * waves_per_band <= 4 && !fit_group; g *= 2)
          if (pl.resident_bands % g == 0 && pl.resident_bands / g <= cus_per_xcd) fit_group = g;
      pl.resident_one_xcd = env.resident_one_xcd.value(fit_group ? 1 : 0) ? 1 : 0;
      const int group = env.resident_group.value((pl.resident_one_xcd && fit_group) ? fit_group : 1);
      pl.resident_group = (group < 1 || pl.resident_bands % group != 0 || nx * group > (nx > 512 ? 1024 : 512)) ? 1 : group;
      // a launch costs about 20 us before its first step (lattice into registers, back out, reduce, status copy);
      // measured wall time of one lbm_run(n) + sync, per-pass kernels | resident (tools/resident_crossover.py):
      // 128^2 n = 4 24.5 | 27.0, n = 8 32.9 | 32.4, n = 16 50.0 | 44.4; 256^2 n = 4 28.8 | 28.4, n = 8 41.0 | 35.4;
      // 1024^2 n = 4 59.8 | 50.4, n = 8 96.2 | 69.1
      const int min_steps = env.resident_min_steps.value(cells >= 48L * 1024 ? 4 : 8);
      pl.resident_min_steps = min_steps < 1 ? 1 : min_steps;
      pl.resident_timeout = (long long)env.resident_timeout_ms.value(2000) * 100000LL;  // wall_clock64(): 100 MHz
    }
  }
  return pl;
}

// ---- which stream kernel a pass launches ----------------------------------------------------------------------------
// The instantiation that advances k (2..4) timesteps in one pass under a plan: the kernel family and the template
// arguments that differ between its instantiations, with every request that has no kernel of its own already folded
// onto the one that runs instead.  lbm_hip.hip keeps the tables of function pointers and indexes them with this answer;
// tests/plan_dump.cpp prints it, so what a forced environment launches is known without a device.
//   step2_stream  <math, nts, lane_cells>             two steps, scalar arithmetic, four or two cells per lane
//   stepk_stream  <math, nts, 4, k, prefetch>         scalar arithmetic, four cells per lane
//   stepk_pk      <nts, k, prefetch, lds>             pairs of cells (exact arithmetic, both math modes), two pairs per lane
//   stepk_pk1     <nts, k, prefetch, lds, false, 1>   ... one pair per lane
enum StreamFamily { ROW_STEP2_STREAM = 0, ROW_STEPK_STREAM = 1, ROW_STEPK_PK = 2, ROW_STEPK_PK1 = 3 };
struct StreamRow {
  int family;      // StreamFamily
  int math;        // 0 exact, 1 fast (the packed kernels have the exact arithmetic only: 0)
  int nts;         // nontemporal stores
  int lane_cells;  // 4 or 2
  int k;           // timesteps of the pass
  int prefetch;    // the next row is requested before the current one is relaxed
  int lds;         // sliding windows kept in LDS (packed kernels)
};
inline StreamRow stream_row(const KernelPlan& pl, int k, bool exact) {
  const int math = exact ? 0 : 1, pf = pl.prefetch ? 1 : 0;
  if (pl.packed && pl.lane_cells == 2) {
    // one pair per lane: at most one window in LDS; K = 4 prefetches only with that window there (else it spills)
    const int lds = (pl.lds_windows < k ? pl.lds_windows : k - 1) ? 1 : 0;
    return {ROW_STEPK_PK1, 0, pl.nts, 2, k, (k == 4 && !lds) ? 0 : pf, lds};
  }
  if (pl.packed && pl.lane_cells == 4) {
    // a K-step pass has K - 1 sliding windows; K = 4 prefetches only with two of its three windows in LDS
    const int lds = pl.lds_windows < k ? pl.lds_windows : k - 1;
    return {ROW_STEPK_PK, 0, pl.nts, 4, k, (k == 4 && lds < 2) ? 0 : pf, lds};
  }
  // scalar arithmetic.  The two-cell form exists for two steps only (step2_stream); the four-cell form runs two steps
  // through stepk_stream where something only that kernel has is asked for.  K = 4 with the next row prefetched does not
  // fit the register file (112 bytes of scratch per lane), so that request runs the kernel without prefetch.
  if (pl.lane_cells == 4 && (k > 2 || pl.prefetch || pl.xcd_chunk || pl.use_stepk))
    return {ROW_STEPK_STREAM, math, pl.nts, 4, k, k == 4 ? 0 : pf, 0};
  return {ROW_STEP2_STREAM, math, pl.nts, pl.lane_cells == 2 ? 2 : 4, 2, 0, 0};
}

// ---- which shape of the resident kernel a plan launches -------------------------------------------------------------
// lbm::resident_band<MAXT, JOINT, ROWS, BATCH, REC> is compiled in five shapes for each (BATCH, REC); lbm_hip.hip keeps
// the instantiations (resident_form<BATCH, REC>) and indexes them with this answer; tests/plan_dump.cpp prints it
// ("resident_form"), so which of the 50 forms a forced environment launches is known without a device
// (tests/resident_forms.py).
//   0  <1024, false, 2>   two-row bands, nx > 512
//   1  <512, false, 2>    two-row bands, nx <= 512
//   2  <1024, false, 4>   four-row bands, nx > 512
//   3  <512, true, 4>     four-row bands, both pairs relaxed jointly (resident_joint)
//   4  <512, false, 4>    four-row bands, the interior pair ahead of the halo wait
inline int resident_form(int nx, int rows, int joint) {
  return (rows == 2) ? (nx > 512 ? 0 : 1) : (nx > 512 ? 2 : (joint ? 3 : 4));
}

}  // namespace lbm_plan
