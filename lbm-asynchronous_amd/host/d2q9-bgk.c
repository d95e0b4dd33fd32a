/*
 * d2q9-bgk.c -- the reference's command line on the MI355X engine (plain C99 host program).
 *
 *   ./d2q9-bgk <paramfile> <obstaclefile>
 *
 * Same arguments, same final_state.dat / av_vels.dat, same stdout block as
 * /root/reference/SerialCode/d2q9-bgk.c (main() :132-205).  The timestep loop (:166-170) is one
 * call into the C-ABI engine (include/lbm_hip.h); everything numerical happens on the GPU.
 *
 * Optional environment (the two-argument form stays valid), read by lbm_parse_options (lbm_options.c).  A malformed
 * value or a refused combination ends the program with a message before the parameter file is read and before any
 * device is touched.
 *   LBM_GPUS=<n>          row slabs / GPUs in this process (default 1)
 *   LBM_MATH=exact|fast   collision arithmetic (default exact: bit-identical to SerialCode)
 *   LBM_TILE=<tx>x<ty>    the obstacle file describes a tx x ty tile that is repeated over the
 *                         nx x ny grid of the parameter file (synthetic 8192^2 / 16384^2 grids)
 *   LBM_OUTPUT=text|none  write final_state.dat / av_vels.dat (default) or skip final_state.dat
 *   LBM_PRESSURE_BIN=<f>  additionally dump the fp32 pressure field (ny*nx floats) to <f>
 *   LBM_PRECISION=double  run the double-precision engine (lbm_double_*): the parameter file's density, accel and omega are
 *                         read as doubles, and final_state.dat / av_vels.dat hold the double results in the same formats
 *                         -- what the reference's golden files were computed in.  One GPU, plain runs only: with none of
 *                         the modes below, nor LBM_GPUS other than 1, LBM_MATH=fast, LBM_TILE or LBM_PRESSURE_BIN.
 *
 * Modes: at most one of LBM_STEADY, LBM_PROBES, LBM_ANIMATION, LBM_MEAN, LBM_STATES, LBM_FORCES and LBM_STATS; the numbers in their
 * values are plain decimal, digits only.  Every mode leaves final_state.dat unchanged.  All but LBM_STEADY leave
 * av_vels.dat unchanged where the run is resident (all four reference data sets); elsewhere it is that of the same run
 * issued as calls split at the sample steps.  LBM_PROBES, LBM_ANIMATION, LBM_STATES, LBM_FORCES and LBM_STATS record on the device
 * into a ring; the loop runs in segments that fill it (run_in_segments), each drained and written after it.
 *   LBM_STEADY=<tol>[:<check_every>[:<patience>]]
 *                         run to the steady state instead of for maxIters steps (lbm_run_until; check_every defaults to
 *                         1024, patience to 2): maxIters is the cap, av_vels.dat holds the steps that were run, and one
 *                         line "[Not steady|Steady] after N steps (rel. change X)" is printed before the ==done== block.
 *   LBM_PROBES=<x>,<y>[;<x>,<y>...][:<every>]
 *                         write probes.dat: one line "tt x y u_x u_y u pressure" per probed cell (at most 256) after every
 *                         timestep tt with tt % every == 0 (default 1); lbm_set_probes, a ring of 64 MiB.
 *   LBM_ANIMATION=<every> write animation_data/velocity_magnitude_%06d.dat, created if missing, after every timestep tt with
 *                         tt % every == 0 (the reference's commented-out write_animation_data hook, :171-173, :802-849);
 *                         unset or 0: off; lbm_set_frames, a ring of 1 GiB.
 *   LBM_MEAN=<every>[:<from>]
 *                         write mean_state.dat, final_state.dat's format with the time averages of u_x, u_y, u and pressure
 *                         (lbm_set_mean: float64 sums on the device, divided by the number of samples and rounded to
 *                         float): the loop runs <from> steps (default 0) unarmed, arms, and runs the rest, so the samples
 *                         are the steps tt >= from with tt % every == 0.  One line "Mean over N samples" is printed before
 *                         the ==done== block.
 *   LBM_MEAN_ORDER=1|2    with LBM_MEAN, and dies without: 2 also accumulates the second moments (lbm_set_mean_order) and
 *                         writes rms_state.dat, final_state.dat's format with the columns rms u_x, rms u_y, the Reynolds
 *                         shear stress <u'v'> and rms pressure over the same samples (var = max(<x x> - <x>^2, 0) in
 *                         double, rounded to float).
 *   LBM_STATES=<every>[:<x0>,<y0>,<nx>,<ny>]
 *                         write state_data/final_state_%06d.dat, created if missing: final_state.dat's format for the cells
 *                         of the window (default: the whole grid) after every timestep tt with tt % every == 0;
 *                         lbm_set_field_frames, a ring of 1 GiB.
 *   LBM_FORCES=<every>    write forces.dat: the force of the fluid on the obstacles (momentum exchange over the boundary
 *                         links, all blocked cells one body), one line "%d:\t%.12E\t%.12E" = tt, F_x, F_y after every step
 *                         tt with tt % every == 0, in av_vels.dat's style; lbm_set_forces, a ring of 4096 rows.
 *   LBM_STATS=<every>     write stats.dat: the statistics of the whole lattice (lbm_set_stats, a ring of 4096 rows), one line
 *                         "tt:\tmass\tmom_x\tmom_y\tsum_u_sq\tmax_u\tmax_x\tmax_y\tnonfinite" after every step tt with
 *                         tt % every == 0, the reals as %.12E.  If the last row counts cells that are not finite, one line on
 *                         stderr names the first sampled step that did.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/stat.h>
#include <sys/time.h>

#include "lbm_io.h"
#include "lbm_options.h"

static double wall_seconds(void)
{
  struct timeval t;
  gettimeofday(&t, NULL);
  return t.tv_sec + (t.tv_usec / 1000000.0);
}

static const char* environment(const char* name) { return getenv(name); }

/* an engine call that must not fail: dies with the engine's message */
static void must(int rc)
{
  if (rc != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
}

static void* must_alloc(size_t bytes, const char* message)
{
  void* p = malloc(bytes);
  if (p == NULL) lbm_die(message, __LINE__, __FILE__);
  return p;
}

static FILE* must_open(const char* path, const char* how)
{
  FILE* fp = fopen(path, how);
  if (fp == NULL) lbm_die("could not open file output file", __LINE__, __FILE__);
  return fp;
}

static void ensure_dir(const char* name)
{
  struct stat st;
  char message[64];
  snprintf(message, sizeof(message), "could not create %s", name);
  if (mkdir(name, 0777) != 0 && (stat(name, &st) != 0 || !S_ISDIR(st.st_mode))) lbm_die(message, __LINE__, __FILE__);
}

/* how many records the ring of a recording run holds: what fits the byte budget, no more than the run samples, at least 1 */
static int ring_capacity(size_t budget_bytes, size_t record_bytes, int max_iters, int every)
{
  long cap = (long)(budget_bytes / record_bytes);
  const long total = max_iters > 0 ? ((long)max_iters + every - 1) / every : 0;
  if (cap > total) cap = total;
  return cap < 1 ? 1 : (int)cap;
}

/* what a recording run keeps between its segments */
typedef struct {
  lbm_ctx* ctx;
  const lbm_params* params;
  const lbm_options* opt;    /* LBM_STATES: its window is set */
  const int* obstacles;
  void* records; int* steps; /* the host copy of the ring: cap records and their timesteps */
  FILE* fp;                  /* probes.dat, forces.dat, stats.dat */
  int bad_step;              /* LBM_STATS: the first sampled step with cells that are not finite (-1: none so far) ... */
  long long bad_last;        /* ... and how many the last row counted */
} recording;

/* the timestep loop of the recording modes: segments of cap samples, the ring drained after each */
static void run_in_segments(lbm_ctx* ctx, int max_iters, int every, int cap, void (*drain)(recording*, int), recording* state)
{
  const long seg = (long)cap * (long)every;
  for (long t = 0, n; t < max_iters; t += n) {
    n = (max_iters - t < seg) ? max_iters - t : seg;
    must(lbm_run(ctx, (int)n));
    drain(state, cap);
  }
}

static void drain_animation(recording* r, int cap)
{
  const size_t frame_cells = (size_t)r->params->nx * (size_t)r->params->ny;
  int n_read = 0;
  must(lbm_read_frames(r->ctx, cap, (float*)r->records, r->steps, &n_read));
  for (int i = 0; i < n_read; i++) {
    lbm_write_animation_frame("animation_data", r->params->nx, r->params->ny, r->steps[i], (const float*)r->records + (size_t)i * frame_cells);
    printf("Written animation data for timestep %d\n", r->steps[i]);
  }
}

static void drain_states(recording* r, int cap)
{
  const lbm_window* window = &r->opt->window;
  const size_t plane_cells = (size_t)window->nx * (size_t)window->ny;
  int n_read = 0;
  must(lbm_read_field_frames(r->ctx, cap, (float*)r->records, r->steps, &n_read));
  for (int i = 0; i < n_read; i++) {
    const float* f = (const float*)r->records + (size_t)i * 4 * plane_cells;
    lbm_write_state_frame("state_data", r->params, window, r->steps[i], f, f + plane_cells, f + 2 * plane_cells,
                          f + 3 * plane_cells, r->obstacles);
    printf("Written state data for timestep %d\n", r->steps[i]);
  }
}

static void drain_probes(recording* r, int cap)
{
  const int n_probes = r->opt->n_probes;
  const lbm_probe* cells = r->opt->probes;
  int n_read = 0;
  must(lbm_read_probes(r->ctx, cap, (lbm_probe_sample*)r->records, r->steps, &n_read));
  for (int i = 0; i < n_read; i++)
    for (int q = 0; q < n_probes; q++) {
      const lbm_probe_sample* v = (const lbm_probe_sample*)r->records + (size_t)i * (size_t)n_probes + q;
      fprintf(r->fp, "%d %d %d %.12E %.12E %.12E %.12E\n", r->steps[i], cells[q].x, cells[q].y, v->u_x, v->u_y, v->u_mag, v->pressure);
    }
}

static void drain_forces(recording* r, int cap)
{
  const double* rows = (const double*)r->records;
  int n_read = 0;
  must(lbm_read_forces(r->ctx, cap, (double*)r->records, r->steps, &n_read));
  for (int i = 0; i < n_read; i++) fprintf(r->fp, "%d:\t%.12E\t%.12E\n", r->steps[i], rows[2 * i], rows[2 * i + 1]);
}

static void drain_stats(recording* r, int cap)
{
  const lbm_stats_row* rows = (const lbm_stats_row*)r->records;
  int n_read = 0;
  must(lbm_read_stats(r->ctx, cap, (lbm_stats_row*)r->records, r->steps, &n_read));
  for (int i = 0; i < n_read; i++) {
    const lbm_stats_row* v = rows + i;
    fprintf(r->fp, "%d:\t%.12E\t%.12E\t%.12E\t%.12E\t%.12E\t%d\t%d\t%lld\n", r->steps[i], v->mass, v->mom_x, v->mom_y, v->sum_u_sq,
            (double)v->max_u, v->max_x, v->max_y, v->nonfinite);
    if (v->nonfinite > 0 && r->bad_step < 0) r->bad_step = r->steps[i];
    r->bad_last = v->nonfinite;
  }
}

/* the rest of a recording run once the device's ring is armed: allocate its host copy, open the file, run in segments */
static void record(recording* r, int cap, size_t record_bytes, const char* no_memory, const char* file, void (*drain)(recording*, int))
{
  r->records = must_alloc(record_bytes * (size_t)cap, no_memory);
  r->steps = (int*)must_alloc(sizeof(int) * (size_t)cap, no_memory);
  if (file) r->fp = must_open(file, "w");
  run_in_segments(r->ctx, r->params->max_iters, r->opt->every, cap, drain, r);
  if (file) fclose(r->fp);
  free(r->records);
  free(r->steps);
}

/* the recording modes: each case holds what differs -- record size, ring budget, arming call, output and drain function */
static void run_recording(lbm_ctx* ctx, const lbm_params* params, const lbm_options* opt, const int* obstacles)
{
  recording r = {ctx, params, opt, obstacles, NULL, NULL, NULL, -1, 0};
  const int every = opt->every, max_iters = params->max_iters;
  size_t record_bytes;
  int cap;
  switch (opt->mode) {
    case LBM_MODE_ANIMATION:
      record_bytes = (size_t)params->nx * (size_t)params->ny * sizeof(float);
      cap = ring_capacity(1UL << 30, record_bytes, max_iters, every);
      ensure_dir("animation_data");
      must(lbm_set_frames(ctx, every, cap));
      record(&r, cap, record_bytes, "cannot allocate memory for animation frames", NULL, drain_animation);
      break;
    case LBM_MODE_STATES:
      record_bytes = 4 * (size_t)opt->window.nx * (size_t)opt->window.ny * sizeof(float);
      cap = ring_capacity(1UL << 30, record_bytes, max_iters, every);
      must(lbm_set_field_frames(ctx, every, cap, LBM_FIELD_ALL, &opt->window));
      ensure_dir("state_data");
      record(&r, cap, record_bytes, "cannot allocate memory for field frames", NULL, drain_states);
      break;
    case LBM_MODE_PROBES:
      record_bytes = (size_t)opt->n_probes * sizeof(lbm_probe_sample);
      cap = ring_capacity(64UL << 20, record_bytes, max_iters, every);
      must(lbm_set_probes(ctx, opt->n_probes, opt->probes, every, cap));
      record(&r, cap, record_bytes, "cannot allocate memory for probe samples", LBM_PROBESFILE, drain_probes);
      break;
    case LBM_MODE_STATS: /* a ring of 4096 rows */
      record_bytes = sizeof(lbm_stats_row);
      cap = ring_capacity(4096 * record_bytes, record_bytes, max_iters, every);
      must(lbm_set_stats(ctx, every, cap));
      record(&r, cap, record_bytes, "cannot allocate memory for statistics rows", LBM_STATSFILE, drain_stats);
      if (r.bad_last > 0)
        fprintf(stderr, "%lld cells of the lattice are not finite; the first sampled step with such cells was %d\n", r.bad_last, r.bad_step);
      break;
    default: /* LBM_MODE_FORCES: a ring of 4096 rows */
      record_bytes = 2 * sizeof(double);
      cap = ring_capacity(4096 * record_bytes, record_bytes, max_iters, every);
      must(lbm_set_forces(ctx, 1, NULL, every, cap));
      record(&r, cap, record_bytes, "cannot allocate memory for force rows", LBM_FORCESFILE, drain_forces);
  }
}

/* the reference's report (:195-200) */
static void report(double reynolds, double tot_tic, double init_toc, double comp_toc, double col_toc)
{
  printf("==done==\n");
  printf("Reynolds number:\t\t%.12E\n", reynolds);
  printf("Elapsed Init time:\t\t\t%.6lf (s)\n", init_toc - tot_tic);
  printf("Elapsed Compute time:\t\t\t%.6lf (s)\n", comp_toc - init_toc);
  printf("Elapsed Collate time:\t\t\t%.6lf (s)\n", col_toc - comp_toc);
  printf("Elapsed Total time:\t\t\t%.6lf (s)\n", col_toc - tot_tic);
}

/* a file in final_state.dat's format from four planes [ny][nx]: of floats with params, of doubles with params_double */
static void write_state_file(const char* path, const lbm_params* params, const lbm_params_double* params_double, const void* fields,
                             const int* obstacles)
{
  static char iobuf[1 << 22];
  const int ny = params ? params->ny : params_double->ny;
  const size_t n = (size_t)(params ? params->nx : params_double->nx) * (size_t)ny;
  const float* f = (const float*)fields;
  const double* d = (const double*)fields;
  FILE* fp = must_open(path, "w");
  setvbuf(fp, iobuf, _IOFBF, sizeof(iobuf));
  if (params) lbm_write_final_state_rows(fp, params, 0, ny, f, f + n, f + 2 * n, f + 3 * n, obstacles);
  else lbm_write_final_state_rows_double(fp, params_double, 0, ny, d, d + n, d + 2 * n, d + 3 * n, obstacles);
  fclose(fp);
}

/* LBM_MEAN's files from the device's sums (4 planes, with order 2 another 4); lbm.fluctuations_of is the twin of the second */
static void write_mean_files(const lbm_params* params, const double* mean_sums, int order, long long mean_samples, const int* obstacles)
{
  const size_t n_cells = (size_t)params->nx * (size_t)params->ny;
  /* the sums divided by the number of samples, rounded to float, in final_state.dat's format */
  float* mean = (float*)must_alloc(sizeof(float) * 4 * n_cells, "cannot allocate memory for the mean fields");
  for (size_t i = 0; i < 4 * n_cells; i++) mean[i] = (float)(mean_sums[i] / (double)mean_samples);
  write_state_file(LBM_MEANSTATEFILE, params, NULL, mean, obstacles);
  if (order == 2) {
    /* m = S1 / n, q = S2 / n in double: rms = sqrt(max(q - m m, 0)), <u'v'> = q_xy - m_x m_y; rounded to float */
    const double n = (double)mean_samples;
    const double *s1x = mean_sums, *s1y = mean_sums + n_cells, *s1p = mean_sums + 3 * n_cells;
    const double *sxx = mean_sums + 4 * n_cells, *syy = sxx + n_cells, *sxy = syy + n_cells, *spp = sxy + n_cells;
    for (size_t i = 0; i < n_cells; i++) {
      const double mx = s1x[i] / n, my = s1y[i] / n, mp = s1p[i] / n;
      const double vx = sxx[i] / n - mx * mx, vy = syy[i] / n - my * my, vp = spp[i] / n - mp * mp;
      mean[i] = (float)sqrt(vx > 0.0 ? vx : 0.0);
      mean[n_cells + i] = (float)sqrt(vy > 0.0 ? vy : 0.0);
      mean[2 * n_cells + i] = (float)(sxy[i] / n - mx * my);
      mean[3 * n_cells + i] = (float)sqrt(vp > 0.0 ? vp : 0.0);
    }
    write_state_file(LBM_RMSSTATEFILE, params, NULL, mean, obstacles);
  }
  free(mean);
}

/* LBM_PRECISION=double: the same program on the double engine (main() :132-205 with every float read as double) */
static int main_double(const char* paramfile, const char* obstaclefile, const lbm_options* opt)
{
  const double tot_tic = wall_seconds();
  lbm_params_double params;
  lbm_read_params_double(paramfile, &params);
  const lbm_params shape = {params.nx, params.ny, params.max_iters, params.reynolds_dim, 0.f, 0.f, 0.f};
  int* obstacles = lbm_read_obstacles(obstaclefile, &shape);
  lbm_double_ctx* ctx = lbm_double_create(&params, obstacles, NULL);
  lbm_double_sync(ctx);
  const double init_toc = wall_seconds();

  lbm_double_run(ctx, params.max_iters);
  lbm_double_sync(ctx);
  const double comp_toc = wall_seconds();

  const size_t n_cells = (size_t)params.nx * (size_t)params.ny;
  double* av_vels = (double*)must_alloc(sizeof(double) * (size_t)(params.max_iters > 0 ? params.max_iters : 1), "cannot allocate memory for av_vels");
  lbm_double_read_av_vels(ctx, av_vels, params.max_iters);
  double reynolds = 0.0;
  lbm_double_calc_reynolds(ctx, &reynolds);
  double* fields = NULL;
  if (opt->write_text) {
    fields = (double*)must_alloc(sizeof(double) * 4 * n_cells, "cannot allocate memory for cells");
    lbm_double_read_final_state(ctx, fields, fields + n_cells, fields + 2 * n_cells, fields + 3 * n_cells);
  }
  const double col_toc = wall_seconds();

  report(reynolds, tot_tic, init_toc, comp_toc, col_toc);
  if (opt->write_text) write_state_file(LBM_FINALSTATEFILE, NULL, &params, fields, obstacles);
  lbm_write_av_vels_double(LBM_AVVELSFILE, av_vels, params.max_iters);

  lbm_double_destroy(ctx);
  free(fields);
  free(av_vels);
  free(obstacles);
  return EXIT_SUCCESS;
}

int main(int argc, char* argv[])
{
  if (argc != 3) lbm_usage(argv[0]);
  const char* paramfile = argv[1];
  const char* obstaclefile = argv[2];
  static lbm_options opt;
  lbm_parse_options(environment, &opt);
  if (opt.is_double) return main_double(paramfile, obstaclefile, &opt);

  /* Total/init time starts here (SerialCode/d2q9-bgk.c:156-159) */
  const double tot_tic = wall_seconds();
  lbm_params params;
  lbm_read_params(paramfile, &params);
  const lbm_window whole_grid = {0, 0, params.nx, params.ny};
  if (opt.mode == LBM_MODE_STATES && opt.window.nx == 0) opt.window = whole_grid;

  /* uniform equilibrium start is generated on the device (cells_aos == NULL); with LBM_TILE the mask is
   * expanded on the device from the tile, and the global map is only built if a file is written that shows it
   * (its last column is the obstacle flag, SerialCode/d2q9-bgk.c:722) */
  int* obstacles = NULL;
  lbm_ctx* ctx;
  if (opt.tiled) {
    const lbm_params tile_params = {opt.tile_nx, opt.tile_ny, 0, 0, 0.f, 0.f, 0.f};
    int* tile = lbm_read_obstacles(obstaclefile, &tile_params);
    ctx = lbm_create_tiled(&params, tile, opt.tile_nx, opt.tile_ny, NULL, opt.n_gpus, opt.math_mode);
    if (opt.write_text || opt.mode == LBM_MODE_MEAN || opt.mode == LBM_MODE_STATES)
      obstacles = lbm_tile_obstacles(tile, opt.tile_nx, opt.tile_ny, params.nx, params.ny);
    free(tile);
  } else {
    obstacles = lbm_read_obstacles(obstaclefile, &params);
    ctx = lbm_create(&params, obstacles, NULL, opt.n_gpus, opt.math_mode);
  }
  if (opt.n_gpus > 1) {
    /* the MPI programs announce their ranks ("Process %d of %d started.", MPI/d2q9-bgk.c:151): here, what the halo
       transport is -- which RCCL, and how many ranks its communicators count */
    lbm_rccl_status st;
    lbm_info info;
    if (lbm_rccl_info(ctx, &st) == LBM_SUCCESS && lbm_get_info(ctx, &info) == LBM_SUCCESS) {
      const int n_devices = lbm_device_count() < opt.n_gpus ? lbm_device_count() : opt.n_gpus;
      if (st.n_comms > 0)
        fprintf(stderr, "%d row slabs on %d device(s): RCCL %d.%d.%d (%s), %d communicators of %d ranks\n", info.n_slabs, n_devices,
                st.version / 10000, st.version / 100 % 100, st.version % 100, st.library, st.n_comms, st.nranks);
      else
        fprintf(stderr, "%d row slabs on %d device(s): halo rows by device copies\n", info.n_slabs, n_devices);
    }
  }
  lbm_sync(ctx);
  const double init_toc = wall_seconds();

  /* Compute time: the whole timestep loop (:166-170), run by mode */
  int steps_run = params.max_iters;
  lbm_steady_result steady = {0};
  if (opt.mode == LBM_MODE_STEADY) {
    /* maxIters is the cap: the loop ends when the average velocity has stopped changing */
    must(lbm_run_until(ctx, params.max_iters, opt.every, opt.steady_tol, opt.steady_patience, &steady));
    steps_run = steady.steps_run;
  } else if (opt.mode == LBM_MODE_MEAN) {
    /* <from> steps unarmed, then the rest armed */
    const int from = opt.mean_from < params.max_iters ? opt.mean_from : params.max_iters;
    must(lbm_run(ctx, from));
    must(lbm_set_mean_order(ctx, opt.every, opt.mean_order));
    must(lbm_run(ctx, params.max_iters - from));
  } else if (opt.mode != LBM_MODE_PLAIN) {
    run_recording(ctx, &params, &opt, obstacles);
  } else {
    lbm_run(ctx, params.max_iters);
  }
  lbm_sync(ctx);
  const double comp_toc = wall_seconds();

  /* Collate: bring the results back to the host */
  const size_t n_cells = (size_t)params.nx * (size_t)params.ny;
  float* av_vels = (float*)must_alloc(sizeof(float) * (size_t)(params.max_iters > 0 ? params.max_iters : 1), "cannot allocate memory for av_vels");
  lbm_read_av_vels(ctx, av_vels, steps_run);
  float reynolds = 0.f;
  lbm_calc_reynolds(ctx, &reynolds);
  float* fields = NULL;
  if (opt.write_text || opt.pressure_bin) {
    fields = (float*)must_alloc(sizeof(float) * 4 * n_cells, "cannot allocate memory for cells");
    lbm_read_final_state(ctx, fields, fields + n_cells, fields + 2 * n_cells, fields + 3 * n_cells);
  }
  double* mean_sums = NULL;
  long long mean_samples = 0;
  if (opt.mode == LBM_MODE_MEAN) {
    mean_sums = (double*)must_alloc(sizeof(double) * 4 * (size_t)opt.mean_order * n_cells, "cannot allocate memory for the mean fields");
    must(lbm_read_mean(ctx, mean_sums, mean_sums + n_cells, mean_sums + 2 * n_cells, mean_sums + 3 * n_cells, &mean_samples));
    if (opt.mean_order == 2)
      must(lbm_read_mean2(ctx, mean_sums + 4 * n_cells, mean_sums + 5 * n_cells, mean_sums + 6 * n_cells, mean_sums + 7 * n_cells, NULL));
  }
  const double col_toc = wall_seconds();

  if (opt.mode == LBM_MODE_STEADY)
    printf("%s after %d steps (rel. change %.6E)\n", steady.steady ? "Steady" : "Not steady", steady.steps_run, steady.last_rel);
  if (opt.mode == LBM_MODE_MEAN) printf("Mean over %lld samples\n", mean_samples);
  report(reynolds, tot_tic, init_toc, comp_toc, col_toc);

  if (opt.write_text) write_state_file(LBM_FINALSTATEFILE, &params, NULL, fields, obstacles);
  lbm_write_av_vels(LBM_AVVELSFILE, av_vels, steps_run);
  if (opt.mode == LBM_MODE_MEAN && mean_samples > 0) write_mean_files(&params, mean_sums, opt.mean_order, mean_samples, obstacles);
  if (opt.pressure_bin) {
    FILE* fp = must_open(opt.pressure_bin, "wb");
    fwrite(fields + 3 * n_cells, sizeof(float), n_cells, fp);
    fclose(fp);
  }

  lbm_destroy(ctx);
  free(fields);
  free(mean_sums);
  free(av_vels);
  free(obstacles);
  return EXIT_SUCCESS;
}
