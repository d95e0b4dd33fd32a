/*
 * d2q9-bgk.c -- the reference's command line on the MI355X engine (plain C99 host program).
 *
 *   ./d2q9-bgk <paramfile> <obstaclefile>
 *
 * Same arguments, same final_state.dat / av_vels.dat, same stdout block as
 * /root/reference/SerialCode/d2q9-bgk.c (main() :132-205).  The timestep loop (:166-170) is one
 * call into the C-ABI engine (include/lbm_hip.h); everything numerical happens on the GPU.
 *
 * Optional environment (the two-argument form stays valid):
 *   LBM_GPUS=<n>          row slabs / GPUs in this process (default 1)
 *   LBM_MATH=exact|fast   collision arithmetic (default exact: bit-identical to SerialCode)
 *   LBM_TILE=<tx>x<ty>    the obstacle file describes a tx x ty tile that is repeated over the
 *                         nx x ny grid of the parameter file (synthetic 8192^2 / 16384^2 grids)
 *   LBM_OUTPUT=text|none  write final_state.dat / av_vels.dat (default) or skip final_state.dat
 *   LBM_PRESSURE_BIN=<f>  additionally dump the fp32 pressure field (ny*nx floats) to <f>
 *   LBM_ANIMATION=<every> write animation_data/velocity_magnitude_%06d.dat after every timestep tt with
 *                         tt % every == 0 (the reference's commented-out write_animation_data hook, :171-173,
 *                         :802-849), created if missing; unset or 0: off.  The frames are recorded on the device
 *                         (lbm_set_frames); the loop runs in segments whose frames fit 1 GiB and is drained after each.
 *                         final_state.dat and av_vels.dat are unchanged.
 *   LBM_STEADY=<tol>[:<check_every>[:<patience>]]
 *                         run to the steady state instead of for maxIters steps (lbm_run_until; check_every defaults to
 *                         1024, patience to 2): maxIters is the cap, av_vels.dat holds the steps that were run, and one
 *                         line "Steady after N steps (rel. change X)" / "Not steady after N steps (rel. change X)" is
 *                         printed before the ==done== block.  Not together with LBM_ANIMATION.
 *   LBM_MEAN=<every>[:<from>]
 *                         additionally write mean_state.dat, final_state.dat's format with the time averages of u_x, u_y,
 *                         u and pressure (lbm_set_mean: float64 sums on the device, divided by the number of samples and
 *                         rounded to float): the loop runs <from> steps (default 0) unarmed, arms, and runs the rest, so
 *                         the samples are the steps tt >= from with tt % every == 0.  One line "Mean over N samples" is
 *                         printed before the ==done== block.  final_state.dat is unchanged; av_vels.dat is unchanged where
 *                         the run is resident (all four reference data sets), elsewhere it is that of the same run issued
 *                         as calls split at <from> and at the sample steps.  Not together with LBM_ANIMATION, LBM_PROBES
 *                         or LBM_STEADY.
 *   LBM_MEAN_ORDER=1|2    with LBM_MEAN: 2 also accumulates the second moments (lbm_set_mean_order) and additionally writes
 *                         rms_state.dat, final_state.dat's format with the columns rms u_x, rms u_y, the Reynolds shear
 *                         stress <u'v'> and rms pressure over the same samples (var = max(<x x> - <x>^2, 0) in double,
 *                         rounded to float).  The other files are unchanged.  Dies when set without LBM_MEAN.
 *   LBM_PRECISION=double  run the double-precision engine (lbm_double_*): the parameter file's density, accel and omega are
 *                         read as doubles, and final_state.dat / av_vels.dat hold the double results in the same formats
 *                         -- what the reference's golden files were computed in.  One GPU, plain runs only: dies together
 *                         with LBM_GPUS > 1, LBM_MATH=fast, LBM_TILE, LBM_ANIMATION, LBM_STEADY, LBM_PROBES, LBM_MEAN or
 *                         LBM_PRESSURE_BIN.  Unset or "single": everything above, unchanged.
 *   LBM_FORCES=<every>    additionally write forces.dat: the force of the fluid on the obstacles (lbm_set_forces: momentum
 *                         exchange over the boundary links, all blocked cells one body), one line "%d:\t%.12E\t%.12E" =
 *                         tt, F_x, F_y after every step tt with tt % every == 0, in av_vels.dat's style.  final_state.dat
 *                         is unchanged; av_vels.dat is that of the same run issued as calls split at the sample steps.  Not
 *                         together with LBM_ANIMATION, LBM_STATES, LBM_PROBES, LBM_MEAN, LBM_STEADY or LBM_PRECISION=double.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/time.h>

#include "lbm_io.h"

static double wall_seconds(void)
{
  struct timeval t;
  gettimeofday(&t, NULL);
  return t.tv_sec + (t.tv_usec / 1000000.0);
}

/* LBM_STEADY=<tol>[:<check_every>[:<patience>]]; dies on anything else, as lbm_read_params does on a bad file */
static void parse_steady(const char* text, double* tol, int* check_every, int* patience)
{
  char* end = NULL;
  *tol = strtod(text, &end);
  int ok = (end != text) && *tol >= 0.0;
  long v[2] = {1024, 2};
  for (int i = 0; ok && i < 2 && *end == ':'; i++) {
    const char* from = end + 1;
    v[i] = strtol(from, &end, 10);
    ok = (end != from) && v[i] >= 1 && v[i] <= 2147483647L;
  }
  if (!ok || *end != '\0')
    lbm_die("could not read LBM_STEADY: expected <tol>[:<check_every>[:<patience>]] with tol >= 0, check_every >= 1, patience >= 1",
            __LINE__, __FILE__);
  *check_every = (int)v[0];
  *patience = (int)v[1];
}

/* LBM_PROBES=x,y[;x,y...][:every] (every defaults to 1); plain decimal numbers only; dies on anything else */
static int parse_probes(const char* text, lbm_probe* cells, int* every)
{
  const char* s = text;
  int n = 0, ok = 1;
  *every = 1;
  for (;;) {
    long v[2];
    for (int i = 0; ok && i < 2; i++) {
      char* end = NULL;
      ok = (*s >= '0' && *s <= '9');
      if (!ok) break;
      v[i] = strtol(s, &end, 10);
      ok = v[i] <= 2147483647L && (i == 1 || *end == ',');
      s = (i == 0 && ok) ? end + 1 : end;
    }
    if (!ok || n == LBM_MAX_PROBES) { ok = 0; break; }
    cells[n].x = (int)v[0];
    cells[n].y = (int)v[1];
    n++;
    if (*s != ';') break;
    s++;
  }
  if (ok && *s == ':') {
    char* end = NULL;
    s++;
    ok = (*s >= '0' && *s <= '9');
    const long e = ok ? strtol(s, &end, 10) : 0;
    ok = ok && e >= 1 && e <= 2147483647L;
    *every = (int)e;
    if (ok) s = end;
  }
  if (!ok || *s != '\0')
    lbm_die("could not read LBM_PROBES: expected <x>,<y>[;<x>,<y>...][:<every>] with at most 256 cells and every >= 1", __LINE__, __FILE__);
  return n;
}

/* LBM_MEAN=<every>[:<from>] (from defaults to 0); plain decimal numbers only; dies on anything else */
static void parse_mean(const char* text, int* every, int* from)
{
  const char* s = text;
  long v[2] = {0, 0};
  int ok = 1;
  for (int i = 0; ok && i < 2; i++) {
    char* end = NULL;
    ok = (*s >= '0' && *s <= '9');
    if (!ok) break;
    v[i] = strtol(s, &end, 10);
    ok = v[i] <= 2147483647L;
    s = end;
    if (i == 0 && *s != ':') break;
    if (i == 0) s++;
  }
  if (!ok || *s != '\0' || v[0] < 1)
    lbm_die("could not read LBM_MEAN: expected <every>[:<from>] with every >= 1 and from >= 0", __LINE__, __FILE__);
  *every = (int)v[0];
  *from = (int)v[1];
}

/* LBM_STATES=<every>[:<x0>,<y0>,<nx>,<ny>] (the window defaults to the whole grid: nx = 0 here); plain decimal numbers
   only; dies on anything else */
static void parse_states(const char* text, int* every, lbm_window* window)
{
  const char* s = text;
  long v[5] = {0, 0, 0, 0, 0};
  int ok = 1, n = 0;
  for (; ok && n < 5; n++) {
    char* end = NULL;
    ok = (*s >= '0' && *s <= '9');
    if (!ok) break;
    v[n] = strtol(s, &end, 10);
    ok = v[n] <= 2147483647L;
    s = end;
    if (*s != (n == 0 ? ':' : ',') || n == 4) { n++; break; }
    s++;
  }
  if (!ok || *s != '\0' || (n != 1 && n != 5) || v[0] < 1 || (n == 5 && (v[3] < 1 || v[4] < 1)))
    lbm_die("could not read LBM_STATES: expected <every>[:<x0>,<y0>,<nx>,<ny>] with every >= 1, nx >= 1 and ny >= 1", __LINE__, __FILE__);
  *every = (int)v[0];
  window->x0 = (int)v[1];
  window->y0 = (int)v[2];
  window->nx = (int)v[3];
  window->ny = (int)v[4];
}

/* LBM_FORCES=<every>: a plain decimal number >= 1, nothing else */
static int parse_forces(const char* text)
{
  char* end = NULL;
  const long v = strtol(text, &end, 10);
  if (end == text || *end != '\0' || text[0] < '0' || text[0] > '9' || v < 1 || v > 2147483647L)
    lbm_die("could not read LBM_FORCES: expected <every> with every >= 1", __LINE__, __FILE__);
  return (int)v;
}

/* LBM_PRECISION=double: the same program on the double engine (main() :132-205 with every float read as double) */
static int main_double(const char* paramfile, const char* obstaclefile)
{
  static const char* const not_offered[] = {"LBM_TILE", "LBM_ANIMATION", "LBM_STEADY", "LBM_PROBES", "LBM_MEAN",
                                            "LBM_MEAN_ORDER", "LBM_PRESSURE_BIN"};
  const char* env;
  char message[256];
  for (size_t i = 0; i < sizeof(not_offered) / sizeof(not_offered[0]); i++)
    if ((env = getenv(not_offered[i])) && *env) {
      snprintf(message, sizeof(message), "%s is not offered with LBM_PRECISION=double", not_offered[i]);
      lbm_die(message, __LINE__, __FILE__);
    }
  if ((env = getenv("LBM_GPUS")) && *env && atoi(env) != 1) lbm_die("LBM_GPUS is not offered with LBM_PRECISION=double", __LINE__, __FILE__);
  if ((env = getenv("LBM_MATH")) && !strcmp(env, "fast")) lbm_die("LBM_MATH=fast is not offered with LBM_PRECISION=double", __LINE__, __FILE__);
  int write_text = 1;
  if ((env = getenv("LBM_OUTPUT")) && !strcmp(env, "none")) write_text = 0;

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
  double* av_vels = (double*)malloc(sizeof(double) * (size_t)(params.max_iters > 0 ? params.max_iters : 1));
  if (av_vels == NULL) lbm_die("cannot allocate memory for av_vels", __LINE__, __FILE__);
  lbm_double_read_av_vels(ctx, av_vels, params.max_iters);
  double reynolds = 0.0;
  lbm_double_calc_reynolds(ctx, &reynolds);
  double* fields = NULL;
  if (write_text) {
    fields = (double*)malloc(sizeof(double) * 4 * n_cells);
    if (fields == NULL) lbm_die("cannot allocate memory for cells", __LINE__, __FILE__);
    lbm_double_read_final_state(ctx, fields, fields + n_cells, fields + 2 * n_cells, fields + 3 * n_cells);
  }
  const double col_toc = wall_seconds();

  printf("==done==\n");
  printf("Reynolds number:\t\t%.12E\n", reynolds);
  printf("Elapsed Init time:\t\t\t%.6lf (s)\n", init_toc - tot_tic);
  printf("Elapsed Compute time:\t\t\t%.6lf (s)\n", comp_toc - init_toc);
  printf("Elapsed Collate time:\t\t\t%.6lf (s)\n", col_toc - comp_toc);
  printf("Elapsed Total time:\t\t\t%.6lf (s)\n", col_toc - tot_tic);

  if (write_text) {
    FILE* fp = fopen(LBM_FINALSTATEFILE, "w");
    if (fp == NULL) lbm_die("could not open file output file", __LINE__, __FILE__);
    lbm_write_final_state_rows_double(fp, &params, 0, params.ny, fields, fields + n_cells, fields + 2 * n_cells,
                                      fields + 3 * n_cells, obstacles);
    fclose(fp);
  }
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

  const char* env;
  const char* states_env = getenv("LBM_STATES");
  int states_every = 0;
  lbm_window states_window = {0, 0, 0, 0};
  if (states_env && *states_env) parse_states(states_env, &states_every, &states_window);
  if (states_every > 0 && (env = getenv("LBM_PRECISION")) && !strcmp(env, "double"))
    lbm_die("LBM_PRECISION=double and LBM_STATES cannot be combined", __LINE__, __FILE__);
  const char* forces_env = getenv("LBM_FORCES");
  const int forces_every = (forces_env && *forces_env) ? parse_forces(forces_env) : 0;
  if (forces_every > 0 && (env = getenv("LBM_PRECISION")) && !strcmp(env, "double"))
    lbm_die("LBM_PRECISION=double and LBM_FORCES cannot be combined", __LINE__, __FILE__);
  if ((env = getenv("LBM_PRECISION")) && *env) {
    if (!strcmp(env, "double")) return main_double(paramfile, obstaclefile);
    if (strcmp(env, "single")) lbm_die("could not read LBM_PRECISION: expected single or double", __LINE__, __FILE__);
  }
  int n_gpus = 1;
  if ((env = getenv("LBM_GPUS")) && *env) n_gpus = atoi(env);
  int math_mode = LBM_MATH_EXACT;
  if ((env = getenv("LBM_MATH")) && !strcmp(env, "fast")) math_mode = LBM_MATH_FAST;
  int write_text = 1;
  if ((env = getenv("LBM_OUTPUT")) && !strcmp(env, "none")) write_text = 0;

  const char* steady_env = getenv("LBM_STEADY");
  const int until = steady_env && *steady_env;
  double steady_tol = 0.0;
  int steady_every = 0, steady_patience = 0;
  if (until) parse_steady(steady_env, &steady_tol, &steady_every, &steady_patience);

  const char* probes_env = getenv("LBM_PROBES");
  static lbm_probe probe_cells[LBM_MAX_PROBES];
  int probe_every = 0;
  const int n_probes = (probes_env && *probes_env) ? parse_probes(probes_env, probe_cells, &probe_every) : 0;
  if (n_probes > 0 && until) lbm_die("LBM_STEADY and LBM_PROBES cannot be combined", __LINE__, __FILE__);

  const char* mean_env = getenv("LBM_MEAN");
  int mean_every = 0, mean_from = 0;
  if (mean_env && *mean_env) parse_mean(mean_env, &mean_every, &mean_from);
  const char* order_env = getenv("LBM_MEAN_ORDER");
  int mean_order = 1;
  if (order_env && *order_env) {
    /* plain decimal 1 or 2, nothing else */
    if ((order_env[0] != '1' && order_env[0] != '2') || order_env[1] != '\0')
      lbm_die("could not read LBM_MEAN_ORDER: expected 1 or 2", __LINE__, __FILE__);
    if (mean_every == 0) lbm_die("LBM_MEAN_ORDER needs LBM_MEAN", __LINE__, __FILE__);
    mean_order = order_env[0] - '0';
  }
  if (mean_every > 0 && until) lbm_die("LBM_STEADY and LBM_MEAN cannot be combined", __LINE__, __FILE__);
  if (mean_every > 0 && n_probes > 0) lbm_die("LBM_PROBES and LBM_MEAN cannot be combined", __LINE__, __FILE__);
  if (mean_every > 0 && (env = getenv("LBM_ANIMATION")) && *env && atoi(env) > 0)
    lbm_die("LBM_ANIMATION and LBM_MEAN cannot be combined", __LINE__, __FILE__);
  if (states_every > 0 && until) lbm_die("LBM_STEADY and LBM_STATES cannot be combined", __LINE__, __FILE__);
  if (states_every > 0 && n_probes > 0) lbm_die("LBM_PROBES and LBM_STATES cannot be combined", __LINE__, __FILE__);
  if (states_every > 0 && mean_every > 0) lbm_die("LBM_MEAN and LBM_STATES cannot be combined", __LINE__, __FILE__);
  if (states_every > 0 && (env = getenv("LBM_ANIMATION")) && *env && atoi(env) > 0)
    lbm_die("LBM_ANIMATION and LBM_STATES cannot be combined", __LINE__, __FILE__);
  if (forces_every > 0 && until) lbm_die("LBM_STEADY and LBM_FORCES cannot be combined", __LINE__, __FILE__);
  if (forces_every > 0 && n_probes > 0) lbm_die("LBM_PROBES and LBM_FORCES cannot be combined", __LINE__, __FILE__);
  if (forces_every > 0 && mean_every > 0) lbm_die("LBM_MEAN and LBM_FORCES cannot be combined", __LINE__, __FILE__);
  if (forces_every > 0 && states_every > 0) lbm_die("LBM_STATES and LBM_FORCES cannot be combined", __LINE__, __FILE__);
  if (forces_every > 0 && (env = getenv("LBM_ANIMATION")) && *env && atoi(env) > 0)
    lbm_die("LBM_ANIMATION and LBM_FORCES cannot be combined", __LINE__, __FILE__);

  /* Total/init time starts here (SerialCode/d2q9-bgk.c:156-159) */
  const double tot_tic = wall_seconds();
  lbm_params params;
  lbm_read_params(paramfile, &params);

  /* uniform equilibrium start is generated on the device (cells_aos == NULL); with LBM_TILE the mask is
   * expanded on the device from the tile, and the global map is only built if final_state.dat is written
   * (its last column is the obstacle flag, SerialCode/d2q9-bgk.c:722) */
  int* obstacles = NULL;
  int tile_nx = 0, tile_ny = 0;
  lbm_ctx* ctx;
  if ((env = getenv("LBM_TILE")) && sscanf(env, "%dx%d", &tile_nx, &tile_ny) == 2) {
    lbm_params tile_params = params;
    tile_params.nx = tile_nx;
    tile_params.ny = tile_ny;
    int* tile = lbm_read_obstacles(obstaclefile, &tile_params);
    ctx = lbm_create_tiled(&params, tile, tile_nx, tile_ny, NULL, n_gpus, math_mode);
    if (write_text || mean_every > 0 || states_every > 0) obstacles = lbm_tile_obstacles(tile, tile_nx, tile_ny, params.nx, params.ny);
    free(tile);
  } else {
    obstacles = lbm_read_obstacles(obstaclefile, &params);
    ctx = lbm_create(&params, obstacles, NULL, n_gpus, math_mode);
  }
  if (n_gpus > 1) {
    /* the MPI programs announce their ranks ("Process %d of %d started.", MPI/d2q9-bgk.c:151): here, what the halo
       transport is -- which RCCL, and how many ranks its communicators count */
    lbm_rccl_status st;
    lbm_info info;
    if (lbm_rccl_info(ctx, &st) == LBM_SUCCESS && lbm_get_info(ctx, &info) == LBM_SUCCESS) {
      if (st.n_comms > 0)
        fprintf(stderr, "%d row slabs on %d device(s): RCCL %d.%d.%d (%s), %d communicators of %d ranks\n", info.n_slabs,
                lbm_device_count() < n_gpus ? lbm_device_count() : n_gpus, st.version / 10000, st.version / 100 % 100,
                st.version % 100, st.library, st.n_comms, st.nranks);
      else
        fprintf(stderr, "%d row slabs on %d device(s): halo rows by device copies\n", info.n_slabs,
                lbm_device_count() < n_gpus ? lbm_device_count() : n_gpus);
    }
  }
  lbm_sync(ctx);
  const double init_toc = wall_seconds();

  int anim_every = 0;
  if ((env = getenv("LBM_ANIMATION")) && *env) anim_every = atoi(env);

  if (until && anim_every > 0) lbm_die("LBM_STEADY and LBM_ANIMATION cannot be combined", __LINE__, __FILE__);
  if (n_probes > 0 && anim_every > 0) lbm_die("LBM_PROBES and LBM_ANIMATION cannot be combined", __LINE__, __FILE__);
  int steps_run = params.max_iters;
  lbm_steady_result steady;
  memset(&steady, 0, sizeof(steady));

  /* Compute time: the whole timestep loop (:166-170) */
  if (until) {
    /* maxIters is the cap: the loop ends when the average velocity has stopped changing */
    if (lbm_run_until(ctx, params.max_iters, steady_every, steady_tol, steady_patience, &steady) != LBM_SUCCESS)
      lbm_die(lbm_last_error(), __LINE__, __FILE__);
    steps_run = steady.steps_run;
  } else if (anim_every > 0) {
    /* with frames: segments whose frames fit 1 GiB of device memory, each drained and written after it */
    const size_t frame_cells = (size_t)params.nx * (size_t)params.ny;
    long cap = (long)((1UL << 30) / (frame_cells * sizeof(float)));
    const long total_frames = params.max_iters > 0 ? (params.max_iters + anim_every - 1) / anim_every : 0;
    if (cap > total_frames) cap = total_frames;
    if (cap < 1) cap = 1;
    if (mkdir("animation_data", 0777) != 0) {
      struct stat st;
      if (stat("animation_data", &st) != 0 || !S_ISDIR(st.st_mode)) lbm_die("could not create animation_data", __LINE__, __FILE__);
    }
    if (lbm_set_frames(ctx, anim_every, (int)cap) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
    float* frames = (float*)malloc(frame_cells * sizeof(float) * (size_t)cap);
    int* steps = (int*)malloc(sizeof(int) * (size_t)cap);
    if (frames == NULL || steps == NULL) lbm_die("cannot allocate memory for animation frames", __LINE__, __FILE__);
    const long seg = cap * (long)anim_every;
    for (long t = 0; t < params.max_iters;) {
      const int n = (int)((params.max_iters - t < seg) ? params.max_iters - t : seg);
      if (lbm_run(ctx, n) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
      int n_read = 0;
      if (lbm_read_frames(ctx, (int)cap, frames, steps, &n_read) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
      for (int i = 0; i < n_read; i++) {
        lbm_write_animation_frame("animation_data", params.nx, params.ny, steps[i], frames + (size_t)i * frame_cells);
        printf("Written animation data for timestep %d\n", steps[i]);
      }
      t += n;
    }
    free(frames);
    free(steps);
  } else if (states_every > 0) {
    /* with field frames: segments whose frames fit 1 GiB of device memory, each drained and written after it */
    if (states_window.nx == 0) {
      states_window.nx = params.nx;
      states_window.ny = params.ny;
    }
    const size_t plane_cells = (size_t)states_window.nx * (size_t)states_window.ny, frame_cells = 4 * plane_cells;
    long cap = (long)((1UL << 30) / (frame_cells * sizeof(float)));
    const long total_frames = params.max_iters > 0 ? (params.max_iters + states_every - 1) / states_every : 0;
    if (cap > total_frames) cap = total_frames;
    if (cap < 1) cap = 1;
    if (lbm_set_field_frames(ctx, states_every, (int)cap, LBM_FIELD_ALL, &states_window) != LBM_SUCCESS)
      lbm_die(lbm_last_error(), __LINE__, __FILE__);
    if (mkdir("state_data", 0777) != 0) {
      struct stat st;
      if (stat("state_data", &st) != 0 || !S_ISDIR(st.st_mode)) lbm_die("could not create state_data", __LINE__, __FILE__);
    }
    float* frames = (float*)malloc(frame_cells * sizeof(float) * (size_t)cap);
    int* steps = (int*)malloc(sizeof(int) * (size_t)cap);
    if (frames == NULL || steps == NULL) lbm_die("cannot allocate memory for field frames", __LINE__, __FILE__);
    const long seg = cap * (long)states_every;
    for (long t = 0; t < params.max_iters;) {
      const int n = (int)((params.max_iters - t < seg) ? params.max_iters - t : seg);
      if (lbm_run(ctx, n) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
      int n_read = 0;
      if (lbm_read_field_frames(ctx, (int)cap, frames, steps, &n_read) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
      for (int i = 0; i < n_read; i++) {
        const float* f = frames + (size_t)i * frame_cells;
        lbm_write_state_frame("state_data", &params, &states_window, steps[i], f, f + plane_cells, f + 2 * plane_cells,
                              f + 3 * plane_cells, obstacles);
        printf("Written state data for timestep %d\n", steps[i]);
      }
      t += n;
    }
    free(frames);
    free(steps);
  } else if (n_probes > 0) {
    /* with probes: segments whose sample rows fit a ring of 64 MiB, each drained and written after it */
    const size_t row_bytes = (size_t)n_probes * sizeof(lbm_probe_sample);
    long cap = (long)((64UL << 20) / row_bytes);
    const long total_rows = params.max_iters > 0 ? (params.max_iters + probe_every - 1) / probe_every : 0;
    if (cap > total_rows) cap = total_rows;
    if (cap < 1) cap = 1;
    if (lbm_set_probes(ctx, n_probes, probe_cells, probe_every, (int)cap) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
    lbm_probe_sample* samples = (lbm_probe_sample*)malloc(row_bytes * (size_t)cap);
    int* steps = (int*)malloc(sizeof(int) * (size_t)cap);
    FILE* fp = fopen(LBM_PROBESFILE, "w");
    if (samples == NULL || steps == NULL) lbm_die("cannot allocate memory for probe samples", __LINE__, __FILE__);
    if (fp == NULL) lbm_die("could not open file output file", __LINE__, __FILE__);
    const long seg = cap * (long)probe_every;
    for (long t = 0; t < params.max_iters;) {
      const int n = (int)((params.max_iters - t < seg) ? params.max_iters - t : seg);
      if (lbm_run(ctx, n) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
      int n_read = 0;
      if (lbm_read_probes(ctx, (int)cap, samples, steps, &n_read) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
      for (int i = 0; i < n_read; i++)
        for (int q = 0; q < n_probes; q++) {
          const lbm_probe_sample* v = samples + (size_t)i * (size_t)n_probes + q;
          fprintf(fp, "%d %d %d %.12E %.12E %.12E %.12E\n", steps[i], probe_cells[q].x, probe_cells[q].y, v->u_x, v->u_y, v->u_mag,
                  v->pressure);
        }
      t += n;
    }
    fclose(fp);
    free(samples);
    free(steps);
  } else if (forces_every > 0) {
    /* with the forces: segments whose rows fit a ring of 4096, each drained and written after it */
    const long total_rows = params.max_iters > 0 ? (params.max_iters + forces_every - 1) / forces_every : 0;
    long cap = 4096;
    if (cap > total_rows) cap = total_rows;
    if (cap < 1) cap = 1;
    if (lbm_set_forces(ctx, 1, NULL, forces_every, (int)cap) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
    double* rows = (double*)malloc(2 * sizeof(double) * (size_t)cap);
    int* steps = (int*)malloc(sizeof(int) * (size_t)cap);
    FILE* fp = fopen(LBM_FORCESFILE, "w");
    if (rows == NULL || steps == NULL) lbm_die("cannot allocate memory for force rows", __LINE__, __FILE__);
    if (fp == NULL) lbm_die("could not open file output file", __LINE__, __FILE__);
    const long seg = cap * (long)forces_every;
    for (long t = 0; t < params.max_iters;) {
      const int n = (int)((params.max_iters - t < seg) ? params.max_iters - t : seg);
      if (lbm_run(ctx, n) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
      int n_read = 0;
      if (lbm_read_forces(ctx, (int)cap, rows, steps, &n_read) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
      for (int i = 0; i < n_read; i++) fprintf(fp, "%d:\t%.12E\t%.12E\n", steps[i], rows[2 * i], rows[2 * i + 1]);
      t += n;
    }
    fclose(fp);
    free(rows);
    free(steps);
  } else if (mean_every > 0) {
    /* with the mean fields: <from> steps unarmed, then the rest armed */
    const int from = mean_from < params.max_iters ? mean_from : params.max_iters;
    if (lbm_run(ctx, from) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
    if (lbm_set_mean_order(ctx, mean_every, mean_order) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
    if (lbm_run(ctx, params.max_iters - from) != LBM_SUCCESS) lbm_die(lbm_last_error(), __LINE__, __FILE__);
  } else {
    lbm_run(ctx, params.max_iters);
  }
  lbm_sync(ctx);
  const double comp_toc = wall_seconds();

  /* Collate: bring the results back to the host */
  const size_t n_cells = (size_t)params.nx * (size_t)params.ny;
  float* av_vels = (float*)malloc(sizeof(float) * (size_t)(params.max_iters > 0 ? params.max_iters : 1));
  if (av_vels == NULL) lbm_die("cannot allocate memory for av_vels", __LINE__, __FILE__);
  lbm_read_av_vels(ctx, av_vels, steps_run);
  float reynolds = 0.f;
  lbm_calc_reynolds(ctx, &reynolds);
  float* fields = NULL;
  const int want_fields = write_text || getenv("LBM_PRESSURE_BIN");
  if (want_fields) {
    fields = (float*)malloc(sizeof(float) * 4 * n_cells);
    if (fields == NULL) lbm_die("cannot allocate memory for cells", __LINE__, __FILE__);
    lbm_read_final_state(ctx, fields, fields + n_cells, fields + 2 * n_cells, fields + 3 * n_cells);
  }
  double* mean_sums = NULL;
  long long mean_samples = 0;
  if (mean_every > 0) {
    mean_sums = (double*)malloc(sizeof(double) * 4 * (size_t)mean_order * n_cells);
    if (mean_sums == NULL) lbm_die("cannot allocate memory for the mean fields", __LINE__, __FILE__);
    if (lbm_read_mean(ctx, mean_sums, mean_sums + n_cells, mean_sums + 2 * n_cells, mean_sums + 3 * n_cells, &mean_samples) != LBM_SUCCESS)
      lbm_die(lbm_last_error(), __LINE__, __FILE__);
    if (mean_order == 2 &&
        lbm_read_mean2(ctx, mean_sums + 4 * n_cells, mean_sums + 5 * n_cells, mean_sums + 6 * n_cells, mean_sums + 7 * n_cells, NULL) != LBM_SUCCESS)
      lbm_die(lbm_last_error(), __LINE__, __FILE__);
  }
  const double col_toc = wall_seconds();

  if (until)
    printf("%s after %d steps (rel. change %.6E)\n", steady.steady ? "Steady" : "Not steady", steady.steps_run, steady.last_rel);
  if (mean_every > 0) printf("Mean over %lld samples\n", mean_samples);
  /* the reference's report (:195-200) */
  printf("==done==\n");
  printf("Reynolds number:\t\t%.12E\n", reynolds);
  printf("Elapsed Init time:\t\t\t%.6lf (s)\n", init_toc - tot_tic);
  printf("Elapsed Compute time:\t\t\t%.6lf (s)\n", comp_toc - init_toc);
  printf("Elapsed Collate time:\t\t\t%.6lf (s)\n", col_toc - comp_toc);
  printf("Elapsed Total time:\t\t\t%.6lf (s)\n", col_toc - tot_tic);

  if (write_text) {
    FILE* fp = fopen(LBM_FINALSTATEFILE, "w");
    if (fp == NULL) lbm_die("could not open file output file", __LINE__, __FILE__);
    static char iobuf[1 << 22];
    setvbuf(fp, iobuf, _IOFBF, sizeof(iobuf));
    lbm_write_final_state_rows(fp, &params, 0, params.ny, fields, fields + n_cells, fields + 2 * n_cells,
                               fields + 3 * n_cells, obstacles);
    fclose(fp);
  }
  lbm_write_av_vels(LBM_AVVELSFILE, av_vels, steps_run);
  if (mean_every > 0 && mean_samples > 0) {
    /* the sums divided by the number of samples, rounded to float, in final_state.dat's format */
    float* mean = (float*)malloc(sizeof(float) * 4 * n_cells);
    if (mean == NULL) lbm_die("cannot allocate memory for the mean fields", __LINE__, __FILE__);
    for (size_t i = 0; i < 4 * n_cells; i++) mean[i] = (float)(mean_sums[i] / (double)mean_samples);
    FILE* fp = fopen(LBM_MEANSTATEFILE, "w");
    if (fp == NULL) lbm_die("could not open file output file", __LINE__, __FILE__);
    lbm_write_final_state_rows(fp, &params, 0, params.ny, mean, mean + n_cells, mean + 2 * n_cells, mean + 3 * n_cells, obstacles);
    fclose(fp);
    if (mean_order == 2) {
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
      fp = fopen(LBM_RMSSTATEFILE, "w");
      if (fp == NULL) lbm_die("could not open file output file", __LINE__, __FILE__);
      lbm_write_final_state_rows(fp, &params, 0, params.ny, mean, mean + n_cells, mean + 2 * n_cells, mean + 3 * n_cells, obstacles);
      fclose(fp);
    }
    free(mean);
  }
  if ((env = getenv("LBM_PRESSURE_BIN")) && *env) {
    FILE* fp = fopen(env, "wb");
    if (fp == NULL) lbm_die("could not open file output file", __LINE__, __FILE__);
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
