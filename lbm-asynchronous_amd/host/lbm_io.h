/*
 * lbm_io.h -- host-side file formats of the d2q9-bgk command line (plain C99).
 *
 * Reads the 7-value parameter file and the "x y 1" obstacle file, and writes
 * final_state.dat / av_vels.dat, in the formats and with the error messages of the reference
 * program (/root/reference/SerialCode/d2q9-bgk.c: initialise() :460-613, write_values()
 * :662-743, die() :745-751, usage() :753-757).  No lattice arithmetic happens here: the
 * per-cell output quantities arrive already computed (on the device, lbm_read_final_state()).
 */
#ifndef LBM_IO_H
#define LBM_IO_H

#include <stdio.h>

#include "../../include/lbm_hip.h"

#define LBM_FINALSTATEFILE "final_state.dat" /* SerialCode/d2q9-bgk.c:62 */
#define LBM_AVVELSFILE     "av_vels.dat"     /* :63 */
#define LBM_PROBESFILE     "probes.dat"      /* LBM_PROBES: the time series at the probed cells (no counterpart) */
#define LBM_MEANSTATEFILE  "mean_state.dat"  /* LBM_MEAN: final_state.dat's format with the time-averaged fields (no counterpart) */
#define LBM_FORCESFILE     "forces.dat"      /* LBM_FORCES: the force on the obstacles at the sample steps (no counterpart) */
#define LBM_STATSFILE      "stats.dat"       /* LBM_STATS: the lattice statistics at the sample steps (no counterpart) */
#define LBM_RMSSTATEFILE   "rms_state.dat"   /* LBM_MEAN_ORDER=2: the same format with rms u_x, rms u_y, <u'v'>, rms pressure */

/* message to stderr + exit(EXIT_FAILURE), the reference's die() (:745-751) */
void lbm_die(const char* message, const int line, const char* file);
/* "Usage: %s <paramfile> <obstaclefile>" + exit(EXIT_FAILURE) (:753-757) */
void lbm_usage(const char* exe);

/* the seven fscanf reads of initialise() (:471-509); dies with the reference's messages */
void lbm_read_params(const char* paramfile, lbm_params* params);

/* the same file for the double engine: density, accel and omega scanned as doubles ("%lf") */
void lbm_read_params_double(const char* paramfile, lbm_params_double* params);

/* malloc + zero an int[ny*nx] map and fill it from the obstacle file (:541-604);
 * dies with the reference's messages on malformed or out-of-range lines */
int* lbm_read_obstacles(const char* obstaclefile, const lbm_params* params);

/* synthetic large grids: tile a small obstacle map periodically,
 * cell (x,y) of the big map is blocked iff (x % tile_nx, y % tile_ny) is blocked in the tile */
int* lbm_tile_obstacles(const int* tile, int tile_nx, int tile_ny, int nx, int ny);

/* final_state.dat: "%d %d %.12E %.12E %.12E %.12E %d\n" = ii jj u_x u_y u pressure obstacle,
 * jj outer / ii inner (:679-723).  Rows [row_first, row_first+row_count) are appended to fp. */
void lbm_write_final_state_rows(FILE* fp, const lbm_params* params, int row_first, int row_count,
                                const float* u_x, const float* u_y, const float* u_mag,
                                const float* pressure, const int* obstacles);

/* <dir>/final_state_%06d.dat (LBM_STATES, no counterpart): final_state.dat's line format for the cells of `window`
 * (global ii jj, jj outer / ii inner) from the four planes [window->ny][window->nx] of one field frame; `obstacles` is
 * the whole grid's map */
void lbm_write_state_frame(const char* dir, const lbm_params* params, const lbm_window* window, int timestep,
                           const float* u_x, const float* u_y, const float* u_mag, const float* pressure,
                           const int* obstacles);

/* animation_data/velocity_magnitude_%06d.dat of write_animation_data() (:802-849): "# nx=%d ny=%d timestep=%d",
 * then one "%.6E" line per cell of u_mag[ny*nx] (0 for blocked cells), jj outer / ii inner */
void lbm_write_animation_frame(const char* dir, int nx, int ny, int timestep, const float* u_mag);
/* av_vels.dat: "%d:\t%.12E\n" (:735-738) */
void lbm_write_av_vels(const char* path, const float* av_vels, int n);

/* the two writers for the double engine's results: the same formats ("%.12E"), which show a double's first 13 digits */
void lbm_write_final_state_rows_double(FILE* fp, const lbm_params_double* params, int row_first, int row_count,
                                       const double* u_x, const double* u_y, const double* u_mag,
                                       const double* pressure, const int* obstacles);
void lbm_write_av_vels_double(const char* path, const double* av_vels, int n);

#endif /* LBM_IO_H */
