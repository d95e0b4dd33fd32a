/*
 * lbm_io.c -- parameter / obstacle readers and result writers of the d2q9-bgk command line.
 * Formats and messages follow /root/reference/SerialCode/d2q9-bgk.c (lines cited in lbm_io.h).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "lbm_io.h"

void lbm_die(const char* message, const int line, const char* file)
{
  fprintf(stderr, "Error at line %d of file %s:\n", line, file);
  fprintf(stderr, "%s\n", message);
  fflush(stderr);
  exit(EXIT_FAILURE);
}

void lbm_usage(const char* exe)
{
  fprintf(stderr, "Usage: %s <paramfile> <obstaclefile>\n", exe);
  exit(EXIT_FAILURE);
}

/* seven values, one per line, in this order (SerialCode/d2q9-bgk.c:480-506); the last three scanned with real_fmt */
static void read_params(const char* paramfile, int* nx, int* ny, int* max_iters, int* reynolds_dim, const char* real_fmt,
                        void* density, void* accel, void* omega)
{
  char message[1024];
  FILE* fp = fopen(paramfile, "r");
  if (fp == NULL) {
    snprintf(message, sizeof(message), "could not open input parameter file: %s", paramfile);
    lbm_die(message, __LINE__, __FILE__);
  }
  struct { const char* fmt; void* dst; const char* what; } field[7] = {
    { "%d\n",    nx,           "could not read param file: nx" },
    { "%d\n",    ny,           "could not read param file: ny" },
    { "%d\n",    max_iters,    "could not read param file: maxIters" },
    { "%d\n",    reynolds_dim, "could not read param file: reynolds_dim" },
    { real_fmt,  density,      "could not read param file: density" },
    { real_fmt,  accel,        "could not read param file: accel" },
    { real_fmt,  omega,        "could not read param file: omega" },
  };
  for (int i = 0; i < 7; i++)
    if (fscanf(fp, field[i].fmt, field[i].dst) != 1) lbm_die(field[i].what, __LINE__, __FILE__);
  fclose(fp);
}

void lbm_read_params(const char* paramfile, lbm_params* p)
{
  read_params(paramfile, &p->nx, &p->ny, &p->max_iters, &p->reynolds_dim, "%f\n", &p->density, &p->accel, &p->omega);
}

/* scanned as doubles, so 1.85 is the double 1.85, not (double)1.85f */
void lbm_read_params_double(const char* paramfile, lbm_params_double* p)
{
  read_params(paramfile, &p->nx, &p->ny, &p->max_iters, &p->reynolds_dim, "%lf\n", &p->density, &p->accel, &p->omega);
}

int* lbm_read_obstacles(const char* obstaclefile, const lbm_params* params)
{
  char message[1024];
  const size_t n = (size_t)params->nx * (size_t)params->ny;
  int* map = (int*)calloc(n, sizeof(int));
  if (map == NULL) lbm_die("cannot allocate column memory for obstacles", __LINE__, __FILE__);

  FILE* fp = fopen(obstaclefile, "r");
  if (fp == NULL) {
    snprintf(message, sizeof(message), "could not open input obstacles file: %s", obstaclefile);
    lbm_die(message, __LINE__, __FILE__);
  }

  int xx, yy, blocked, got;
  while ((got = fscanf(fp, "%d %d %d\n", &xx, &yy, &blocked)) != EOF) {
    /* the reference's checks and messages, SerialCode/d2q9-bgk.c:591-597 */
    if (got != 3) lbm_die("expected 3 values per line in obstacle file", __LINE__, __FILE__);
    if (xx < 0 || xx > params->nx - 1) lbm_die("obstacle x-coord out of range", __LINE__, __FILE__);
    if (yy < 0 || yy > params->ny - 1) lbm_die("obstacle y-coord out of range", __LINE__, __FILE__);
    if (blocked != 1) lbm_die("obstacle blocked value should be 1", __LINE__, __FILE__);
    map[(size_t)xx + (size_t)yy * params->nx] = blocked;
  }
  fclose(fp);
  return map;
}

int* lbm_tile_obstacles(const int* tile, int tile_nx, int tile_ny, int nx, int ny)
{
  int* map = (int*)malloc((size_t)nx * (size_t)ny * sizeof(int));
  if (map == NULL) lbm_die("cannot allocate column memory for obstacles", __LINE__, __FILE__);
  for (int y = 0; y < ny; y++) {
    const int* trow = tile + (size_t)(y % tile_ny) * tile_nx;
    int* row = map + (size_t)y * nx;
    for (int x = 0; x < nx; x++) row[x] = trow[x % tile_nx];
  }
  return map;
}

/* one line per cell is ~85 bytes of printf work; 8192^2 is 5.7 GB of text.  Rows are formatted by
 * all cores into per-thread buffers (snprintf, so the bytes are exactly what the reference's
 * fprintf produces) and written out in order. */
#define LBM_LINE_MAX 128 /* "%d %d" + 4 x "%.12E" (<= 20 chars each) + " %d\n" */

/* element c of a field of floats or of doubles, as printf receives it (a float argument is promoted to double) */
static inline double field_at(const void* field, int is_double, size_t c)
{
  return is_double ? ((const double*)field)[c] : (double)((const float*)field)[c];
}

static void write_final_state_rows(FILE* fp, int nx, int row_first, int row_count, int is_double,
                                   const void* u_x, const void* u_y, const void* u_mag,
                                   const void* pressure, const int* obstacles)
{
  int n_threads = 1;
#ifdef _OPENMP
  n_threads = omp_get_max_threads();
#endif
  /* rows per thread and round: keep each buffer around 4 MiB */
  int rows_per_task = (int)((4L << 20) / ((long)nx * LBM_LINE_MAX));
  if (rows_per_task < 1) rows_per_task = 1;
  const size_t buf_bytes = (size_t)rows_per_task * nx * LBM_LINE_MAX;
  char** buf = (char**)malloc(sizeof(char*) * (size_t)n_threads);
  size_t* used = (size_t*)malloc(sizeof(size_t) * (size_t)n_threads);
  if (buf == NULL || used == NULL) lbm_die("cannot allocate memory for output buffers", __LINE__, __FILE__);
  for (int t = 0; t < n_threads; t++) {
    buf[t] = (char*)malloc(buf_bytes);
    if (buf[t] == NULL) lbm_die("cannot allocate memory for output buffers", __LINE__, __FILE__);
  }

  for (int r0 = 0; r0 < row_count; r0 += rows_per_task * n_threads) {
#pragma omp parallel for schedule(static, 1)
    for (int t = 0; t < n_threads; t++) {
      const int begin = r0 + t * rows_per_task;
      int end = begin + rows_per_task;
      if (end > row_count) end = row_count;
      char* out = buf[t];
      for (int r = begin; r < end; r++) {
        const int jj = row_first + r;
        for (int ii = 0; ii < nx; ii++) {
          const size_t c = (size_t)r * nx + ii;
          /* the reference's format, SerialCode/d2q9-bgk.c:722 */
          out += snprintf(out, LBM_LINE_MAX, "%d %d %.12E %.12E %.12E %.12E %d\n", ii, jj, field_at(u_x, is_double, c),
                          field_at(u_y, is_double, c), field_at(u_mag, is_double, c), field_at(pressure, is_double, c),
                          obstacles[(size_t)jj * nx + ii]);
        }
      }
      used[t] = (size_t)(out - buf[t]);
    }
    for (int t = 0; t < n_threads; t++)
      if (used[t] > 0 && fwrite(buf[t], 1, used[t], fp) != used[t])
        lbm_die("could not write file output file", __LINE__, __FILE__);
  }
  for (int t = 0; t < n_threads; t++) free(buf[t]);
  free(buf);
  free(used);
}

void lbm_write_final_state_rows(FILE* fp, const lbm_params* params, int row_first, int row_count,
                                const float* u_x, const float* u_y, const float* u_mag,
                                const float* pressure, const int* obstacles)
{
  write_final_state_rows(fp, params->nx, row_first, row_count, 0, u_x, u_y, u_mag, pressure, obstacles);
}

void lbm_write_final_state_rows_double(FILE* fp, const lbm_params_double* params, int row_first, int row_count,
                                       const double* u_x, const double* u_y, const double* u_mag,
                                       const double* pressure, const int* obstacles)
{
  write_final_state_rows(fp, params->nx, row_first, row_count, 1, u_x, u_y, u_mag, pressure, obstacles);
}

/* av_vels.dat from floats or from doubles */
static void write_av_vels(const char* path, const void* av_vels, int is_double, int n)
{
  FILE* fp = fopen(path, "w");
  if (fp == NULL) lbm_die("could not open file output file", __LINE__, __FILE__);
  for (int ii = 0; ii < n; ii++) fprintf(fp, "%d:\t%.12E\n", ii, field_at(av_vels, is_double, (size_t)ii));
  fclose(fp);
}

void lbm_write_av_vels_double(const char* path, const double* av_vels, int n) { write_av_vels(path, av_vels, 1, n); }
void lbm_write_av_vels(const char* path, const float* av_vels, int n) { write_av_vels(path, av_vels, 0, n); }

void lbm_write_state_frame(const char* dir, const lbm_params* params, const lbm_window* window, int timestep,
                           const float* u_x, const float* u_y, const float* u_mag, const float* pressure,
                           const int* obstacles)
{
  char filename[4096];
  snprintf(filename, sizeof(filename), "%s/final_state_%06d.dat", dir, timestep);
  FILE* fp = fopen(filename, "w");
  if (fp == NULL) lbm_die("could not open state data file", __LINE__, __FILE__);
  for (int j = 0; j < window->ny; j++)
    for (int i = 0; i < window->nx; i++) {
      const size_t c = (size_t)j * (size_t)window->nx + (size_t)i;
      const int ii = window->x0 + i, jj = window->y0 + j;
      fprintf(fp, "%d %d %.12E %.12E %.12E %.12E %d\n", ii, jj, u_x[c], u_y[c], u_mag[c], pressure[c],
              obstacles[(size_t)jj * (size_t)params->nx + (size_t)ii]);
    }
  fclose(fp);
}

void lbm_write_animation_frame(const char* dir, int nx, int ny, int timestep, const float* u_mag)
{
  char filename[4096];
  snprintf(filename, sizeof(filename), "%s/velocity_magnitude_%06d.dat", dir, timestep);
  FILE* fp = fopen(filename, "w");
  if (fp == NULL) lbm_die("could not open animation data file", __LINE__, __FILE__);
  fprintf(fp, "# nx=%d ny=%d timestep=%d\n", nx, ny, timestep);
  const size_t n = (size_t)nx * (size_t)ny;
  for (size_t c = 0; c < n; c++) fprintf(fp, "%.6E\n", u_mag[c]);
  fclose(fp);
}
