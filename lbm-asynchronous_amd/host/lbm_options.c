/* lbm_options.c -- the environment of the d2q9-bgk command line: one number scanner, one parser per value format and one
   table of what cannot be combined. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lbm_io.h"
#include "lbm_options.h"

/* Row 0, then one row per lbm_mode in its order, then the switches that are no modes but are not offered in double.  Two
   rows that are both set are refused as "<earlier> and <later> cannot be combined"; against row 0, the rows marked
   not_offered as "<row> is not offered with LBM_PRECISION=double". */
enum { ROW_DOUBLE = 0, ROW_TILE = LBM_N_MODES, ROW_MEAN_ORDER, ROW_PRESSURE_BIN, ROW_GPUS, ROW_MATH_FAST, N_ROWS };
static const struct { const char* name; int not_offered; } rows[N_ROWS] = {
  {"LBM_PRECISION=double", 0}, {"LBM_STEADY", 1}, {"LBM_PROBES", 1}, {"LBM_ANIMATION", 1}, {"LBM_MEAN", 1},
  {"LBM_STATES", 0}, {"LBM_FORCES", 0}, {"LBM_STATS", 1},
  {"LBM_TILE", 1}, {"LBM_MEAN_ORDER", 1}, {"LBM_PRESSURE_BIN", 1}, {"LBM_GPUS", 1}, {"LBM_MATH=fast", 1},
};

static void refuse(int earlier, int later)
{
  char message[128];
  if (earlier == ROW_DOUBLE && rows[later].not_offered)
    snprintf(message, sizeof(message), "%s is not offered with %s", rows[later].name, rows[ROW_DOUBLE].name);
  else
    snprintf(message, sizeof(message), "%s and %s cannot be combined", rows[earlier].name, rows[later].name);
  lbm_die(message, __LINE__, __FILE__);
}

/* The one number format of LBM_PROBES, LBM_MEAN, LBM_MEAN_ORDER, LBM_STATES, LBM_FORCES and LBM_STATS: decimal digits only (no
   sign, no space, no exponent), at most 2147483647.  Reads one at *s and returns the character after it, which the caller
   compares with the separator it expects: that character is skipped, unless it is the '\0' at the end.  -1: no such
   number here. */
static int scan_number(const char** s, int* value)
{
  const char* p = *s;
  long long v = 0;
  if (*p < '0' || *p > '9') return -1;
  for (; *p >= '0' && *p <= '9'; p++)
    if ((v = v * 10 + (*p - '0')) > 2147483647LL) return -1;
  *value = (int)v;
  *s = *p ? p + 1 : p;
  return (unsigned char)*p;
}

/* LBM_STEADY=<tol>[:<check_every>[:<patience>]] */
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
    lbm_die("could not read LBM_STEADY: expected <tol>[:<check_every>[:<patience>]] with tol >= 0, check_every >= 1, patience >= 1", __LINE__, __FILE__);
  *check_every = (int)v[0];
  *patience = (int)v[1];
}

/* LBM_PROBES=x,y[;x,y...][:every] (every defaults to 1) */
static int parse_probes(const char* s, lbm_probe* cells, int* every)
{
  int n = 0, next;
  *every = 1;
  do {
    next = (n < LBM_MAX_PROBES && scan_number(&s, &cells[n].x) == ',') ? scan_number(&s, &cells[n].y) : -1;
    n++;
  } while (next == ';');
  if (next == ':') next = (scan_number(&s, every) == '\0' && *every >= 1) ? '\0' : -1;
  if (next != '\0')
    lbm_die("could not read LBM_PROBES: expected <x>,<y>[;<x>,<y>...][:<every>] with at most 256 cells and every >= 1", __LINE__, __FILE__);
  return n;
}

/* LBM_MEAN=<every>[:<from>] (from defaults to 0) */
static void parse_mean(const char* s, int* every, int* from)
{
  int next = scan_number(&s, every);
  *from = 0;
  if (next == ':') next = scan_number(&s, from);
  if (next != '\0' || *every < 1)
    lbm_die("could not read LBM_MEAN: expected <every>[:<from>] with every >= 1 and from >= 0", __LINE__, __FILE__);
}

/* LBM_STATES=<every>[:<x0>,<y0>,<nx>,<ny>] (the window defaults to the whole grid: nx = 0 here) */
static void parse_states(const char* s, int* every, lbm_window* window)
{
  int* const v[5] = {every, &window->x0, &window->y0, &window->nx, &window->ny};
  int n = 0, next;
  do next = scan_number(&s, v[n]);
  while (++n < 5 && next == (n == 1 ? ':' : ','));
  if (next != '\0' || (n != 1 && n != 5) || *every < 1 || (n == 5 && (window->nx < 1 || window->ny < 1)))
    lbm_die("could not read LBM_STATES: expected <every>[:<x0>,<y0>,<nx>,<ny>] with every >= 1, nx >= 1 and ny >= 1", __LINE__, __FILE__);
}

void lbm_parse_options(const char* (*lookup)(const char*), lbm_options* out)
{
  const char* value[N_ROWS]; /* a row's variable where it is set and not empty, else NULL */
  int every[LBM_N_MODES] = {0};
  const char* v;
  memset(out, 0, sizeof(*out));
  for (int r = 0; r < N_ROWS; r++) {
    v = lookup(r == ROW_DOUBLE ? "LBM_PRECISION" : r == ROW_MATH_FAST ? "LBM_MATH" : rows[r].name);
    value[r] = (v && *v) ? v : NULL;
  }

  /* malformed values first */
  if ((v = value[LBM_MODE_STATES])) parse_states(v, &every[LBM_MODE_STATES], &out->window);
  if ((v = value[LBM_MODE_FORCES]) && (scan_number(&v, &every[LBM_MODE_FORCES]) != '\0' || every[LBM_MODE_FORCES] < 1))
    lbm_die("could not read LBM_FORCES: expected <every> with every >= 1", __LINE__, __FILE__);
  if ((v = value[LBM_MODE_STATS]) && (scan_number(&v, &every[LBM_MODE_STATS]) != '\0' || every[LBM_MODE_STATS] < 1))
    lbm_die("could not read LBM_STATS: expected <every> with every >= 1", __LINE__, __FILE__);
  out->is_double = (v = value[ROW_DOUBLE]) && !strcmp(v, "double");
  if (v && !out->is_double && strcmp(v, "single")) lbm_die("could not read LBM_PRECISION: expected single or double", __LINE__, __FILE__);
  out->n_gpus = value[ROW_GPUS] ? atoi(value[ROW_GPUS]) : 1;
  if (out->n_gpus == 1) value[ROW_GPUS] = NULL;
  if (value[ROW_MATH_FAST] && strcmp(value[ROW_MATH_FAST], "fast")) value[ROW_MATH_FAST] = NULL;
  out->math_mode = value[ROW_MATH_FAST] ? LBM_MATH_FAST : LBM_MATH_EXACT;
  out->write_text = !((v = lookup("LBM_OUTPUT")) && !strcmp(v, "none"));
  out->pressure_bin = value[ROW_PRESSURE_BIN];
  out->tiled = value[ROW_TILE] && sscanf(value[ROW_TILE], "%dx%d", &out->tile_nx, &out->tile_ny) == 2;
  if ((v = value[LBM_MODE_STEADY])) parse_steady(v, &out->steady_tol, &every[LBM_MODE_STEADY], &out->steady_patience);
  if ((v = value[LBM_MODE_PROBES])) out->n_probes = parse_probes(v, out->probes, &every[LBM_MODE_PROBES]);
  if ((v = value[LBM_MODE_MEAN])) parse_mean(v, &every[LBM_MODE_MEAN], &out->mean_from);
  out->mean_order = 1;
  if ((v = value[ROW_MEAN_ORDER]) && (scan_number(&v, &out->mean_order) != '\0' || out->mean_order < 1 || out->mean_order > 2))
    lbm_die("could not read LBM_MEAN_ORDER: expected 1 or 2", __LINE__, __FILE__);
  if (value[LBM_MODE_ANIMATION]) every[LBM_MODE_ANIMATION] = atoi(value[LBM_MODE_ANIMATION]);

  /* then the table: double against every row that is set (LBM_ANIMATION=0 too), the modes against each other */
  for (int r = 1; out->is_double && r < N_ROWS; r++)
    if (value[r]) refuse(ROW_DOUBLE, r);
  if (value[ROW_MEAN_ORDER] && every[LBM_MODE_MEAN] == 0) lbm_die("LBM_MEAN_ORDER needs LBM_MEAN", __LINE__, __FILE__);
  for (int r = 1; r < LBM_N_MODES; r++) {
    if (every[r] <= 0) continue;
    if (out->mode != LBM_MODE_PLAIN) refuse(out->mode, r);
    out->mode = (lbm_mode)r;
    out->every = every[r];
  }
}
