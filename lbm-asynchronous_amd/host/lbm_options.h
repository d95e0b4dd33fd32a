/*
 * lbm_options.h -- everything the d2q9-bgk command line reads from its environment, parsed in one place (plain C99, no
 * engine calls).  The variables, their formats and what they do are listed at the head of d2q9-bgk.c.
 */
#ifndef LBM_OPTIONS_H
#define LBM_OPTIONS_H

#include "../../include/lbm_hip.h"

/* What the timestep loop does besides stepping: at most one of these.  The values index the option table of
   lbm_options.c, whose row 0 is LBM_PRECISION=double. */
typedef enum {
  LBM_MODE_PLAIN = 0, LBM_MODE_STEADY, LBM_MODE_PROBES, LBM_MODE_ANIMATION, LBM_MODE_MEAN, LBM_MODE_STATES, LBM_MODE_FORCES,
  LBM_MODE_STATS, LBM_N_MODES
} lbm_mode;

typedef struct {
  int is_double;               /* LBM_PRECISION=double */
  int n_gpus;                  /* LBM_GPUS, default 1 */
  int math_mode;               /* LBM_MATH: LBM_MATH_EXACT (default) or LBM_MATH_FAST */
  int write_text;              /* LBM_OUTPUT: 0 for "none" */
  const char* pressure_bin;    /* LBM_PRESSURE_BIN, NULL when unset or empty */
  int tiled, tile_nx, tile_ny; /* LBM_TILE=<tx>x<ty> */
  lbm_mode mode;
  int every;                   /* the mode's interval in steps; LBM_STEADY: check_every */
  double steady_tol;           /* LBM_STEADY */
  int steady_patience;
  int n_probes;                /* LBM_PROBES */
  lbm_probe probes[LBM_MAX_PROBES];
  int mean_from, mean_order;   /* LBM_MEAN, LBM_MEAN_ORDER (default 1) */
  lbm_window window;           /* LBM_STATES; nx == 0: the whole grid */
} lbm_options;

/* Reads every variable through `lookup` (main() passes getenv).  Dies through lbm_die -- message, exit(EXIT_FAILURE) --
   on a malformed value first, then on two table entries that cannot be combined; nothing else has happened by then. */
void lbm_parse_options(const char* (*lookup)(const char*), lbm_options* out);

#endif /* LBM_OPTIONS_H */
