/* options_check NAME=VALUE... -- lbm_parse_options (lbm-asynchronous_amd/host/lbm_options.c) over the given variables
   instead of the environment; prints the parsed options on one line.  Built by tests/test_cli_options.py from
   lbm_options.c and lbm_io.c alone, under AddressSanitizer and UBSan, as a stand-alone program. */
#include <stdio.h>
#include <string.h>

#include "../lbm-asynchronous_amd/host/lbm_options.h"

static int n_vars;
static char** vars;

static const char* lookup(const char* name)
{
  const size_t len = strlen(name);
  for (int i = 0; i < n_vars; i++)
    if (!strncmp(vars[i], name, len) && vars[i][len] == '=') return vars[i] + len + 1;
  return NULL;
}

int main(int argc, char* argv[])
{
  static const char* const mode[LBM_N_MODES] = {"PLAIN", "STEADY", "PROBES", "ANIMATION", "MEAN", "STATES", "FORCES"};
  static lbm_options o;
  n_vars = argc - 1;
  vars = argv + 1;
  lbm_parse_options(lookup, &o);
  printf("double=%d gpus=%d math=%s text=%d pressure_bin=%s tile=%d:%dx%d mode=%s every=%d tol=%g patience=%d from=%d order=%d "
         "window=%d,%d,%d,%d probes=%d", o.is_double, o.n_gpus, o.math_mode == LBM_MATH_FAST ? "fast" : "exact", o.write_text,
         o.pressure_bin ? o.pressure_bin : "-", o.tiled, o.tile_nx, o.tile_ny, mode[o.mode], o.every, o.steady_tol,
         o.steady_patience, o.mean_from, o.mean_order, o.window.x0, o.window.y0, o.window.nx, o.window.ny, o.n_probes);
  for (int i = 0; i < o.n_probes; i++) printf("%c%d,%d", i ? ';' : ':', o.probes[i].x, o.probes[i].y);
  printf("\n");
  return 0;
}
