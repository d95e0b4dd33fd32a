/* stats_options_check NAME=VALUE... -- lbm_parse_options (lbm-asynchronous_amd/host/lbm_options.c) over the given
   variables instead of the environment; prints whether the mode is LBM_MODE_STATS, the mode's number and its interval.
   Built by tests/test_stats_abi.py from lbm_options.c and lbm_io.c alone, under AddressSanitizer and UBSan, as a
   stand-alone program (tests/options_check.c names the modes it was written with). */
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
  static lbm_options o;
  n_vars = argc - 1;
  vars = argv + 1;
  lbm_parse_options(lookup, &o);
  printf("stats=%d mode=%d of %d every=%d double=%d\n", o.mode == LBM_MODE_STATS, (int)o.mode, (int)LBM_N_MODES, o.every, o.is_double);
  return 0;
}
