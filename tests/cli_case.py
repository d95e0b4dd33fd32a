"""The one way the tests run the d2q9-bgk command line: two input files written into a directory, the program run there
with the given variables and with none of its own inherited from the caller's environment."""
import os
import subprocess

# every variable the option table of lbm-asynchronous_amd/host/lbm_options.c reads
CLI_VARS = ("LBM_PRECISION", "LBM_STEADY", "LBM_PROBES", "LBM_ANIMATION", "LBM_MEAN", "LBM_STATES", "LBM_FORCES", "LBM_TILE",
            "LBM_MEAN_ORDER", "LBM_PRESSURE_BIN", "LBM_GPUS", "LBM_MATH", "LBM_OUTPUT")

# a 64 x 16 channel whose bottom row is blocked, 10 steps: the case of the tests that never reach a device
SMALL_PARAMS = "64\n16\n10\n16\n0.1\n0.005\n1.0\n"
SMALL_OBSTACLES = "".join("%d 0 1\n" % x for x in range(64))


def params_text(p):
    return "%d\n%d\n%d\n%d\n%.9g\n%.9g\n%.9g\n" % (p.nx, p.ny, p.max_iters, p.reynolds_dim, p.density, p.accel, p.omega)


def obstacles_text(ob):
    ys, xs = ob.nonzero()
    return "".join("%d %d 1\n" % (x, y) for y, x in zip(ys, xs))


def run_cli(lbm, tmp_path, params=SMALL_PARAMS, obstacles=SMALL_OBSTACLES, **env):
    """Writes the texts `params` and `obstacles` to input.params / obstacles.dat in tmp_path (created if missing), runs
    d2q9-bgk there with `env` on top of the cleaned environment and returns the CompletedProcess."""
    if not os.path.exists(lbm.CLI_PATH):
        lbm.build()
    os.makedirs(tmp_path, exist_ok=True)
    pf, of = os.path.join(tmp_path, "input.params"), os.path.join(tmp_path, "obstacles.dat")
    with open(pf, "w") as f:
        f.write(params)
    with open(of, "w") as f:
        f.write(obstacles)
    clean = {k: v for k, v in os.environ.items() if k not in CLI_VARS}
    return subprocess.run([lbm.CLI_PATH, pf, of], cwd=tmp_path, capture_output=True, text=True, env=dict(clean, **env), timeout=120)


# ---- the corpus of tests/test_cli_options.py and tools/cli_ab.sh ------------------------------------------------------
# values the parser must refuse with "could not read <NAME>"; the *_abi tests run each through the program itself
MALFORMED = {
    "LBM_STATES": ["abc", "0", "-5", "10:", "10:x", "10:-1", ":5", "10,5", "10:5:2", "10 ", " 10", "+10", "1e2", "99999999999",
                   "10:1,2,3", "10:1,2,0,4", "10:1,2,3,0", "10:a,b,c,d", "10:1,2,3,4,5", "10:1,2,3,4:5", "10:1,2,3,",
                   "10:1,-2,3,4", "10:1,2,3,99999999999", "10:1;2;3;4"],
    "LBM_MEAN": ["abc", "0", "-5", "10:", "10:x", "10:-1", ":5", "10,5", "10:5:2", "10 ", " 10", "+10", "1e2", "99999999999"],
    "LBM_MEAN_ORDER": ["0", "3", "2x", " 2", "+2", "12", "-2", "2 "],          # with LBM_MEAN=10:2
    "LBM_PROBES": ["abc", "1,2;", "1,2:0", "1,2:x", "1;2", "-1,2", "1,2 "],
    "LBM_STEADY": ["abc", "1e-3:", "1e-3:0", "1e-3:512:0", "1e-3:512:2:9", "-1", "1e-3:x", "1e-3 "],
    "LBM_FORCES": ["-5", "ten", "10x"],
}
MANY_PROBES = ";".join("%d,%d" % (i, 2 * i) for i in range(257))                # 257 cells: one more than LBM_MAX_PROBES
# at the edges: 257 probes, and 2^31 where 2^31 - 1 is the largest number
MALFORMED_EDGES = [{"LBM_PROBES": MANY_PROBES}, {"LBM_PROBES": "1,2:2147483648"}, {"LBM_PROBES": "2147483648,2"},
                   {"LBM_FORCES": "2147483648"}, {"LBM_MEAN": "2147483648"}, {"LBM_MEAN": "10:2147483648"},
                   {"LBM_STATES": "2147483648"}, {"LBM_STATES": "10:0,0,2147483648,1"}]

PLAIN = dict(double=0, gpus=1, math="exact", text=1, pressure_bin="-", tile="0:0x0", mode="PLAIN", every=0, tol="0", patience=0,
             **{"from": 0}, order=1, window="0,0,0,0", probes="0")
# (variables, what tests/options_check prints for them where it differs from PLAIN)
VALID = [
    ({}, {}),
    ({"LBM_PROBES": MANY_PROBES.rsplit(";", 1)[0]},
     dict(mode="PROBES", every=1, probes="256:" + MANY_PROBES.rsplit(";", 1)[0])),
    ({"LBM_PROBES": "2147483647,0;5,2147483647:2147483647"},
     dict(mode="PROBES", every=2147483647, probes="2:2147483647,0;5,2147483647")),
    ({"LBM_FORCES": "2147483647"}, dict(mode="FORCES", every=2147483647)),
    ({"LBM_STATES": "2147483647"}, dict(mode="STATES", every=2147483647)),
    ({"LBM_STATES": "100:3,2,40,30"}, dict(mode="STATES", every=100, window="3,2,40,30")),
    ({"LBM_STATES": "1:0,2147483647,1,2147483647"}, dict(mode="STATES", every=1, window="0,2147483647,1,2147483647")),
    ({"LBM_MEAN": "7:0"}, dict(mode="MEAN", every=7)),
    ({"LBM_MEAN": "2147483647:2147483647", "LBM_MEAN_ORDER": "2"},
     dict(mode="MEAN", every=2147483647, order=2, **{"from": 2147483647})),
    ({"LBM_MEAN": "10", "LBM_MEAN_ORDER": "1"}, dict(mode="MEAN", every=10)),
    ({"LBM_STEADY": "1e-6"}, dict(mode="STEADY", every=1024, tol="1e-06", patience=2)),
    ({"LBM_STEADY": "0:2147483647:2147483647"}, dict(mode="STEADY", every=2147483647, tol="0", patience=2147483647)),
    ({"LBM_ANIMATION": "100"}, dict(mode="ANIMATION", every=100)),
    ({"LBM_ANIMATION": "abc", "LBM_GPUS": "2", "LBM_MATH": "fast", "LBM_OUTPUT": "none", "LBM_PRESSURE_BIN": "p.bin",
      "LBM_TILE": "128x64", "LBM_PRECISION": "single"},
     dict(gpus=2, math="fast", text=0, pressure_bin="p.bin", tile="1:128x64")),
    ({"LBM_PRECISION": "double", "LBM_GPUS": "1", "LBM_MATH": "exact"}, dict(double=1)),
]

# the option table, in its order, each entry with a value that sets it
TABLE = [("LBM_PRECISION=double", {"LBM_PRECISION": "double"}), ("LBM_STEADY", {"LBM_STEADY": "1e-6"}),
         ("LBM_PROBES", {"LBM_PROBES": "1,2"}), ("LBM_ANIMATION", {"LBM_ANIMATION": "100"}), ("LBM_MEAN", {"LBM_MEAN": "10:2"}),
         ("LBM_STATES", {"LBM_STATES": "10"}), ("LBM_FORCES", {"LBM_FORCES": "50"})]


def malformed_cases():
    """[(variables, NAME)]: the program must end with "could not read NAME"."""
    cases = [({name: value, **({"LBM_MEAN": "10:2"} if name == "LBM_MEAN_ORDER" else {})}, name)
             for name, values in MALFORMED.items() for value in values]
    return cases + [(env, next(iter(env))) for env in MALFORMED_EDGES]


def pair_cases():
    """[(variables, message)]: the 21 pairs of TABLE and the one message each is refused with."""
    cases = []
    for i, (earlier, env_i) in enumerate(TABLE):
        for later, env_j in TABLE[i + 1:]:
            if i == 0 and later not in ("LBM_STATES", "LBM_FORCES"):
                message = "%s is not offered with LBM_PRECISION=double" % later
            else:
                message = "%s and %s cannot be combined" % (earlier, later)
            cases.append((dict(env_i, **env_j), message))
    return cases


def printed(expect):
    return " ".join("%s=%s" % kv for kv in dict(PLAIN, **expect).items())


if __name__ == "__main__":      # one case per line, NAME=VALUE separated by tabs: what tools/cli_ab.sh reads
    for env, _ in malformed_cases() + VALID + pair_cases():
        print("\t".join("%s=%s" % kv for kv in env.items()))
