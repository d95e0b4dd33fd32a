"""The 50 forms of the resident kernel, and the GPU cases that launch every one of them.

TEST INFRASTRUCTURE: numpy and the oracle binding only, no GPU.  tests/test_resident_forms.py checks all of this on the CPU
against the planner (tests/plan_dump.cpp: "plan" and "resident_form"); tests/test_gpu_resident_forms.py runs every case
against the oracle bit for bit.

lbm::resident_band<MAXT, JOINT, ROWS, BATCH, REC> (lbm-asynchronous_amd/csrc/lbm_kernels.hip.h) is compiled in
2 (BATCH) x 5 (REC: none, frames, probes, mean, fields) x 5 shapes = 50 forms: resident_form<BATCH, REC>(shape) in
lbm_hip.hip, the shape being lbm_plan::resident_form(nx, rows, joint) (lbm_plan.h):

    0  <1024, false, 2>   two-row bands, nx > 512
    1  <512, false, 2>    two-row bands, nx <= 512
    2  <1024, false, 4>   four-row bands, nx > 512
    3  <512, true, 4>     four-row bands, JOINT
    4  <512, false, 4>    four-row bands, not JOINT

CASES names one case per form at the smallest shape that still has what the form can get wrong (GEOMETRY), five more
for the batch placement that is not one-XCD (shape 1 at 320 columns) and four whose chunk is two launches.

What the recorder tests that existed before launch -- their (nx, ny, env) lists through the planner at 256 CUs.  The
planner prefers two-row bands whenever ny / 2 <= CUs and sets resident_joint with four-row bands only, so most of them
run shapes 0 and 1 whatever their environment asks of JOINT (tests/test_resident_forms.py fails when this table moves):

    nx x ny     environment                                    rows  joint  form   modules (see EXISTING_USERS)
    128 x 16    -                                              2     0      1      frames probes mean moments fields
    128 x 64    LBM_RESIDENT_ROWS=4                            4     1      3      frames probes mean moments fields
    256 x 64    LBM_RESIDENT_JOINT=0                           2     0      1      frames probes mean
    320 x 24    LBM_RESIDENT_JOINT=1                           2     0      1      frames probes mean moments fields
    1024 x 128  LBM_RESIDENT_XCD=0                             2     0      0      frames probes mean
    1024 x 64   -                                              2     0      0      frames probes mean moments fields
    512 x 64    LBM_RESIDENT_ROWS=2                            2     0      1      frames probes mean
    128 x 128   LBM_RESIDENT_ONE_XCD=0 LBM_RESIDENT_GROUP=4    2     0      1      frames probes mean moments fields
    128 x 64    LBM_RESIDENT_GROUP=2 LBM_RESIDENT_XCD=0        2     0      1      frames probes mean
    128 x 128   - (every batched recorder test, 8 members)     2     0      1      one-XCD placement, one launch
    128 x 256   - (reference data set)                         2     0      1      frames probes mean
    256 x 256   - (reference data set)                         2     0      1      frames probes mean
    1024 x 1024 - (reference data set)                         4     0      2      frames probes mean

So before tests/test_gpu_resident_forms.py shape 4 was launched by no test at all, shape 2 by a single engine only (plain,
and with frames, probes and order-1 mean fields through the 1024 x 1024 data set; never with field frames or second
moments), and a batch recorded on shape 1 only, one-XCD, in one launch.
"""
import functools

import numpy as np

REC = ("none", "frames", "probes", "mean", "fields")        # kRecNone .. kRecFields, the order of resident_kernel()'s table
# shape -> (MAXT, JOINT, ROWS), resident_form<BATCH, REC>'s switch
SHAPES = {0: (1024, False, 2), 1: (512, False, 2), 2: (1024, False, 4), 3: (512, True, 4), 4: (512, False, 4)}
# resident_kernel(): forms[batch][rec](shape)
FORMS = [(batch, rec, shape) for batch in (0, 1) for rec in REC for shape in sorted(SHAPES)]

CUS = 256                       # the cases are planned for the MI355X's CU count
CALLS = (1, 2, 19, 5)           # a sample on step 0 = a call's last step (accel_last), on the first and last step of a launch, inside one
STEPS = sum(CALLS)

# the (nx, ny, env) of the recorder tests that existed before this table, and the form each really launches
EXISTING = [
    (128, 16, {}, 1), (128, 64, {"LBM_RESIDENT_ROWS": "4"}, 3), (256, 64, {"LBM_RESIDENT_JOINT": "0"}, 1),
    (320, 24, {"LBM_RESIDENT_JOINT": "1"}, 1), (1024, 128, {"LBM_RESIDENT_XCD": "0"}, 0), (1024, 64, {}, 0),
    (512, 64, {"LBM_RESIDENT_ROWS": "2"}, 1), (128, 128, {"LBM_RESIDENT_ONE_XCD": "0", "LBM_RESIDENT_GROUP": "4"}, 1),
    (128, 64, {"LBM_RESIDENT_GROUP": "2", "LBM_RESIDENT_XCD": "0"}, 1), (128, 128, {}, 1),
    (128, 256, {}, 1), (256, 256, {}, 1), (1024, 1024, {}, 2)]          # test_resident_reference_datasets: frames, probes, mean
# module -> (the name of its parameter list's test, how many of EXISTING's first nine it runs)
EXISTING_USERS = {"test_gpu_frames": ("test_resident_random_lattices", 9), "test_gpu_probes": ("test_resident_random_lattices", 9),
                  "test_gpu_mean": ("test_resident_random_lattices", 9), "test_gpu_moments": ("test_resident_forms", 5),
                  "test_gpu_fields": ("test_resident_random_lattices", 5)}

# ---------------------------------------------------------------------------------------------------------------------
# the shapes
# ---------------------------------------------------------------------------------------------------------------------
# Twelve rows are three four-row bands (a band's south and north neighbours differ; eight rows would make them one band)
# and six two-row bands; the lid row is 10, and 10 % 4 == 2 as the recorder forms of four-row bands require.
#   576 columns: nine waves per band, one more than a 512-thread form holds;   128: two waves, the one-XCD placement;
#   320: five waves, not one-XCD, and four-row bands that are not JOINT (nx > 256)
ROWS4 = {"LBM_RESIDENT_ROWS": "4"}
# name -> (nx, ny, env, shape, rows, one_xcd)
GEOMETRY = {
    "576x12": (576, 12, {}, 0, 2, 0), "128x12": (128, 12, {}, 1, 2, 1), "320x12": (320, 12, {}, 1, 2, 0),
    "576x12-rows4": (576, 12, ROWS4, 2, 4, 0), "128x12-rows4": (128, 12, ROWS4, 3, 4, 0), "320x12-rows4": (320, 12, ROWS4, 4, 4, 0),
    # a chunk of two launches: 128 (64) bands leave room for 2 (4) members per launch, and 128 % 8 == 64 % 8 == 0, so the
    # XCD-affinity band permutation runs inside every member
    "576x256": (576, 256, {}, 0, 2, 0), "320x256-rows4": (320, 256, ROWS4, 4, 4, 0)}
GEOMETRY_OF_SHAPE = {0: "576x12", 1: "128x12", 2: "576x12-rows4", 3: "128x12-rows4", 4: "320x12-rows4"}


class Case:
    """One engine (members == 1, batch == 0) or batch configuration.  kind: "form" (the one case that claims the form),
    "placement" (shape 1 with members at blockIdx.x / round_up(member_wgs, 8)) or "two-launch" (an armed member in the
    second launch of a chunk).  expect: what Engine.info() must report; per_launch / launches: Batch.info()'s
    members_per_launch and launches_per_chunk."""

    def __init__(self, batch, rec, geometry, kind="form", members=None, per_launch=None):
        self.batch, self.rec, self.geometry, self.kind = batch, rec, geometry, kind
        self.nx, self.ny, env, self.shape, self.rows, self.one_xcd = GEOMETRY[geometry]
        self.env = dict(env, LBM_RESIDENT_MIN_STEPS="1")
        self.form = (batch, rec, self.shape)
        self.members = members if members is not None else (3 if batch else 1)
        self.bands = self.ny // self.rows
        self.expect = {"resident_rows": self.rows, "resident_group": 1, "resident_one_xcd": self.one_xcd}
        # lbm_create_batch: 8 one-XCD members per launch; else floor(CUs / bands), thinned until no XCD is dealt more
        # working workgroups than it has CUs
        self.per_launch = per_launch if per_launch is not None else (8 if self.one_xcd else None)
        self.launches = -(-self.members // self.per_launch) if self.per_launch else None
        self.id = f"{'batch' if batch else 'single'}-{rec}-form{self.shape}-{geometry}" + (f"-{kind}" if kind != "form" else "")

    # the members: (first armed, second armed, unarmed).  A two-launch case arms a member of the first launch and the
    # last member, which runs in the second
    @property
    def armed(self):
        if not self.batch:
            return (0,)
        return (0, self.members - 1)

    @property
    def unarmed(self):
        return [i for i in range(self.members) if i not in self.armed]


def members_per_launch(bands, cus=CUS):
    """lbm_create_batch's co-residency rule for shapes that are not one-XCD."""
    mpl = cus // bands
    while mpl > 1 and mpl * -(-bands // 8) > cus // 8:
        mpl -= 1
    return max(mpl, 1)


def _cases():
    out = []
    for batch, rec, shape in FORMS:
        geometry = GEOMETRY_OF_SHAPE[shape]
        bands = GEOMETRY[geometry][1] // GEOMETRY[geometry][4]
        out.append(Case(batch, rec, geometry, per_launch=None if (not batch or GEOMETRY[geometry][5]) else members_per_launch(bands)))
    for rec in REC:
        out.append(Case(1, rec, "320x12", "placement", per_launch=members_per_launch(6)))
    for rec in ("frames", "probes"):
        out.append(Case(1, rec, "576x256", "two-launch", members=3, per_launch=members_per_launch(128)))
    for rec in ("mean", "fields"):
        out.append(Case(1, rec, "320x256-rows4", "two-launch", members=5, per_launch=members_per_launch(64)))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), "case ids must be unique"
    return out


CASES = _cases()


# ---------------------------------------------------------------------------------------------------------------------
# the lattices
# ---------------------------------------------------------------------------------------------------------------------
def wave_edge_columns(nx):
    """Both sides of the first wave seam, the two ends of a row, and for the 1024-thread forms the seam behind the
    eighth wave and the last column."""
    return sorted({0, 63, 64, nx - 1} | ({511, 512, 575} if nx == 576 else set()))


def mark_rows(ny):
    """Rows that get blocked cells at the wave edges: a four-row band's rows 0, 1 and 3 (two-row bands: both rows of one,
    the upper of the next), and the row below the lid row -- the lid row itself keeps fluid cells there for the probes."""
    return (0, 1, 3, ny - 3)


@functools.lru_cache(maxsize=None)
def lattice(nx, ny):
    """(Params, obstacles, cells) of member 0: test_gpu_parity.random_case without side walls, so both wraps are live, with
    blocked cells on the lid row, on both seam rows of every band (of four rows and of two) and at the wave edges."""
    import conftest
    from test_gpu_parity import random_case
    p, ob, cells = random_case(conftest.load_package(), nx, ny, nx + 7 * ny, blocked_frac=0.05, walls=False)
    ob[ny - 2, ::5] = 1                     # lid row
    ob[ny - 2, [x for x in wave_edge_columns(nx) + [1] if x % 5]] = 0       # ... with fluid cells at the wave seams
    ob[3::4, ::7] = 1                       # seam rows of four-row bands: a band's last row ...
    ob[0::4, 3::7] = 1                      # ... and its first
    ob[1::4, 5::9] = 1                      # the interior pair of a four-row band: seam rows of two-row bands
    ob[2::4, 6::13] = 1
    for y in mark_rows(ny):
        ob[y, wave_edge_columns(nx)] = 1
    ob.setflags(write=False)
    cells.setflags(write=False)
    return p, ob, cells


@functools.lru_cache(maxsize=None)
def member_inputs(nx, ny, members):
    """(params, obstacles, cells) of a batch: every member its own omega and accel, the obstacle map rolled along x and the
    lattice along y (the lid row keeps its blocked cells).  Member 0 is lattice(nx, ny)."""
    import conftest
    lbm = conftest.load_package()
    p0, ob0, c0 = lattice(nx, ny)
    params = [p0] + [lbm.Params(nx, ny, p0.max_iters, p0.reynolds_dim, p0.density, float(np.float32(0.005 + 0.001 * i)),
                                float(np.float32(1.85 - 0.04 * i))) for i in range(1, members)]
    obstacles = [np.roll(ob0, i, axis=1) for i in range(members)]
    cells = [np.roll(c0, i, axis=0) for i in range(members)]
    for a in (*obstacles, *cells):
        a.setflags(write=False)
    return params, obstacles, cells


def inputs(case, member=0):
    params, obstacles, cells = member_inputs(case.nx, case.ny, case.members)
    return params[member], obstacles[member], cells[member]


_models = {}


def model(case, member=0):
    """The oracle's run of one member for STEPS steps: (lattice, the per-step `moment` speed maps the resident kernel's
    av_vels are summed from -- av_model.step_speeds; twelve-row shapes only, where the plain forms' cases are), computed
    once per lattice and never changed."""
    import av_model
    import oracle_binding
    key = (case.nx, case.ny, case.members, member)
    if key not in _models:
        oracle = oracle_binding.load()
        p, ob, cells = inputs(case, member)
        ref = cells.copy()
        oracle.run(p, ref, ob, STEPS)
        ref.setflags(write=False)
        moment = None
        if case.ny <= 16:
            speeds = av_model.step_speeds(oracle, p, ob, cells, STEPS)
            assert np.array_equal(speeds.cells.view(np.uint32), ref.view(np.uint32))
            moment = speeds.moment
        _models[key] = (ref, moment)
    return _models[key]


# ---------------------------------------------------------------------------------------------------------------------
# what the recorders are asked for
# ---------------------------------------------------------------------------------------------------------------------
EVERY = (3, 4)                  # the first and the second armed member
# ring capacities below the run's records (9 and 7 frames, 27 sample rows), at least the longest call's (7, 5, 19): the
# slot index wraps, and the second member's ring is another size than the first's
CAPACITY = (7, 6)
PROBE_CAPACITY = (19, 6)


def probe_sets(nx, ny):
    """(with the lid row, without it): the wave-edge columns (and one x >= 512 where there are that many) on the lid row,
    on both seam rows of a four-row band (4 and 7; each a seam row of a two-row band) and on its interior rows (5, 6);
    the periodic seam; a duplicate.  Only a band with a probe ON the lid row defers the lid's acceleration."""
    cols = wave_edge_columns(nx) + ([530] if nx > 512 else [])
    off = [(x, y) for y in (4, 7, 5, 6) for x in cols] + [(5, 0), (7, ny - 1), (nx // 3, ny - 3), (nx // 3, ny - 1)]
    off.append(off[2])
    lid = [(x, ny - 2) for x in cols] + [(nx // 3, ny - 2), (1, ny - 2)] + off
    return lid, off


def field_windows(nx, ny):
    """The whole grid; the lid row and the row below it across the wave seam(s); rows 1..2, the interior pair of a four-row
    band; and the window of the field subset."""
    x1 = 516 if nx > 512 else 70
    return {"whole": None, "lid-seam": (60, ny - 3, x1 - 60, 2), "rows-1-2": (5, 1, nx - 9, 2), "subset": (11, 1, 70, ny - 3)}


SUBSET = ("u_x", "pressure")
