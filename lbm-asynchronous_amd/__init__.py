"""Python host-side binding of the MI355X D2Q9-BGK engine (ctypes over the C ABI).

The directory name carries a hyphen (it mirrors the reference repository's name), so load it
with :func:`importlib` -- ``tests/conftest.py`` and ``bench.py`` do::

    spec = importlib.util.spec_from_file_location("lbm_asynchronous_amd", ".../__init__.py")

Everything here is plumbing around ``liblbm_hip.so`` (``include/lbm_hip.h``): numpy arrays in the
reference's host layouts go in, numpy arrays come out.  There is no Python or CPU compute path;
if the shared library is missing or no HIP device is usable, calls raise :class:`LbmError`.

Reference interfaces mirrored (``/root/reference/SerialCode/d2q9-bgk.c``):
``t_param`` (:66-75) -> :class:`Params`; ``initialise`` file formats (:460-613) ->
:func:`read_params`, :func:`read_obstacles`; the ``timestep``/``av_velocity`` loop (:166-170) ->
:meth:`Engine.run`, for many lattices at once :meth:`Batch.run`; ``write_values`` (:662-743) ->
:func:`write_final_state`, :func:`write_av_vels`; its time average :meth:`Engine.mean`, :func:`write_mean_state`, and the
fluctuations about it :meth:`Engine.fluctuations`, :func:`write_rms_state`.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LBM_LIB") or os.path.join(_HERE, "liblbm_hip.so")   # LBM_LIB: experiments only
CLI_PATH = os.path.join(_HERE, "d2q9-bgk")

MATH_EXACT = 0
MATH_FAST = 1
_MATH = {"exact": MATH_EXACT, "fast": MATH_FAST, MATH_EXACT: MATH_EXACT, MATH_FAST: MATH_FAST}
RCCL_ID_BYTES = 128
MASK_HALO_ROWS = 3        # LBM_MASK_HALO_ROWS of include/lbm_hip.h
HALO_SYNC = 0
HALO_STALE = 1
HALO_FRESHEST = 2
_HALO = {"sync": HALO_SYNC, "stale": HALO_STALE, "freshest": HALO_FRESHEST,
         HALO_SYNC: HALO_SYNC, HALO_STALE: HALO_STALE, HALO_FRESHEST: HALO_FRESHEST}

# every symbol include/lbm_hip.h declares (tests check the .so exports them all)
ABI_SYMBOLS = (
    "lbm_set_error_mode", "lbm_last_error", "lbm_version", "lbm_device_count",
    "lbm_partition_rows", "lbm_halo_plan", "lbm_plan_halo_depth", "lbm_create", "lbm_rccl_unique_id", "lbm_rccl_info", "lbm_create_rank", "lbm_create_rank_rows",
    "lbm_create_tiled", "lbm_create_rank_tiled", "lbm_create_rank_hosted", "lbm_create_rank_hosted_rows",
    "lbm_create_rank_hosted_tiled", "lbm_destroy",
    "lbm_get_info", "lbm_set_halo_mode", "lbm_read_halo_log", "lbm_run", "lbm_sync", "lbm_run_timed", "lbm_read_av_vels", "lbm_read_cells",
    "lbm_read_final_state", "lbm_av_velocity", "lbm_total_density", "lbm_calc_reynolds",
    "lbm_set_frames", "lbm_read_frames", "lbm_set_probes", "lbm_read_probes", "lbm_set_mean", "lbm_read_mean", "lbm_set_mean_order",
    "lbm_set_field_frames", "lbm_read_field_frames", "lbm_set_forces", "lbm_read_forces", "lbm_forces_links",
    "lbm_run_until", "lbm_batch_run_until",
    "lbm_create_batch", "lbm_batch_member", "lbm_batch_run", "lbm_batch_sync", "lbm_batch_get_info", "lbm_destroy_batch",
    "lbm_batch_set_forces", "lbm_batch_read_forces", "lbm_batch_forces_links",
    "lbm_set_stats", "lbm_read_stats", "lbm_batch_set_stats", "lbm_batch_read_stats",
    "lbm_set_residual", "lbm_read_residual", "lbm_batch_set_residual", "lbm_batch_read_residual",
    "lbm_run_until_residual", "lbm_batch_run_until_residual",
    "lbm_set_profiles", "lbm_read_profiles", "lbm_batch_set_profiles", "lbm_batch_read_profiles",
    "lbm_read_coarse", "lbm_set_coarse_frames", "lbm_read_coarse_frames", "lbm_batch_set_coarse_frames", "lbm_batch_read_coarse_frames",
    "lbm_read_vorticity", "lbm_set_enstrophy", "lbm_read_enstrophy", "lbm_batch_set_enstrophy", "lbm_batch_read_enstrophy",
    "lbm_read_psi", "lbm_set_psi", "lbm_read_psi_rows", "lbm_batch_set_psi", "lbm_batch_read_psi_rows",
    "lbm_read_stress", "lbm_set_stress", "lbm_read_stress_rows", "lbm_batch_set_stress", "lbm_batch_read_stress_rows",
    "lbm_set_tracers", "lbm_read_tracers", "lbm_tracers_now", "lbm_batch_set_tracers", "lbm_batch_read_tracers", "lbm_batch_tracers_now",
    "lbm_double_create", "lbm_double_destroy", "lbm_double_get_info", "lbm_double_run", "lbm_double_run_timed",
    "lbm_double_sync", "lbm_double_read_av_vels", "lbm_double_read_cells", "lbm_double_read_final_state",
    "lbm_double_av_velocity", "lbm_double_total_density", "lbm_double_calc_reynolds",
)
# declared and exported too, kept apart: ABI_SYMBOLS is compared with a scan of the header for names of letters and
# underscores (tests/test_abi.py), which a name that ends in a digit is not
ABI_SYMBOLS_NUMBERED = ("lbm_read_mean2",)


class LbmError(RuntimeError):
    pass


class _CParams(ctypes.Structure):
    _fields_ = [("nx", ctypes.c_int), ("ny", ctypes.c_int), ("max_iters", ctypes.c_int),
                ("reynolds_dim", ctypes.c_int), ("density", ctypes.c_float),
                ("accel", ctypes.c_float), ("omega", ctypes.c_float)]


class _CParamsDouble(ctypes.Structure):
    _fields_ = [("nx", ctypes.c_int), ("ny", ctypes.c_int), ("max_iters", ctypes.c_int),
                ("reynolds_dim", ctypes.c_int), ("density", ctypes.c_double),
                ("accel", ctypes.c_double), ("omega", ctypes.c_double)]


class _CDoubleInfo(ctypes.Structure):
    _fields_ = [("fluid_cells", ctypes.c_int), ("steps_done", ctypes.c_int), ("lane_cells", ctypes.c_int),
                ("nontemporal", ctypes.c_int)]


class _CInfo(ctypes.Structure):
    _fields_ = [("n_slabs", ctypes.c_int), ("row_first", ctypes.c_int), ("row_count", ctypes.c_int),
                ("fluid_cells", ctypes.c_int), ("steps_done", ctypes.c_int),
                ("math_mode", ctypes.c_int), ("world_rank", ctypes.c_int),
                ("world_size", ctypes.c_int), ("steps_per_launch", ctypes.c_int),
                ("halo_mode", ctypes.c_int), ("band_rows", ctypes.c_int), ("lane_cells", ctypes.c_int),
                ("nontemporal", ctypes.c_int), ("graph_steps", ctypes.c_int),
                ("resident_steps", ctypes.c_int), ("resident_min_steps", ctypes.c_int),
                ("resident_rows", ctypes.c_int), ("resident_group", ctypes.c_int), ("resident_one_xcd", ctypes.c_int),
                ("band_groups", ctypes.c_int)]


class _CBatchInfo(ctypes.Structure):
    _fields_ = [("members", ctypes.c_int), ("members_per_launch", ctypes.c_int), ("launches_per_chunk", ctypes.c_int),
                ("resident_steps", ctypes.c_int), ("resident_min_steps", ctypes.c_int), ("steps_done", ctypes.c_int)]


class _CSteadyResult(ctypes.Structure):
    _fields_ = [("steps_run", ctypes.c_int), ("steady", ctypes.c_int), ("steady_step", ctypes.c_int),
                ("checks", ctypes.c_int), ("last_rel", ctypes.c_double), ("last_mean", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {"steps_run": self.steps_run, "steady": bool(self.steady), "steady_step": self.steady_step,
                "checks": self.checks, "last_rel": self.last_rel, "last_mean": self.last_mean}


class _CResidualRow(ctypes.Structure):      # lbm_residual_row, 40 bytes (RESIDUAL_DTYPE)
    _fields_ = [("sum_du_sq", ctypes.c_double), ("sum_u_sq", ctypes.c_double), ("nonfinite", ctypes.c_longlong),
                ("max_du", ctypes.c_float), ("max_x", ctypes.c_int), ("max_y", ctypes.c_int), ("span", ctypes.c_int)]


class _CResidualSteadyResult(ctypes.Structure):      # lbm_residual_steady_result, 72 bytes
    _fields_ = [("steps_run", ctypes.c_int), ("steady", ctypes.c_int), ("steady_step", ctypes.c_int),
                ("checks", ctypes.c_int), ("diverged", ctypes.c_int), ("reserved", ctypes.c_int),
                ("last_rel", ctypes.c_double), ("last", _CResidualRow)]

    def as_dict(self) -> dict:
        last = np.frombuffer(bytes(self.last), dtype=RESIDUAL_DTYPE)[0]
        return {"steps_run": self.steps_run, "steady": bool(self.steady), "steady_step": self.steady_step,
                "checks": self.checks, "diverged": bool(self.diverged), "last_rel": self.last_rel, "last": last}


class _CRcclStatus(ctypes.Structure):
    _fields_ = [("loaded", ctypes.c_int), ("version", ctypes.c_int), ("n_comms", ctypes.c_int),
                ("nranks", ctypes.c_int), ("rank", ctypes.c_int), ("library", ctypes.c_char * 512)]


class _CWindow(ctypes.Structure):
    _fields_ = [("x0", ctypes.c_int), ("y0", ctypes.c_int), ("nx", ctypes.c_int), ("ny", ctypes.c_int)]


class _CHaloOp(ctypes.Structure):
    _fields_ = [("is_send", ctypes.c_int), ("peer", ctypes.c_int), ("row_first", ctypes.c_int),
                ("row_count", ctypes.c_int)]


_EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_CHaloOp),
                                ctypes.POINTER(ctypes.POINTER(ctypes.c_float)), ctypes.c_size_t)
_ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int)


class _CHostComm(ctypes.Structure):
    _fields_ = [("exchange", _EXCHANGE_FN), ("allreduce_sum", _ALLREDUCE_FN), ("user", ctypes.c_void_p)]


@dataclass
class Params:
    """The reference's t_param (SerialCode/d2q9-bgk.c:66-75)."""
    nx: int
    ny: int
    max_iters: int
    reynolds_dim: int
    density: float
    accel: float
    omega: float

    def _c(self) -> _CParams:
        return _CParams(self.nx, self.ny, self.max_iters, self.reynolds_dim,
                        self.density, self.accel, self.omega)


@dataclass
class ParamsDouble:
    """The reference's t_param with its three floats read as doubles (lbm_params_double): Python floats, unrounded."""
    nx: int
    ny: int
    max_iters: int
    reynolds_dim: int
    density: float
    accel: float
    omega: float

    def _c(self) -> _CParamsDouble:
        return _CParamsDouble(self.nx, self.ny, self.max_iters, self.reynolds_dim,
                              self.density, self.accel, self.omega)


# ------------------------------------------------------------------------------------------------
# building and loading the shared library
# ------------------------------------------------------------------------------------------------
def build(force: bool = False) -> None:
    """Compile liblbm_hip.so (gfx950) and the d2q9-bgk host program in-tree with make."""
    cmd = ["make", "-C", _HERE] + (["-B"] if force else [])
    out = subprocess.run(cmd, capture_output=True, text=True)
    if out.returncode != 0:
        raise LbmError("building liblbm_hip.so failed:\n" + out.stdout + out.stderr)


_lib = None


def load_library() -> ctypes.CDLL:
    """dlopen liblbm_hip.so and declare the C-ABI prototypes.  Fails loudly if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LbmError(f"{LIB_PATH} not built: run `make -C {_HERE}` (no fallback path exists)")
    lib = ctypes.CDLL(LIB_PATH)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    PF, PI = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    lib.lbm_set_error_mode.argtypes = [I]; lib.lbm_set_error_mode.restype = None
    lib.lbm_last_error.argtypes = []; lib.lbm_last_error.restype = ctypes.c_char_p
    lib.lbm_version.argtypes = []; lib.lbm_version.restype = ctypes.c_char_p
    lib.lbm_device_count.argtypes = []; lib.lbm_device_count.restype = I
    lib.lbm_partition_rows.argtypes = [I, I, I, PI, PI]; lib.lbm_partition_rows.restype = I
    lib.lbm_halo_plan.argtypes = [I, I, I, I, ctypes.POINTER(_CHaloOp)]; lib.lbm_halo_plan.restype = I
    lib.lbm_plan_halo_depth.argtypes = [ctypes.POINTER(_CParams), I, I]; lib.lbm_plan_halo_depth.restype = I
    lib.lbm_create.argtypes = [ctypes.POINTER(_CParams), P, P, I, I]; lib.lbm_create.restype = P
    lib.lbm_rccl_unique_id.argtypes = [P]; lib.lbm_rccl_unique_id.restype = I
    lib.lbm_rccl_info.argtypes = [P, ctypes.POINTER(_CRcclStatus)]; lib.lbm_rccl_info.restype = I
    lib.lbm_create_rank.argtypes = [ctypes.POINTER(_CParams), P, P, I, I, P, I, I]
    lib.lbm_create_rank.restype = P
    lib.lbm_create_rank_rows.argtypes = [ctypes.POINTER(_CParams), P, P, I, I, P, I, I]
    lib.lbm_create_rank_rows.restype = P
    lib.lbm_create_tiled.argtypes = [ctypes.POINTER(_CParams), P, I, I, P, I, I]; lib.lbm_create_tiled.restype = P
    lib.lbm_create_rank_tiled.argtypes = [ctypes.POINTER(_CParams), P, I, I, I, I, P, I, I]
    lib.lbm_create_rank_tiled.restype = P
    lib.lbm_create_rank_hosted.argtypes = [ctypes.POINTER(_CParams), P, P, I, I, ctypes.POINTER(_CHostComm), I, I]
    lib.lbm_create_rank_hosted.restype = P
    lib.lbm_create_rank_hosted_rows.argtypes = [ctypes.POINTER(_CParams), P, P, I, I, ctypes.POINTER(_CHostComm), I, I]
    lib.lbm_create_rank_hosted_rows.restype = P
    lib.lbm_create_rank_hosted_tiled.argtypes = [ctypes.POINTER(_CParams), P, I, I, I, I, ctypes.POINTER(_CHostComm), I, I]
    lib.lbm_create_rank_hosted_tiled.restype = P
    lib.lbm_destroy.argtypes = [P]; lib.lbm_destroy.restype = None
    lib.lbm_get_info.argtypes = [P, ctypes.POINTER(_CInfo)]; lib.lbm_get_info.restype = I
    lib.lbm_set_halo_mode.argtypes = [P, I]; lib.lbm_set_halo_mode.restype = I
    lib.lbm_read_halo_log.argtypes = [P, ctypes.c_void_p, I]; lib.lbm_read_halo_log.restype = I
    lib.lbm_run.argtypes = [P, I]; lib.lbm_run.restype = I
    lib.lbm_sync.argtypes = [P]; lib.lbm_sync.restype = I
    lib.lbm_run_timed.argtypes = [P, I, PF]; lib.lbm_run_timed.restype = I
    lib.lbm_read_av_vels.argtypes = [P, P, I]; lib.lbm_read_av_vels.restype = I
    lib.lbm_read_cells.argtypes = [P, P]; lib.lbm_read_cells.restype = I
    lib.lbm_read_final_state.argtypes = [P, P, P, P, P]; lib.lbm_read_final_state.restype = I
    lib.lbm_av_velocity.argtypes = [P, PF]; lib.lbm_av_velocity.restype = I
    lib.lbm_total_density.argtypes = [P, ctypes.POINTER(ctypes.c_double)]
    lib.lbm_total_density.restype = I
    lib.lbm_calc_reynolds.argtypes = [P, PF]; lib.lbm_calc_reynolds.restype = I
    lib.lbm_set_frames.argtypes = [P, I, I]; lib.lbm_set_frames.restype = I
    lib.lbm_read_frames.argtypes = [P, I, P, P, PI]; lib.lbm_read_frames.restype = I
    lib.lbm_set_probes.argtypes = [P, I, P, I, I]; lib.lbm_set_probes.restype = I
    lib.lbm_read_probes.argtypes = [P, I, P, P, PI]; lib.lbm_read_probes.restype = I
    lib.lbm_set_mean.argtypes = [P, I]; lib.lbm_set_mean.restype = I
    lib.lbm_read_mean.argtypes = [P, P, P, P, P, ctypes.POINTER(ctypes.c_longlong)]; lib.lbm_read_mean.restype = I
    lib.lbm_set_mean_order.argtypes = [P, I, I]; lib.lbm_set_mean_order.restype = I
    lib.lbm_read_mean2.argtypes = [P, P, P, P, P, ctypes.POINTER(ctypes.c_longlong)]; lib.lbm_read_mean2.restype = I
    lib.lbm_set_field_frames.argtypes = [P, I, I, I, ctypes.POINTER(_CWindow)]; lib.lbm_set_field_frames.restype = I
    lib.lbm_read_field_frames.argtypes = [P, I, P, P, PI]; lib.lbm_read_field_frames.restype = I
    lib.lbm_set_forces.argtypes = [P, I, P, I, I]; lib.lbm_set_forces.restype = I
    lib.lbm_read_forces.argtypes = [P, I, P, P, PI]; lib.lbm_read_forces.restype = I
    lib.lbm_forces_links.argtypes = [P, P]; lib.lbm_forces_links.restype = I
    lib.lbm_run_until.argtypes = [P, I, I, ctypes.c_double, I, ctypes.POINTER(_CSteadyResult)]
    lib.lbm_run_until.restype = I
    lib.lbm_batch_run_until.argtypes = [P, I, I, ctypes.c_double, I, ctypes.POINTER(_CSteadyResult), PI]
    lib.lbm_batch_run_until.restype = I
    lib.lbm_create_batch.argtypes = [I, ctypes.POINTER(_CParams), P, P, I]; lib.lbm_create_batch.restype = P
    lib.lbm_batch_member.argtypes = [P, I]; lib.lbm_batch_member.restype = P
    lib.lbm_batch_run.argtypes = [P, I]; lib.lbm_batch_run.restype = I
    lib.lbm_batch_sync.argtypes = [P]; lib.lbm_batch_sync.restype = I
    lib.lbm_batch_get_info.argtypes = [P, ctypes.POINTER(_CBatchInfo)]; lib.lbm_batch_get_info.restype = I
    lib.lbm_destroy_batch.argtypes = [P]; lib.lbm_destroy_batch.restype = None
    lib.lbm_batch_set_forces.argtypes = [P, I, P, I, I]; lib.lbm_batch_set_forces.restype = I
    lib.lbm_batch_read_forces.argtypes = [P, I, P, P, PI]; lib.lbm_batch_read_forces.restype = I
    lib.lbm_batch_forces_links.argtypes = [P, P]; lib.lbm_batch_forces_links.restype = I
    lib.lbm_set_stats.argtypes = [P, I, I]; lib.lbm_set_stats.restype = I
    lib.lbm_read_stats.argtypes = [P, I, P, P, PI]; lib.lbm_read_stats.restype = I
    lib.lbm_batch_set_stats.argtypes = [P, I, I]; lib.lbm_batch_set_stats.restype = I
    lib.lbm_batch_read_stats.argtypes = [P, I, P, P, PI]; lib.lbm_batch_read_stats.restype = I
    lib.lbm_set_profiles.argtypes = [P, I, I, I]; lib.lbm_set_profiles.restype = I
    lib.lbm_read_profiles.argtypes = [P, I, P, P, PI]; lib.lbm_read_profiles.restype = I
    lib.lbm_batch_set_profiles.argtypes = [P, I, I, I]; lib.lbm_batch_set_profiles.restype = I
    lib.lbm_batch_read_profiles.argtypes = [P, I, P, P, PI]; lib.lbm_batch_read_profiles.restype = I
    lib.lbm_read_coarse.argtypes = [P, I, I, P]; lib.lbm_read_coarse.restype = I
    lib.lbm_set_coarse_frames.argtypes = [P, I, I, I, I]; lib.lbm_set_coarse_frames.restype = I
    lib.lbm_read_coarse_frames.argtypes = [P, I, P, P, PI]; lib.lbm_read_coarse_frames.restype = I
    lib.lbm_batch_set_coarse_frames.argtypes = [P, I, I, I, I]; lib.lbm_batch_set_coarse_frames.restype = I
    lib.lbm_batch_read_coarse_frames.argtypes = [P, I, P, P, PI]; lib.lbm_batch_read_coarse_frames.restype = I
    lib.lbm_read_vorticity.argtypes = [P, P]; lib.lbm_read_vorticity.restype = I
    lib.lbm_set_enstrophy.argtypes = [P, I, I]; lib.lbm_set_enstrophy.restype = I
    lib.lbm_read_enstrophy.argtypes = [P, I, P, P, PI]; lib.lbm_read_enstrophy.restype = I
    lib.lbm_batch_set_enstrophy.argtypes = [P, I, I]; lib.lbm_batch_set_enstrophy.restype = I
    lib.lbm_batch_read_enstrophy.argtypes = [P, I, P, P, PI]; lib.lbm_batch_read_enstrophy.restype = I
    lib.lbm_read_stress.argtypes = [P, P, P, P]; lib.lbm_read_stress.restype = I
    lib.lbm_set_stress.argtypes = [P, I, I]; lib.lbm_set_stress.restype = I
    lib.lbm_read_stress_rows.argtypes = [P, I, P, P, PI]; lib.lbm_read_stress_rows.restype = I
    lib.lbm_batch_set_stress.argtypes = [P, I, I]; lib.lbm_batch_set_stress.restype = I
    lib.lbm_batch_read_stress_rows.argtypes = [P, I, P, P, PI]; lib.lbm_batch_read_stress_rows.restype = I
    lib.lbm_set_tracers.argtypes = [P, I, P, I, I]; lib.lbm_set_tracers.restype = I
    lib.lbm_read_tracers.argtypes = [P, I, P, P, PI]; lib.lbm_read_tracers.restype = I
    lib.lbm_tracers_now.argtypes = [P, P]; lib.lbm_tracers_now.restype = I
    lib.lbm_batch_set_tracers.argtypes = [P, I, P, I, I]; lib.lbm_batch_set_tracers.restype = I
    lib.lbm_batch_read_tracers.argtypes = [P, I, P, P, PI]; lib.lbm_batch_read_tracers.restype = I
    lib.lbm_batch_tracers_now.argtypes = [P, P]; lib.lbm_batch_tracers_now.restype = I
    lib.lbm_read_psi.argtypes = [P, P]; lib.lbm_read_psi.restype = I
    lib.lbm_set_psi.argtypes = [P, I, I]; lib.lbm_set_psi.restype = I
    lib.lbm_read_psi_rows.argtypes = [P, I, P, P, PI]; lib.lbm_read_psi_rows.restype = I
    lib.lbm_batch_set_psi.argtypes = [P, I, I]; lib.lbm_batch_set_psi.restype = I
    lib.lbm_batch_read_psi_rows.argtypes = [P, I, P, P, PI]; lib.lbm_batch_read_psi_rows.restype = I
    lib.lbm_set_residual.argtypes = [P, I, I]; lib.lbm_set_residual.restype = I
    lib.lbm_read_residual.argtypes = [P, I, P, P, PI]; lib.lbm_read_residual.restype = I
    lib.lbm_batch_set_residual.argtypes = [P, I, I]; lib.lbm_batch_set_residual.restype = I
    lib.lbm_batch_read_residual.argtypes = [P, I, P, P, PI]; lib.lbm_batch_read_residual.restype = I
    lib.lbm_run_until_residual.argtypes = [P, I, I, ctypes.c_double, I, ctypes.POINTER(_CResidualSteadyResult), P, I]
    lib.lbm_run_until_residual.restype = I
    lib.lbm_batch_run_until_residual.argtypes = [P, I, I, ctypes.c_double, I, ctypes.POINTER(_CResidualSteadyResult), PI, P, I]
    lib.lbm_batch_run_until_residual.restype = I
    PD = ctypes.POINTER(ctypes.c_double)
    lib.lbm_double_create.argtypes = [ctypes.POINTER(_CParamsDouble), P, P]; lib.lbm_double_create.restype = P
    lib.lbm_double_destroy.argtypes = [P]; lib.lbm_double_destroy.restype = None
    lib.lbm_double_get_info.argtypes = [P, ctypes.POINTER(_CDoubleInfo)]; lib.lbm_double_get_info.restype = I
    lib.lbm_double_run.argtypes = [P, I]; lib.lbm_double_run.restype = I
    lib.lbm_double_run_timed.argtypes = [P, I, PF]; lib.lbm_double_run_timed.restype = I
    lib.lbm_double_sync.argtypes = [P]; lib.lbm_double_sync.restype = I
    lib.lbm_double_read_av_vels.argtypes = [P, P, I]; lib.lbm_double_read_av_vels.restype = I
    lib.lbm_double_read_cells.argtypes = [P, P]; lib.lbm_double_read_cells.restype = I
    lib.lbm_double_read_final_state.argtypes = [P, P, P, P, P]; lib.lbm_double_read_final_state.restype = I
    lib.lbm_double_av_velocity.argtypes = [P, PD]; lib.lbm_double_av_velocity.restype = I
    lib.lbm_double_total_density.argtypes = [P, PD]; lib.lbm_double_total_density.restype = I
    lib.lbm_double_calc_reynolds.argtypes = [P, PD]; lib.lbm_double_calc_reynolds.restype = I
    # a Python host wants exceptions, not exit(): switch from the reference's die() behaviour
    lib.lbm_set_error_mode(1)
    _lib = lib
    return lib


def _check(lib, rc) -> None:
    if rc != 0:
        raise LbmError(lib.lbm_last_error().decode())


def device_count() -> int:
    return int(load_library().lbm_device_count())


def partition_rows(ny: int, parts: int, index: int) -> tuple[int, int]:
    """Rows [first, first+count) owned by part `index` of `parts` (lbm_partition_rows)."""
    lib = load_library()
    first, count = ctypes.c_int(), ctypes.c_int()
    _check(lib, lib.lbm_partition_rows(ny, parts, index, ctypes.byref(first), ctypes.byref(count)))
    return first.value, count.value


def halo_plan(rows: int, parts: int, index: int, depth: int) -> list[dict]:
    """The four halo messages of one pass in the engine's posting order (lbm_halo_plan)."""
    lib = load_library()
    ops = (_CHaloOp * 4)()
    _check(lib, lib.lbm_halo_plan(rows, parts, index, depth, ops))
    return [{"is_send": bool(o.is_send), "peer": o.peer, "row_first": o.row_first, "row_count": o.row_count}
            for o in ops]


def plan_halo_depth(params: "Params", parts: int, math: str | int = "exact") -> int:
    """Halo depth = timesteps per pass the engine uses for `parts` row slabs (lbm_plan_halo_depth)."""
    lib = load_library()
    cp = params._c()
    d = lib.lbm_plan_halo_depth(ctypes.byref(cp), parts, _MATH[math])
    if d <= 0:
        raise LbmError(lib.lbm_last_error().decode())
    return int(d)


def _rccl_status(lib, handle) -> dict:
    st = _CRcclStatus()
    _check(lib, lib.lbm_rccl_info(handle, ctypes.byref(st)))
    v = st.version
    return {"loaded": bool(st.loaded), "version": v,
            "version_string": f"{v // 10000}.{v // 100 % 100}.{v % 100}" if v else None,
            "n_comms": st.n_comms, "nranks": st.nranks, "rank": st.rank,
            "library": st.library.decode() or None}


def rccl_info() -> dict:
    """Bind RCCL as the first multi-GPU create would and report which library and version (lbm_rccl_info(NULL))."""
    return _rccl_status(load_library(), None)


def rccl_unique_id() -> bytes:
    lib = load_library()
    buf = ctypes.create_string_buffer(RCCL_ID_BYTES)
    _check(lib, lib.lbm_rccl_unique_id(buf))
    return buf.raw


# ------------------------------------------------------------------------------------------------
# the engine handle
# ------------------------------------------------------------------------------------------------
class Engine:
    """One lattice on one or more GPUs.  Mirrors the reference's main()-level use of the hot path:
    create (initialise), run (the timestep/av_velocity loop), read results, close (finalise)."""

    def __init__(self, params: Params, obstacles: np.ndarray, cells: np.ndarray | None = None,
                 n_gpus: int = 1, math: str | int = "exact", *, rank: int | None = None,
                 world_size: int | None = None, unique_id: bytes | None = None, device: int = 0,
                 tiled: bool = False, local_rows: bool = False, host_comm=None):
        """obstacles: the global (ny, nx) map; with tiled=True a small (tile_ny, tile_nx) map repeated
        periodically over the grid (lbm_create_tiled / lbm_create_rank_tiled: the mask is expanded on the
        device); with local_rows=True (rank form only) this rank's rows preceded and followed by
        MASK_HALO_ROWS periodic neighbour rows, and `cells` this rank's rows only (lbm_create_rank_rows)."""
        self.lib = load_library()
        self.params = params
        if params.nx < 1 or params.ny < 2 or params.max_iters < 0:
            raise LbmError("lbm_create: invalid parameters")
        obstacles = np.ascontiguousarray(obstacles, dtype=np.int32)
        cell_rows = params.ny
        if tiled:
            if obstacles.ndim != 2:
                raise LbmError("lbm_create_tiled: the tile must be a 2-D map")
        elif local_rows:
            if rank is None:
                raise LbmError("local_rows needs the rank form")
            _, cell_rows = partition_rows(params.ny, world_size, rank)
            if obstacles.size != params.nx * (cell_rows + 2 * MASK_HALO_ROWS):
                raise LbmError("lbm_create_rank_rows: obstacle rows do not match (row_count + 2*MASK_HALO_ROWS)*nx")
        else:
            if obstacles.size != params.nx * params.ny:
                raise LbmError("lbm_create: obstacle map does not match nx*ny")
            obstacles = obstacles.reshape(params.ny, params.nx)
        self._obstacles = obstacles
        cptr = None
        if cells is not None:
            cells = np.ascontiguousarray(cells, dtype=np.float32)
            if cells.size != params.nx * cell_rows * 9:
                raise LbmError("lbm_create: cells do not match nx*ny*9")
            cells = cells.reshape(cell_rows, params.nx, 9)
            cptr = cells.ctypes.data
        cp = params._c()
        idbuf = ctypes.create_string_buffer(unique_id, RCCL_ID_BYTES) if unique_id else None
        if host_comm is not None:
            if rank is None:
                raise LbmError("host_comm needs the rank form")
            self._host_comm = self._wrap_host_comm(*host_comm)
            if tiled:
                if cells is not None:
                    raise LbmError("lbm_create_rank_hosted_tiled starts from the uniform equilibrium")
                h = self.lib.lbm_create_rank_hosted_tiled(ctypes.byref(cp), obstacles.ctypes.data, obstacles.shape[1],
                                                          obstacles.shape[0], rank, world_size,
                                                          ctypes.byref(self._host_comm), device, _MATH[math])
            elif local_rows:
                h = self.lib.lbm_create_rank_hosted_rows(ctypes.byref(cp), obstacles.ctypes.data, cptr, rank, world_size,
                                                         ctypes.byref(self._host_comm), device, _MATH[math])
            else:
                h = self.lib.lbm_create_rank_hosted(ctypes.byref(cp), obstacles.ctypes.data, cptr, rank, world_size,
                                                    ctypes.byref(self._host_comm), device, _MATH[math])
        elif rank is None:
            if tiled:
                h = self.lib.lbm_create_tiled(ctypes.byref(cp), obstacles.ctypes.data, obstacles.shape[1],
                                              obstacles.shape[0], cptr, n_gpus, _MATH[math])
            else:
                h = self.lib.lbm_create(ctypes.byref(cp), obstacles.ctypes.data, cptr, n_gpus, _MATH[math])
        elif tiled:
            if cells is not None:
                raise LbmError("lbm_create_rank_tiled starts from the uniform equilibrium")
            h = self.lib.lbm_create_rank_tiled(ctypes.byref(cp), obstacles.ctypes.data, obstacles.shape[1],
                                               obstacles.shape[0], rank, world_size, idbuf, device, _MATH[math])
        elif local_rows:
            h = self.lib.lbm_create_rank_rows(ctypes.byref(cp), obstacles.ctypes.data, cptr, rank,
                                              world_size, idbuf, device, _MATH[math])
        else:
            h = self.lib.lbm_create_rank(ctypes.byref(cp), obstacles.ctypes.data, cptr, rank,
                                         world_size, idbuf, device, _MATH[math])
        if not h:
            raise LbmError(self.lib.lbm_last_error().decode())
        self.handle = ctypes.c_void_p(h)

    @staticmethod
    def _wrap_host_comm(exchange, allreduce_sum):
        def c_exchange(_user, n_ops, ops, buffers, floats):
            try:
                plan = [{"is_send": bool(ops[i].is_send), "peer": ops[i].peer, "row_first": ops[i].row_first,
                         "row_count": ops[i].row_count} for i in range(n_ops)]
                views = [np.ctypeslib.as_array(buffers[i], shape=(floats,)) for i in range(n_ops)]
                exchange(plan, views)
                return 0
            except Exception:                   # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1

        def c_allreduce(_user, values, n):
            try:
                allreduce_sum(np.ctypeslib.as_array(values, shape=(n,)))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1

        comm = _CHostComm(_EXCHANGE_FN(c_exchange), _ALLREDUCE_FN(c_allreduce), None)
        comm._keep = (c_exchange, c_allreduce)   # the callbacks must outlive the context
        return comm

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.lbm_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        ci = _CInfo()
        _check(self.lib, self.lib.lbm_get_info(self.handle, ctypes.byref(ci)))
        return {name: getattr(ci, name) for name, _ in _CInfo._fields_}

    def rccl_info(self) -> dict:
        """Which RCCL this context's communicators come from and what they say about the ring (lbm_rccl_info)."""
        return _rccl_status(self.lib, self.handle)

    def set_halo_mode(self, mode) -> None:
        """'sync' (halo rows of the same timestep, the MPI_Waitall pattern), 'stale' (one pass
        old: reproducible analogue of the reference's MPI_Testall variant) or 'freshest' (the rows of this
        step where they have arrived by the time the interior rows are done, else the rows of the step before)."""
        if mode not in _HALO:
            raise LbmError(f"unknown halo mode {mode!r}")
        _check(self.lib, self.lib.lbm_set_halo_mode(self.handle, _HALO[mode]))

    def halo_log(self, n_steps: int) -> np.ndarray:
        """uint8 [n_steps, n_slabs]: what each look of the 'freshest' mode found (bit 0 south, bit 1 north halo row
        fresh); lbm_read_halo_log."""
        out = np.zeros((int(n_steps), self.info()["n_slabs"]), dtype=np.uint8)
        _check(self.lib, self.lib.lbm_read_halo_log(self.handle, out.ctypes.data, int(n_steps)))
        return out

    # -- hot path ----------------------------------------------------------------------------
    def run(self, n_steps: int) -> None:
        _check(self.lib, self.lib.lbm_run(self.handle, int(n_steps)))

    def run_timed(self, n_steps: int) -> float:
        """Advance n_steps; returns the average device milliseconds per step (HIP events on the
        compute stream)."""
        ms = ctypes.c_float()
        _check(self.lib, self.lib.lbm_run_timed(self.handle, int(n_steps), ctypes.byref(ms)))
        return float(ms.value)

    def sync(self) -> None:
        _check(self.lib, self.lib.lbm_sync(self.handle))

    def run_until(self, max_steps: int, check_every: int = 1024, tol: float = 1e-6, patience: int = 2) -> dict:
        """Advance until the average velocity has stopped changing, or by max_steps (lbm_run_until): segments of
        check_every steps; steady when the relative change of the segment means stayed <= tol for `patience` checks in
        a row.  Returns steps_run, steady, steady_step (-1: never), checks, last_rel, last_mean."""
        args = _steady_args(max_steps, check_every, tol, patience)
        res = _CSteadyResult()
        _check(self.lib, self.lib.lbm_run_until(self.handle, *args, ctypes.byref(res)))
        return res.as_dict()

    # -- animation frames (lbm_set_frames / lbm_read_frames) ---------------------------------
    def run_until_residual(self, max_steps: int, check_every: int = 1024, tol: float = 1e-4, patience: int = 2, history=None) -> dict:
        """Advance until the velocity field has stopped changing, or by max_steps (lbm_run_until_residual): after every
        check_every steps the relative L2 residual sqrt(sum_du_sq / sum_u_sq) against the field of the check before (the
        first: of the start of the call) is compared with tol on the device; steady after `patience` consecutive checks
        met; a check that finds a non-finite fluid cell ends the call (diverged).  In fp32 the residual floors near 1e-5,
        and it scales with check_every.  history: None keeps the rows of all checks, an int that many.  Returns
        {steps_run, steady, steady_step, checks, diverged, last_rel, last (a RESIDUAL_DTYPE record),
        history: (steps int32[n], RESIDUAL_DTYPE[n])}, steps counted from the start of the call."""
        args = _steady_args(max_steps, check_every, tol, patience)
        capacity = _until_history_arg(history, args[0], args[1])
        res = _CResidualSteadyResult()
        rows = np.zeros(capacity, dtype=RESIDUAL_DTYPE)
        _check(self.lib, self.lib.lbm_run_until_residual(self.handle, *args, ctypes.byref(res), rows.ctypes.data, capacity))
        out = res.as_dict()
        n = min(res.checks, capacity)
        out["history"] = (np.arange(1, n + 1, dtype=np.int32) * np.int32(args[1]), rows[:n])
        return out

    def set_frames(self, every: int, capacity: int = 0) -> None:
        """Record |u| of the owned rows after every global timestep tt with tt % every == 0 (the reference's
        write_animation_data hook, SerialCode/d2q9-bgk.c:171-173) into a device buffer of `capacity` frames.
        every == 0 disarms; re-arming discards unread frames."""
        every, capacity = _frame_args(every, capacity)
        _check(self.lib, self.lib.lbm_set_frames(self.handle, every, capacity))

    def frames(self, max_frames: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_frames (default: all) waiting frames, oldest first:
        (steps int32[n], frames float32[n, row_count, nx])."""
        if max_frames is not None and (isinstance(max_frames, bool) or not isinstance(max_frames, (int, np.integer))
                                       or max_frames < 0):
            raise LbmError(f"frames: max_frames must be a non-negative integer or None (got {max_frames!r})")
        n = ctypes.c_int()
        _check(self.lib, self.lib.lbm_read_frames(self.handle, 0, None, None, ctypes.byref(n)))  # frames waiting
        max_frames = n.value if max_frames is None else min(int(max_frames), n.value)
        rows = self.info()["row_count"]
        frames = np.empty((int(max_frames), rows, self.params.nx), dtype=np.float32)
        steps = np.empty(int(max_frames), dtype=np.int32)
        _check(self.lib, self.lib.lbm_read_frames(self.handle, int(max_frames), frames.ctypes.data,
                                                  steps.ctypes.data, ctypes.byref(n)))
        return steps[:n.value].copy(), frames[:n.value].copy()

    # -- point probes (lbm_set_probes / lbm_read_probes) ---------------------------------------
    def set_probes(self, cells, every: int = 1, capacity: int = 4096) -> None:
        """Record u_x, u_y, |u| and pressure at `cells` -- a sequence of global (x, y), at most LBM_MAX_PROBES -- after
        every global timestep tt with tt % every == 0, bit for bit what final_state() gives there after tt + 1 steps,
        into a device ring of `capacity` sample rows.  No cells or every == 0 disarms; re-arming discards unread rows."""
        flat, every, capacity = _probe_args(cells, every, capacity)
        arr = (_CProbe * max(1, len(flat)))(*[_CProbe(x, y) for x, y in flat])
        _check(self.lib, self.lib.lbm_set_probes(self.handle, len(flat), arr, every, capacity))
        self._n_probes = len(flat) if every > 0 else 0

    def probes(self, max_samples: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_samples (default: all) waiting sample rows, oldest first:
        (steps int32[n], samples float32[n, n_probes, 4]), columns u_x, u_y, u, pressure."""
        if max_samples is not None and (isinstance(max_samples, bool) or not isinstance(max_samples, (int, np.integer))
                                        or max_samples < 0):
            raise LbmError(f"probes: max_samples must be a non-negative integer or None (got {max_samples!r})")
        n = ctypes.c_int()
        _check(self.lib, self.lib.lbm_read_probes(self.handle, 0, None, None, ctypes.byref(n)))  # rows waiting
        max_samples = n.value if max_samples is None else min(int(max_samples), n.value)
        n_probes = getattr(self, "_n_probes", 0)
        samples = np.empty((int(max_samples), n_probes, 4), dtype=np.float32)
        steps = np.empty(int(max_samples), dtype=np.int32)
        _check(self.lib, self.lib.lbm_read_probes(self.handle, int(max_samples), samples.ctypes.data,
                                                  steps.ctypes.data, ctypes.byref(n)))
        return steps[:n.value].copy(), samples[:n.value].copy()

    # -- mean flow fields (lbm_set_mean / lbm_read_mean) ----------------------------------------
    def set_mean(self, every: int) -> None:
        """Accumulate u_x, u_y, |u| and pressure of every owned cell after every global timestep tt with tt % every == 0,
        bit for bit what final_state() gives after tt + 1 steps, into float64 sums on the device.  every == 0 disarms;
        arming again zeroes the sums and the count."""
        _check(self.lib, self.lib.lbm_set_mean(self.handle, _mean_args(every)))

    def set_mean_order(self, every: int, order: int = 2) -> None:
        """set_mean with the order of the moments (lbm_set_mean_order): order 1 is set_mean(every); order 2 also
        accumulates the exact products u_x u_x, u_y u_y, u_x u_y and pressure pressure of the same samples into four
        more float64 planes (moment_sums, fluctuations).  The sums of set_mean are bit-identical at either order."""
        _check(self.lib, self.lib.lbm_set_mean_order(self.handle, _mean_args(every), _mean_order_arg(order)))

    def mean_sums(self) -> tuple[dict, int]:
        """The sums since arming and the number of samples: ({u_x, u_y, u, pressure: float64 (row_count, nx)}, n).
        Reading does not reset them."""
        rows = self.info()["row_count"]
        f = {k: np.zeros((rows, self.params.nx), dtype=np.float64) for k in ("u_x", "u_y", "u", "pressure")}
        n = ctypes.c_longlong()
        _check(self.lib, self.lib.lbm_read_mean(self.handle, f["u_x"].ctypes.data, f["u_y"].ctypes.data, f["u"].ctypes.data,
                                                f["pressure"].ctypes.data, ctypes.byref(n)))
        return f, int(n.value)

    def mean(self) -> dict:
        """The mean fields over the samples since arming: the sums divided by their number, float64, under the keys of
        final_state(), plus "samples"."""
        sums, n = self.mean_sums()
        if n == 0:
            raise LbmError("mean: no sample has been taken since the mean fields were armed")
        out = {k: v / float(n) for k, v in sums.items()}
        out["samples"] = n
        return out

    def moment_sums(self) -> tuple[dict, int]:
        """The sums of products since arming at order 2 and the number of samples: ({"u_x u_x", "u_y u_y", "u_x u_y",
        "pressure pressure": float64 (row_count, nx)}, n) (lbm_read_mean2).  Reading does not reset them.  Raises
        LbmError when the mean fields are not armed or armed at order 1."""
        rows = self.info()["row_count"]
        f = {k: np.zeros((rows, self.params.nx), dtype=np.float64) for k in MOMENT_FIELDS}
        n = ctypes.c_longlong()
        _check(self.lib, self.lib.lbm_read_mean2(self.handle, *(f[k].ctypes.data for k in MOMENT_FIELDS), ctypes.byref(n)))
        return f, int(n.value)

    def fluctuations(self) -> dict:
        """Variances, rms values and the Reynolds shear stress over the samples since arming at order 2 (host arithmetic
        on the float64 sums, see :func:`fluctuations_of`)."""
        sums, n = self.mean_sums()
        sums2, _ = self.moment_sums()
        return fluctuations_of(sums, sums2, n)

    # -- field frames (lbm_set_field_frames / lbm_read_field_frames) ------------------------------
    def set_field_frames(self, every: int, capacity: int = 0, fields=("u_x", "u_y", "u", "pressure"), window=None) -> None:
        """Record the chosen `fields` -- a non-empty subset of final_state()'s keys -- over `window` = (x0, y0, nx, ny) in
        global cells (None: the whole grid) after every global timestep tt with tt % every == 0, bit for bit what
        final_state() gives there after tt + 1 steps, into a device ring of `capacity` frames.  every == 0 disarms;
        re-arming discards unread frames."""
        every, capacity, mask, window = _field_frame_args(every, capacity, fields, window)
        win = _CWindow(*window) if window is not None else None
        _check(self.lib, self.lib.lbm_set_field_frames(self.handle, every, capacity, mask, ctypes.byref(win) if win else None))
        if every > 0:
            full = (0, 0, self.params.nx, self.params.ny)
            self._field_frames = ([k for k in FIELD_NAMES if mask & FIELD_BITS[k]], window if window is not None else full)
        else:
            self._field_frames = None

    def field_frames(self, max_frames: int | None = None) -> tuple[np.ndarray, dict]:
        """Drain up to max_frames (default: all) waiting field frames, oldest first:
        (steps int32[n], {name: float32[n, window ny, window nx]}) for the armed fields."""
        if max_frames is not None and (isinstance(max_frames, bool) or not isinstance(max_frames, (int, np.integer))
                                       or max_frames < 0):
            raise LbmError(f"field_frames: max_frames must be a non-negative integer or None (got {max_frames!r})")
        n = ctypes.c_int()
        _check(self.lib, self.lib.lbm_read_field_frames(self.handle, 0, None, None, ctypes.byref(n)))  # frames waiting
        max_frames = n.value if max_frames is None else min(int(max_frames), n.value)
        names, window = getattr(self, "_field_frames", None) or ([], (0, 0, 0, 0))
        out = np.empty((int(max_frames), len(names), window[3], window[2]), dtype=np.float32)
        steps = np.empty(int(max_frames), dtype=np.int32)
        if max_frames > 0:
            _check(self.lib, self.lib.lbm_read_field_frames(self.handle, int(max_frames), out.ctypes.data, steps.ctypes.data,
                                                            ctypes.byref(n)))
        return steps[:n.value].copy(), {k: out[:n.value, j].copy() for j, k in enumerate(names)}

    # -- obstacle forces (lbm_set_forces / lbm_read_forces / lbm_forces_links) ---------------------
    def set_forces(self, every: int, capacity: int = 4096, bodies=None, n_bodies: int | None = None) -> None:
        """Record the force of the fluid on the obstacles -- the momentum exchanged over the boundary links, summed
        exactly and rounded once -- after every global timestep tt with tt % every == 0, for the lattice after tt + 1
        steps, into a device ring of `capacity` rows.  `bodies`: None (all blocked cells are body 0) or an integer array
        of the grid's shape (ny, nx) with the body of every blocked cell in 0 .. n_bodies - 1 (entries on fluid cells are
        ignored); n_bodies defaults to the largest label + 1.  every == 0 disarms; re-arming discards unread rows."""
        every, capacity, n_bodies, labels = _forces_args(every, capacity, bodies, n_bodies, self.params.nx, self.params.ny)
        _check(self.lib, self.lib.lbm_set_forces(self.handle, n_bodies, labels.ctypes.data if labels is not None else None,
                                                 every, capacity))
        self._n_bodies = n_bodies if every > 0 else 0

    def forces(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[n], float64[n, n_bodies, 2]),
        columns F_x, F_y."""
        return _drain_rows(self.lib.lbm_read_forces, self.lib, self.handle, "forces", max_rows, (getattr(self, "_n_bodies", 0), 2),
                           np.float64, np.empty)

    def force_links(self) -> np.ndarray:
        """Boundary links of every body of the armed forces, int32[n_bodies] (lbm_forces_links)."""
        out = np.zeros(max(1, getattr(self, "_n_bodies", 0)), dtype=np.int32)
        _check(self.lib, self.lib.lbm_forces_links(self.handle, out.ctypes.data))
        return out[:getattr(self, "_n_bodies", 0)].copy()

    # -- lattice statistics (lbm_set_stats / lbm_read_stats) ---------------------------------------
    def set_stats(self, every: int, capacity: int = 4096) -> None:
        """Record one row of whole-lattice statistics -- mass, momentum and the sum of |u|^2 summed exactly and rounded
        once, the largest |u| and its cell, the cells that are not finite -- after every global timestep tt with
        tt % every == 0, for the lattice after tt + 1 steps, into a device ring of `capacity` rows.  every == 0 disarms;
        re-arming discards unread rows."""
        every, capacity = _stats_args(every, capacity)
        _check(self.lib, self.lib.lbm_set_stats(self.handle, every, capacity))

    def stats(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[n], STATS_DTYPE[n])."""
        return _drain_rows(self.lib.lbm_read_stats, self.lib, self.handle, "stats", max_rows, (), STATS_DTYPE, np.zeros)

    # -- vorticity and enstrophy (lbm_read_vorticity / lbm_set_enstrophy / lbm_read_enstrophy) -------
    def vorticity(self) -> np.ndarray:
        """The vorticity of the current lattice, float32 (row_count, nx): w = 0.5 * ((u_y(x+1) - u_y(x-1)) - (u_x(y+1) -
        u_x(y-1))) of final_state()'s velocities with both periodic wraps, blocked cells 0 (as neighbours too).  Needs
        nothing armed and changes nothing."""
        out = np.empty((self.info()["row_count"], self.params.nx), dtype=np.float32)
        _check(self.lib, self.lib.lbm_read_vorticity(self.handle, out.ctypes.data))
        return out

    def set_enstrophy(self, every: int, capacity: int = 4096) -> None:
        """Record one row of the vorticity's whole-lattice sums -- the enstrophy (sum of w^2) and the circulation (sum of
        w) over the finite fluid cells, summed exactly and rounded once, the largest |w| and its cell, the counts --
        after every global timestep tt with tt % every == 0, for the lattice after tt + 1 steps, into a device ring of
        `capacity` rows.  every == 0 disarms; re-arming discards unread rows."""
        every, capacity = _enstrophy_args(every, capacity)
        _check(self.lib, self.lib.lbm_set_enstrophy(self.handle, every, capacity))

    def enstrophy(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[n], ENSTROPHY_DTYPE[n])."""
        return _drain_rows(self.lib.lbm_read_enstrophy, self.lib, self.handle, "enstrophy", max_rows, (), ENSTROPHY_DTYPE, np.zeros)

    # -- stress and dissipation (lbm_read_stress / lbm_set_stress / lbm_read_stress_rows) ------------
    def stress(self) -> dict:
        """The kinematic non-equilibrium stress of the current (stored, post-collision) lattice: {"txx", "txy", "tyy"},
        float32 (row_count, nx) each, t_ab = Pi_ab / rho from the cell's second moment, blocked cells 0.  strain_rate()
        converts it.  Needs nothing armed and changes nothing."""
        shape = (self.info()["row_count"], self.params.nx)
        out = {name: np.empty(shape, dtype=np.float32) for name in ("txx", "txy", "tyy")}
        _check(self.lib, self.lib.lbm_read_stress(self.handle, out["txx"].ctypes.data, out["txy"].ctypes.data, out["tyy"].ctypes.data))
        return out

    def set_stress(self, every: int, capacity: int = 4096) -> None:
        """Record one row of the stress' whole-lattice sums -- sum_q (q = txx^2 + tyy^2 + 2 txy^2) and sum_txy over the
        finite fluid cells, summed exactly and rounded once, the largest q and its cell, the counts -- after every global
        timestep tt with tt % every == 0, for the lattice after tt + 1 steps, into a device ring of `capacity` rows.
        every == 0 disarms; re-arming discards unread rows.  dissipation() and shear_rate_max() convert the rows."""
        every, capacity = _every_capacity("set_stress", every, capacity, "row")
        _check(self.lib, self.lib.lbm_set_stress(self.handle, every, capacity))

    def stress_rows(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[n], STRESS_DTYPE[n])."""
        return _drain_rows(self.lib.lbm_read_stress_rows, self.lib, self.handle, "stress_rows", max_rows, (), STRESS_DTYPE, np.zeros)

    # -- tracer particles (lbm_set_tracers / lbm_read_tracers / lbm_tracers_now) ----------------------
    def set_tracers(self, xy, every: int, capacity: int = 0) -> None:
        """Advect the tracers `xy`, float64 (n, 2) positions (x, y) with 0 <= x < nx and 0 <= y < ny (a cell's centre is
        its index), through the velocity field on the device: after every global timestep tt with tt % every == 0 each
        advances once by the midpoint rule over the steps since the last sample, and the row of all positions goes into a
        device ring of `capacity` rows.  capacity == 0 (the default) keeps no rows: tracers() gives the positions.
        every == 0 or no tracers disarms; re-arming discards positions and rows.  tracer_seeds() makes a regular cloud."""
        xy, every, capacity = _tracer_args("set_tracers", xy, (), every, capacity)
        _check(self.lib, self.lib.lbm_set_tracers(self.handle, xy.shape[0], xy.ctypes.data, every, capacity))
        self._n_tracers = xy.shape[0] if every > 0 else 0

    def tracer_rows(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[rows], float64[rows, n, 2])."""
        return _drain_rows(self.lib.lbm_read_tracers, self.lib, self.handle, "tracer_rows", max_rows, (getattr(self, "_n_tracers", 0), 2),
                           np.float64, np.zeros)

    def tracers(self) -> np.ndarray:
        """The tracers' current positions, float64 (n, 2): those of the last sample.  Drains nothing."""
        out = np.empty((getattr(self, "_n_tracers", 0), 2), dtype=np.float64)
        _check(self.lib, self.lib.lbm_tracers_now(self.handle, out.ctypes.data))
        return out

    # -- stream function (lbm_read_psi / lbm_set_psi / lbm_read_psi_rows) ----------------------------
    def psi(self) -> np.ndarray:
        """The mass stream function of the current lattice, float64 (row_count, nx): psi[y, x] = the exact sum of j_x over
        the finite fluid cells (x, 0 .. y), rounded once (math.fsum's value); blocked and non-finite cells add 0.  Needs
        nothing armed and changes nothing."""
        out = np.empty((self.info()["row_count"], self.params.nx), dtype=np.float64)
        _check(self.lib, self.lib.lbm_read_psi(self.handle, out.ctypes.data))
        return out

    def set_psi(self, every: int, capacity: int = 4096) -> None:
        """Record one row of the stream function's extrema over the finite fluid cells -- psi_min and psi_max with their
        cells (the vortex centres), ties to the smallest y*nx+x, and the counts -- after every global timestep tt with
        tt % every == 0, for the lattice after tt + 1 steps, into a device ring of `capacity` rows.  every == 0 disarms;
        re-arming discards unread rows."""
        every, capacity = _psi_args(every, capacity)
        _check(self.lib, self.lib.lbm_set_psi(self.handle, every, capacity))

    def psi_rows(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[n], PSI_DTYPE[n])."""
        return _drain_rows(self.lib.lbm_read_psi_rows, self.lib, self.handle, "psi_rows", max_rows, (), PSI_DTYPE, np.zeros)

    # -- velocity residuals (lbm_set_residual / lbm_read_residual) ---------------------------------
    def set_residual(self, every: int, capacity: int = 4096) -> None:
        """Remember the velocity field of the current lattice (the baseline) and, after every global timestep tt with
        tt % every == 0, record one row for the lattice after tt + 1 steps: the exact sums of |u - u_remembered|^2 and of
        |u|^2 over the finite fluid cells, the largest |u - u_remembered| and its cell, the fluid cells that are not
        finite, and the steps the comparison spans; the sample then becomes the remembered field.  Rows wait in a device
        ring of `capacity` rows.  every == 0 disarms; re-arming takes a new baseline and discards unread rows."""
        every, capacity = _residual_args(every, capacity)
        _check(self.lib, self.lib.lbm_set_residual(self.handle, every, capacity))

    def residuals(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[n], RESIDUAL_DTYPE[n])."""
        return _drain_rows(self.lib.lbm_read_residual, self.lib, self.handle, "residuals", max_rows, (), RESIDUAL_DTYPE, np.zeros)

    # -- line profiles (lbm_set_profiles / lbm_read_profiles) ---------------------------------------
    def set_profiles(self, every: int, capacity: int = 16, axes=("rows", "columns")) -> None:
        """Record, after every global timestep tt with tt % every == 0, for the lattice after tt + 1 steps, one line of
        exact sums (rho, jx, jy, ux, uy over the line's finite fluid cells, each rounded once) and two counts per row
        ("rows": sums along x) and per column ("columns": sums along y), into a device ring of `capacity` records.
        `axes`: an int of LBM_PROFILE_* bits or a subset of ("rows", "columns").  every == 0 disarms; re-arming
        discards unread records."""
        every, capacity, axes = _profile_args(every, capacity, axes)
        _check(self.lib, self.lib.lbm_set_profiles(self.handle, every, capacity, axes))
        self._profile_axes = axes if every > 0 else 0

    def profiles(self, max_records: int | None = None) -> tuple[np.ndarray, dict]:
        """Drain up to max_records (default: all) waiting records, oldest first: (steps int32[n], {"rows":
        PROFILE_DTYPE[n, ny], "columns": PROFILE_DTYPE[n, nx]}), the selected keys only."""
        return _read_profiles(self.lib.lbm_read_profiles, self.lib, self.handle, max_records, getattr(self, "_profile_axes", 0), (),
                              self.params.nx, self.params.ny)

    # -- coarse frames (lbm_read_coarse / lbm_set_coarse_frames / lbm_read_coarse_frames) -----------
    def coarse(self, box) -> np.ndarray:
        """The coarse frame of the current lattice, PROFILE_DTYPE (cy, cx): per box of `box` = (bx, by) cells (an int b:
        (b, b)) what a line of set_profiles holds per line, over the box's cells; cx = ceil(nx / bx), cy = ceil(ny / by),
        the last box of an axis may be ragged.  Needs nothing armed and changes nothing."""
        _, _, bx, by = _coarse_args(0, 0, box, "coarse")
        out = np.zeros(_coarse_shape(self.params.nx, self.params.ny, bx, by), dtype=PROFILE_DTYPE)
        _check(self.lib, self.lib.lbm_read_coarse(self.handle, bx, by, out.ctypes.data))
        return out

    def set_coarse_frames(self, every: int, capacity: int = 16, box=(16, 16)) -> None:
        """Record, after every global timestep tt with tt % every == 0, for the lattice after tt + 1 steps, one coarse
        frame (Engine.coarse of `box`) into a device ring of `capacity` frames; a box leaves the device as its rounded
        48-byte line.  every == 0 disarms; re-arming discards unread frames."""
        every, capacity, bx, by = _coarse_args(every, capacity, box)
        _check(self.lib, self.lib.lbm_set_coarse_frames(self.handle, every, capacity, bx, by))
        self._coarse_box = (bx, by) if every > 0 else None

    def coarse_frames(self, max_frames: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_frames (default: all) waiting frames, oldest first: (steps int32[n], PROFILE_DTYPE[n, cy, cx])."""
        return _read_coarse_frames(self.lib.lbm_read_coarse_frames, self.lib, self.handle, max_frames, getattr(self, "_coarse_box", None), (),
                                   self.params.nx, self.params.ny)

    # -- results -----------------------------------------------------------------------------
    def av_vels(self, n: int | None = None) -> np.ndarray:
        n = self.info()["steps_done"] if n is None else n
        out = np.empty(n, dtype=np.float32)
        _check(self.lib, self.lib.lbm_read_av_vels(self.handle, out.ctypes.data, n))
        return out

    def cells(self) -> np.ndarray:
        """Owned rows of the lattice in the reference's AoS layout: (rows, nx, 9) float32."""
        rows = self.info()["row_count"]
        out = np.empty((rows, self.params.nx, 9), dtype=np.float32)
        _check(self.lib, self.lib.lbm_read_cells(self.handle, out.ctypes.data))
        return out

    def final_state(self) -> dict:
        rows = self.info()["row_count"]
        shape = (rows, self.params.nx)
        f = {k: np.empty(shape, dtype=np.float32) for k in ("u_x", "u_y", "u", "pressure")}
        _check(self.lib, self.lib.lbm_read_final_state(
            self.handle, f["u_x"].ctypes.data, f["u_y"].ctypes.data, f["u"].ctypes.data,
            f["pressure"].ctypes.data))
        return f

    def av_velocity(self) -> float:
        v = ctypes.c_float()
        _check(self.lib, self.lib.lbm_av_velocity(self.handle, ctypes.byref(v)))
        return float(v.value)

    def total_density(self) -> float:
        v = ctypes.c_double()
        _check(self.lib, self.lib.lbm_total_density(self.handle, ctypes.byref(v)))
        return float(v.value)

    def reynolds(self) -> float:
        v = ctypes.c_float()
        _check(self.lib, self.lib.lbm_calc_reynolds(self.handle, ctypes.byref(v)))
        return float(v.value)


# ------------------------------------------------------------------------------------------------
# double precision: the reference's algorithm in IEEE double, what its golden results were computed in
# ------------------------------------------------------------------------------------------------
class DoubleEngine:
    """One lattice advanced in double precision (lbm_double_*): the reference's loop with every float read as double,
    bit for bit.  One periodic slab on one device, one timestep per launch; no slabs, ranks, recorders, batches or
    run_until.  `cells`: (ny, nx, 9) float64 or None (uniform equilibrium)."""

    def __init__(self, params: ParamsDouble, obstacles: np.ndarray, cells: np.ndarray | None = None):
        self.lib = load_library()
        self.params = params
        self.handle = None
        obstacles = np.asarray(obstacles)
        if obstacles.size != params.nx * params.ny:
            raise LbmError(f"obstacles has {obstacles.size} cells, the grid {params.nx * params.ny}")
        ob = np.ascontiguousarray(obstacles, dtype=np.int32)
        cp = None
        if cells is not None:
            cells = np.ascontiguousarray(cells, dtype=np.float64)
            if cells.size != params.nx * params.ny * 9:
                raise LbmError(f"cells has {cells.size} values, the grid {params.nx * params.ny * 9}")
            cp = cells.ctypes.data
        cpar = params._c()
        self.handle = self.lib.lbm_double_create(ctypes.byref(cpar), ob.ctypes.data, cp)
        if not self.handle:
            raise LbmError(self.lib.lbm_last_error().decode())

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.lbm_double_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        ci = _CDoubleInfo()
        _check(self.lib, self.lib.lbm_double_get_info(self.handle, ctypes.byref(ci)))
        return {name: getattr(ci, name) for name, _ in _CDoubleInfo._fields_}

    def run(self, n_steps: int) -> None:
        _check(self.lib, self.lib.lbm_double_run(self.handle, int(n_steps)))

    def run_timed(self, n_steps: int) -> float:
        """Advance n_steps; returns the average device milliseconds per step (HIP events on the stream)."""
        ms = ctypes.c_float()
        _check(self.lib, self.lib.lbm_double_run_timed(self.handle, int(n_steps), ctypes.byref(ms)))
        return float(ms.value)

    def sync(self) -> None:
        _check(self.lib, self.lib.lbm_double_sync(self.handle))

    def av_vels(self, n: int | None = None) -> np.ndarray:
        n = self.info()["steps_done"] if n is None else n
        out = np.empty(n, dtype=np.float64)
        _check(self.lib, self.lib.lbm_double_read_av_vels(self.handle, out.ctypes.data, n))
        return out

    def cells(self) -> np.ndarray:
        """The lattice in the reference's AoS layout: (ny, nx, 9) float64."""
        out = np.empty((self.params.ny, self.params.nx, 9), dtype=np.float64)
        _check(self.lib, self.lib.lbm_double_read_cells(self.handle, out.ctypes.data))
        return out

    def final_state(self) -> dict:
        shape = (self.params.ny, self.params.nx)
        f = {k: np.empty(shape, dtype=np.float64) for k in ("u_x", "u_y", "u", "pressure")}
        _check(self.lib, self.lib.lbm_double_read_final_state(
            self.handle, f["u_x"].ctypes.data, f["u_y"].ctypes.data, f["u"].ctypes.data,
            f["pressure"].ctypes.data))
        return f

    def _scalar(self, fn) -> float:
        v = ctypes.c_double()
        _check(self.lib, fn(self.handle, ctypes.byref(v)))
        return float(v.value)

    def av_velocity(self) -> float:
        return self._scalar(self.lib.lbm_double_av_velocity)

    def total_density(self) -> float:
        return self._scalar(self.lib.lbm_double_total_density)

    def reynolds(self) -> float:
        return self._scalar(self.lib.lbm_double_calc_reynolds)


# ------------------------------------------------------------------------------------------------
# batches: many small lattices advanced together
# ------------------------------------------------------------------------------------------------
class Batch:
    """B independent lattices of one shape on one device, advanced together (lbm_create_batch): a sweep over
    omega / accel / obstacle maps in one engine.  Each member is bit-identical to an :class:`Engine` run on the same
    inputs; :meth:`member` gives the readers of one of them."""

    def __init__(self, params_list, obstacles, cells=None, math: str | int = "exact"):
        self.lib = load_library()
        self.handle = None
        self.params = list(params_list)
        n = len(self.params)
        if n < 1:
            raise LbmError("lbm_create_batch: n_members must be at least 1 (got 0)")
        p0 = self.params[0]
        for i, p in enumerate(self.params):
            if p.nx < 1 or p.ny < 2 or p.max_iters < 0:
                raise LbmError(f"lbm_create_batch: member {i} has invalid parameters")
            if (p.nx, p.ny) != (p0.nx, p0.ny):
                raise LbmError(f"lbm_create_batch: member {i} is {p.nx}x{p.ny}, member 0 is {p0.nx}x{p0.ny}")
            if p.max_iters != p0.max_iters:
                raise LbmError(f"lbm_create_batch: member {i} has max_iters {p.max_iters}, member 0 has {p0.max_iters}")
        if math not in _MATH:
            raise LbmError(f"lbm_create_batch: unknown math mode {math!r}")
        self._obstacles = self._stack(obstacles, n, (p0.ny, p0.nx), np.int32, "obstacle maps")
        self._cells = None if cells is None else self._stack(cells, n, (p0.ny, p0.nx, 9), np.float32, "initial lattices")
        cparams = (_CParams * n)(*[p._c() for p in self.params])
        h = self.lib.lbm_create_batch(n, cparams, self._obstacles.ctypes.data,
                                      None if self._cells is None else self._cells.ctypes.data, _MATH[math])
        if not h:
            raise LbmError(self.lib.lbm_last_error().decode())
        self.handle = ctypes.c_void_p(h)
        self._members = [None] * n

    @staticmethod
    def _stack(arrays, n, shape, dtype, what) -> np.ndarray:
        """A sequence of n arrays, or one stacked array, of `shape` each -> contiguous [n, *shape]."""
        items = [np.asarray(a) for a in arrays]
        if len(items) != n:
            raise LbmError(f"lbm_create_batch: {len(items)} {what} for {n} members")
        size = int(np.prod(shape))
        for i, a in enumerate(items):
            if a.size != size:
                raise LbmError(f"lbm_create_batch: member {i}: {what[:-1]} of {a.size} values, expected {'x'.join(map(str, shape))}")
        return np.ascontiguousarray(np.stack([a.reshape(shape) for a in items]), dtype=dtype)

    def __len__(self) -> int:
        return len(self.params)

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.lbm_destroy_batch(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not self.handle:
            raise LbmError("the batch is closed")
        return self.handle

    # -- hot path ----------------------------------------------------------------------------
    def run(self, n_steps: int) -> None:
        """Advance every member by n_steps (lbm_batch_run)."""
        _check(self.lib, self.lib.lbm_batch_run(self._live(), int(n_steps)))

    def sync(self) -> None:
        _check(self.lib, self.lib.lbm_batch_sync(self._live()))

    def run_until(self, max_steps: int, check_every: int = 1024, tol: float = 1e-6, patience: int = 2) -> list[dict]:
        """Advance every member until all of them are steady, or by max_steps (lbm_batch_run_until).  One dict per
        member as Engine.run_until's; steps_run is the batch's, steady_step the member's own."""
        args = _steady_args(max_steps, check_every, tol, patience)
        res = (_CSteadyResult * len(self))()
        steps = ctypes.c_int()
        _check(self.lib, self.lib.lbm_batch_run_until(self._live(), *args, res, ctypes.byref(steps)))
        return [r.as_dict() for r in res]

    def run_until_residual(self, max_steps: int, check_every: int = 1024, tol: float = 1e-4, patience: int = 2, history=None) -> list[dict]:
        """Engine.run_until_residual for every member at once (lbm_batch_run_until_residual): every member its own
        baseline, rows and verdict, frozen once it is steady or diverged; the batch ends when every member is, or at
        max_steps.  A list of one dict per member as Engine.run_until_residual's without "history" (steps_run is the
        batch's); the history of the batch is attached once, to the list: its attribute `history` is
        (steps int32[n], RESIDUAL_DTYPE[n, members])."""
        args = _steady_args(max_steps, check_every, tol, patience)
        capacity = _until_history_arg(history, args[0], args[1])
        res = (_CResidualSteadyResult * len(self))()
        steps = ctypes.c_int()
        rows = np.zeros((capacity, len(self)), dtype=RESIDUAL_DTYPE)
        _check(self.lib, self.lib.lbm_batch_run_until_residual(self._live(), *args, res, ctypes.byref(steps), rows.ctypes.data, capacity))
        out = _BatchResidualSteady(r.as_dict() for r in res)
        n = min(steps.value // args[1], capacity)      # segments judged: the call ends with a checked segment or at the cap
        out.history = (np.arange(1, n + 1, dtype=np.int32) * np.int32(args[1]), rows[:n])
        return out

    def info(self) -> dict:
        bi = _CBatchInfo()
        _check(self.lib, self.lib.lbm_batch_get_info(self._live(), ctypes.byref(bi)))
        return {name: getattr(bi, name) for name, _ in _CBatchInfo._fields_}

    # -- obstacle forces of all members (lbm_batch_set_forces / lbm_batch_read_forces / lbm_batch_forces_links) ------
    def set_forces(self, every: int, capacity: int = 4096, bodies=None, n_bodies: int | None = None) -> None:
        """Engine.set_forces for every member at once: one `every`, `capacity` and `n_bodies` for the batch, rows in one
        device ring.  `bodies`: None (in every member all blocked cells are body 0) or one label map (ny, nx) per member,
        as a sequence or stacked [members, ny, nx]; n_bodies defaults to the largest label of any member + 1.
        every == 0 disarms; re-arming discards unread rows."""
        p0 = self.params[0]
        every, capacity, n_bodies, labels = _batch_forces_args(every, capacity, bodies, n_bodies, len(self), p0.nx, p0.ny)
        _check(self.lib, self.lib.lbm_batch_set_forces(self._live(), n_bodies, labels.ctypes.data if labels is not None else None,
                                                       every, capacity))
        self._n_bodies = n_bodies if every > 0 else 0

    def forces(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[n],
        float64[n, members, n_bodies, 2]), columns F_x, F_y."""
        return _drain_rows(self.lib.lbm_batch_read_forces, self.lib, self._live(), "forces", max_rows,
                           (len(self), getattr(self, "_n_bodies", 0), 2), np.float64, np.empty)

    # -- lattice statistics of all members (lbm_batch_set_stats / lbm_batch_read_stats) -----------------------------
    def set_stats(self, every: int, capacity: int = 4096) -> None:
        """Engine.set_stats for every member at once: one `every` and `capacity` for the batch, rows in one device ring,
        one gather launch per sample whatever the number of members."""
        every, capacity = _stats_args(every, capacity)
        _check(self.lib, self.lib.lbm_batch_set_stats(self._live(), every, capacity))

    def stats(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[n], STATS_DTYPE[n, members])."""
        return _drain_rows(self.lib.lbm_batch_read_stats, self.lib, self._live(), "stats", max_rows, (len(self),), STATS_DTYPE, np.zeros)

    # -- enstrophy of all members (lbm_batch_set_enstrophy / lbm_batch_read_enstrophy) -----------------------------------
    def set_enstrophy(self, every: int, capacity: int = 4096) -> None:
        """Engine.set_enstrophy for every member at once: one `every` and `capacity` for the batch, rows in one device
        ring, one gather launch per sample for all members.  every == 0 disarms."""
        every, capacity = _enstrophy_args(every, capacity)
        _check(self.lib, self.lib.lbm_batch_set_enstrophy(self._live(), every, capacity))

    def enstrophy(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[n], ENSTROPHY_DTYPE[n, members])."""
        return _drain_rows(self.lib.lbm_batch_read_enstrophy, self.lib, self._live(), "enstrophy", max_rows, (len(self),),
                           ENSTROPHY_DTYPE, np.zeros)

    # -- stress rows of all members (lbm_batch_set_stress / lbm_batch_read_stress_rows) --------------------------------------
    def set_stress(self, every: int, capacity: int = 4096) -> None:
        """Engine.set_stress for every member at once: one `every` and `capacity` for the batch, rows in one device ring,
        one gather launch per sample whatever the number of members.  every == 0 disarms."""
        every, capacity = _every_capacity("set_stress", every, capacity, "row")
        _check(self.lib, self.lib.lbm_batch_set_stress(self._live(), every, capacity))

    def stress_rows(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[n], STRESS_DTYPE[n, members])."""
        return _drain_rows(self.lib.lbm_batch_read_stress_rows, self.lib, self._live(), "stress_rows", max_rows, (len(self),),
                           STRESS_DTYPE, np.zeros)

    # -- tracer particles of all members (lbm_batch_set_tracers / lbm_batch_read_tracers / lbm_batch_tracers_now) ------------
    def set_tracers(self, xy, every: int, capacity: int = 0) -> None:
        """Engine.set_tracers for every member at once: `xy` is float64 (members, n, 2), n tracers per member; one `every`
        and `capacity` for the batch, rows in one device ring, one launch per sample whatever the number of members.
        every == 0 or n == 0 disarms."""
        xy, every, capacity = _tracer_args("set_tracers", xy, (len(self),), every, capacity)
        _check(self.lib, self.lib.lbm_batch_set_tracers(self._live(), xy.shape[1], xy.ctypes.data, every, capacity))
        self._n_tracers = xy.shape[1] if every > 0 else 0

    def tracer_rows(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[rows], float64[rows, members, n, 2])."""
        return _drain_rows(self.lib.lbm_batch_read_tracers, self.lib, self._live(), "tracer_rows", max_rows,
                           (len(self), getattr(self, "_n_tracers", 0), 2), np.float64, np.zeros)

    def tracers(self) -> np.ndarray:
        """Every member's tracers' current positions, float64 (members, n, 2).  Drains nothing."""
        out = np.empty((len(self), getattr(self, "_n_tracers", 0), 2), dtype=np.float64)
        _check(self.lib, self.lib.lbm_batch_tracers_now(self._live(), out.ctypes.data))
        return out

    # -- stream function of all members (lbm_batch_set_psi / lbm_batch_read_psi_rows) ---------------------------------------
    def set_psi(self, every: int, capacity: int = 4096) -> None:
        """Engine.set_psi for every member at once: one `every` and `capacity` for the batch, rows in one device ring, one
        launch of each of the scan's kernels per sample for all members.  every == 0 disarms."""
        every, capacity = _psi_args(every, capacity)
        _check(self.lib, self.lib.lbm_batch_set_psi(self._live(), every, capacity))

    def psi_rows(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[n], PSI_DTYPE[n, members])."""
        return _drain_rows(self.lib.lbm_batch_read_psi_rows, self.lib, self._live(), "psi_rows", max_rows, (len(self),),
                           PSI_DTYPE, np.zeros)

    # -- velocity residuals of all members (lbm_batch_set_residual / lbm_batch_read_residual) ------------------------
    def set_residual(self, every: int, capacity: int = 4096) -> None:
        """Engine.set_residual for every member at once: one `every` and `capacity` for the batch, rows in one device
        ring, one gather launch for the baselines and one per sample whatever the number of members."""
        every, capacity = _residual_args(every, capacity)
        _check(self.lib, self.lib.lbm_batch_set_residual(self._live(), every, capacity))

    def residuals(self, max_rows: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_rows (default: all) waiting rows, oldest first: (steps int32[n], RESIDUAL_DTYPE[n, members])."""
        return _drain_rows(self.lib.lbm_batch_read_residual, self.lib, self._live(), "residuals", max_rows, (len(self),), RESIDUAL_DTYPE,
                           np.zeros)

    # -- line profiles of all members (lbm_batch_set_profiles / lbm_batch_read_profiles) ------------------------------
    def set_profiles(self, every: int, capacity: int = 16, axes=("rows", "columns")) -> None:
        """Engine.set_profiles for every member at once: one `every`, one `axes` and one `capacity` for the batch,
        records in one device ring, one launch per selected axis and sample whatever the number of members."""
        every, capacity, axes = _profile_args(every, capacity, axes)
        _check(self.lib, self.lib.lbm_batch_set_profiles(self._live(), every, capacity, axes))
        self._profile_axes = axes if every > 0 else 0

    def profiles(self, max_records: int | None = None) -> tuple[np.ndarray, dict]:
        """Drain up to max_records (default: all) waiting records, oldest first: (steps int32[n], {"rows":
        PROFILE_DTYPE[n, members, ny], "columns": PROFILE_DTYPE[n, members, nx]}), the selected keys only."""
        return _read_profiles(self.lib.lbm_batch_read_profiles, self.lib, self._live(), max_records, getattr(self, "_profile_axes", 0),
                              (len(self),), self.params[0].nx, self.params[0].ny)

    # -- coarse frames of all members (lbm_batch_set_coarse_frames / lbm_batch_read_coarse_frames) ---------------------
    def set_coarse_frames(self, every: int, capacity: int = 16, box=(16, 16)) -> None:
        """Engine.set_coarse_frames for every member at once: one `every`, one `box` and one `capacity` for the batch,
        frames in one device ring, one launch per sample whatever the number of members."""
        every, capacity, bx, by = _coarse_args(every, capacity, box)
        _check(self.lib, self.lib.lbm_batch_set_coarse_frames(self._live(), every, capacity, bx, by))
        self._coarse_box = (bx, by) if every > 0 else None

    def coarse_frames(self, max_frames: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Drain up to max_frames (default: all) waiting frames, oldest first: (steps int32[n], PROFILE_DTYPE[n, members,
        cy, cx])."""
        return _read_coarse_frames(self.lib.lbm_batch_read_coarse_frames, self.lib, self._live(), max_frames, getattr(self, "_coarse_box", None),
                                   (len(self),), self.params[0].nx, self.params[0].ny)

    def force_links(self) -> np.ndarray:
        """Boundary links of every body of every member of the armed forces, int32[members, n_bodies]
        (lbm_batch_forces_links)."""
        n_bodies = getattr(self, "_n_bodies", 0)
        out = np.zeros(max(1, len(self) * n_bodies), dtype=np.int32)
        _check(self.lib, self.lib.lbm_batch_forces_links(self._live(), out.ctypes.data))
        return out[:len(self) * n_bodies].reshape(len(self), n_bodies).copy()

    def member(self, index: int) -> "BatchMember":
        """Read-only view of member `index` (lbm_batch_member)."""
        if not 0 <= index < len(self):
            raise LbmError(f"lbm_batch_member: index {index} out of range (the batch has {len(self)} members)")
        if self._members[index] is None:
            h = self.lib.lbm_batch_member(self._live(), int(index))
            if not h:
                raise LbmError(self.lib.lbm_last_error().decode())
            self._members[index] = BatchMember(self, index, ctypes.c_void_p(h))
        return self._members[index]


class BatchMember(Engine):
    """One member of a :class:`Batch`: the readers of :class:`Engine` (av_vels, cells, final_state, av_velocity,
    total_density, reynolds, info).  The batch advances and owns it: run() raises, close() does nothing."""

    def __init__(self, batch: Batch, index: int, handle):
        self.lib = batch.lib
        self.params = batch.params[index]
        self.index = index
        self._batch = batch
        self._handle = handle

    @property
    def handle(self):
        self._batch._live()
        return self._handle

    def close(self) -> None:
        pass

    def run_until(self, *args, **kwargs):
        raise LbmError("run_until: this engine is a member of a batch; Batch.run_until advances all its members")

    def run_until_residual(self, *args, **kwargs):
        raise LbmError("run_until_residual: this engine is a member of a batch; Batch.run_until_residual advances all its members")


# ------------------------------------------------------------------------------------------------
# file formats of the command line (Python twins of host/lbm_io.c, for tests and bench.py)
# ------------------------------------------------------------------------------------------------
def read_params(path: str) -> Params:
    """7 whitespace-separated values, fixed order (SerialCode/d2q9-bgk.c:480-506)."""
    with open(path) as fh:
        tok = fh.read().split()
    names = ("nx", "ny", "maxIters", "reynolds_dim", "density", "accel", "omega")
    if len(tok) < 7:
        raise LbmError(f"could not read param file: {names[len(tok)]}")
    try:
        return Params(int(tok[0]), int(tok[1]), int(tok[2]), int(tok[3]),
                      float(tok[4]), float(tok[5]), float(tok[6]))
    except ValueError as exc:
        raise LbmError(f"could not read param file: {exc}") from None


def read_params_double(path: str) -> ParamsDouble:
    """The same file with density, accel and omega kept as doubles: 1.85 is 1.85, not float32(1.85)."""
    p = read_params(path)
    return ParamsDouble(p.nx, p.ny, p.max_iters, p.reynolds_dim, p.density, p.accel, p.omega)


def read_obstacles(path: str, nx: int, ny: int) -> np.ndarray:
    """'x y 1' lines -> int32 (ny, nx) map; the reference's range checks (:590-597)."""
    grid = np.zeros((ny, nx), dtype=np.int32)
    with open(path) as fh:
        tok = fh.read().split()
    if len(tok) % 3:
        raise LbmError("expected 3 values per line in obstacle file")
    try:
        arr = np.array(tok, dtype=np.int64).reshape(-1, 3)
    except ValueError:
        raise LbmError("expected 3 values per line in obstacle file") from None
    if arr.size:
        if (arr[:, 0] < 0).any() or (arr[:, 0] > nx - 1).any():
            raise LbmError("obstacle x-coord out of range")
        if (arr[:, 1] < 0).any() or (arr[:, 1] > ny - 1).any():
            raise LbmError("obstacle y-coord out of range")
        if (arr[:, 2] != 1).any():
            raise LbmError("obstacle blocked value should be 1")
        grid[arr[:, 1], arr[:, 0]] = 1
    return grid


def tile_obstacles(tile: np.ndarray, nx: int, ny: int) -> np.ndarray:
    """Synthetic large grids: repeat a small map periodically."""
    ty, tx = tile.shape
    reps = (-(-ny // ty), -(-nx // tx))
    return np.ascontiguousarray(np.tile(tile, reps)[:ny, :nx], dtype=np.int32)


def write_av_vels(path: str, av_vels: np.ndarray) -> None:
    """'%d:\\t%.12E\\n' (SerialCode/d2q9-bgk.c:735-738).  A float64 series (DoubleEngine.av_vels) is written as it is."""
    av_vels = np.asarray(av_vels)
    if av_vels.dtype != np.float64:
        av_vels = av_vels.astype(np.float32)
    with open(path, "w") as fh:
        for i, v in enumerate(av_vels):
            fh.write("%d:\t%.12E\n" % (i, float(v)))


def _every_capacity(setter, every, capacity, record) -> tuple[int, int]:
    """What the recorders' argument checks begin with, under the setter's name: `every` and `capacity` are integers in
    [0, 2^31) and an armed ring holds at least one `record` (None: the caller checks that itself)."""
    for name, v in (("every", every), ("capacity", capacity)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise LbmError(f"{setter}: {name} must be an integer (got {v!r})")
        if not 0 <= int(v) <= 2147483647:
            raise LbmError(f"{setter}: {name} must lie in [0, 2^31) (got {v})")
    if record is not None and every > 0 and capacity < 1:
        raise LbmError(f"{setter}: capacity {capacity}, at least one {record} is needed")
    return int(every), int(capacity)


def _drain_rows(reader, lib, handle, method, max_rows, row_shape, dtype, alloc) -> tuple[np.ndarray, np.ndarray]:
    """What the row readers of Engine and Batch (forces, stats, residuals) share: up to max_rows (None: all) waiting rows
    through `reader`, oldest first, as (steps int32[n], dtype[n, *row_shape]); alloc: np.empty or np.zeros."""
    if max_rows is not None and (isinstance(max_rows, bool) or not isinstance(max_rows, (int, np.integer)) or max_rows < 0):
        raise LbmError(f"{method}: max_rows must be a non-negative integer or None (got {max_rows!r})")
    n = ctypes.c_int()
    _check(lib, reader(handle, 0, None, None, ctypes.byref(n)))  # rows waiting
    max_rows = n.value if max_rows is None else min(int(max_rows), n.value)
    rows = alloc((int(max_rows),) + tuple(row_shape), dtype=dtype)
    steps = np.empty(int(max_rows), dtype=np.int32)
    _check(lib, reader(handle, int(max_rows), rows.ctypes.data, steps.ctypes.data, ctypes.byref(n)))
    return steps[:n.value].copy(), rows[:n.value].copy()


def _frame_args(every, capacity) -> tuple[int, int]:
    """Engine.set_frames' argument checks (no device needed)."""
    return _every_capacity("set_frames", every, capacity, "frame slot")


# the fields of a field frame under final_state()'s keys, in the order of their planes (LBM_FIELD_* of include/lbm_hip.h)
FIELD_NAMES = ("u_x", "u_y", "u", "pressure")
FIELD_BITS = {"u_x": 1, "u_y": 2, "u": 4, "pressure": 8}


def _field_frame_args(every, capacity, fields, window) -> tuple[int, int, int, tuple | None]:
    """Engine.set_field_frames' argument checks (no device needed): (every, capacity, LBM_FIELD_* mask, window or None)."""
    every, capacity = _every_capacity("set_field_frames", every, capacity, "frame slot")
    if isinstance(fields, str):
        fields = (fields,)
    try:
        names = list(fields)
    except TypeError:
        raise LbmError(f"set_field_frames: fields must be a sequence of names among {FIELD_NAMES} (got {fields!r})") from None
    if not names:
        raise LbmError(f"set_field_frames: no fields, at least one of {FIELD_NAMES} is needed")
    mask = 0
    for name in names:
        if not isinstance(name, str) or name not in FIELD_BITS:
            raise LbmError(f"set_field_frames: unknown field {name!r}, the fields are {FIELD_NAMES}")
        if mask & FIELD_BITS[name]:
            raise LbmError(f"set_field_frames: field {name!r} is named twice")
        mask |= FIELD_BITS[name]
    if window is not None:
        try:
            win = tuple(window)
        except TypeError:
            win = ()
        if len(win) != 4 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in win):
            raise LbmError(f"set_field_frames: window must be four integers (x0, y0, nx, ny) (got {window!r})")
        if not all(0 <= int(v) <= 2147483647 for v in win):
            raise LbmError(f"set_field_frames: window values must lie in [0, 2^31) (got {window!r})")
        if win[2] < 1 or win[3] < 1:
            raise LbmError(f"set_field_frames: a window of {win[2]} x {win[3]} cells, at least 1 x 1 is needed")
        window = tuple(int(v) for v in win)
    return int(every), int(capacity), mask, window


LBM_MAX_PROBES = 256


class _CProbe(ctypes.Structure):
    _fields_ = [("x", ctypes.c_int), ("y", ctypes.c_int)]


class _CProbeSample(ctypes.Structure):
    _fields_ = [("u_x", ctypes.c_float), ("u_y", ctypes.c_float), ("u_mag", ctypes.c_float), ("pressure", ctypes.c_float)]


def _probe_args(cells, every, capacity) -> tuple[list, int, int]:
    """Engine.set_probes' argument checks (no device needed): ([(x, y), ...], every, capacity)."""
    every, capacity = _every_capacity("set_probes", every, capacity, None)
    try:
        items = list(cells)
    except TypeError:
        raise LbmError(f"set_probes: cells must be a sequence of (x, y) pairs (got {cells!r})") from None
    if len(items) > LBM_MAX_PROBES:
        raise LbmError(f"set_probes: {len(items)} probes, at most LBM_MAX_PROBES = {LBM_MAX_PROBES} are possible")
    flat = []
    for i, cell in enumerate(items):
        try:
            pair = tuple(cell)
        except TypeError:
            pair = ()
        if len(pair) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in pair):
            raise LbmError(f"set_probes: cell {i} must be a pair of integers (x, y) (got {cell!r})")
        if not all(-2147483648 <= int(v) <= 2147483647 for v in pair):
            raise LbmError(f"set_probes: cell {i} must be a pair of integers (x, y) (got {cell!r})")
        flat.append((int(pair[0]), int(pair[1])))
    if flat and every > 0 and capacity < 1:
        raise LbmError(f"set_probes: capacity {capacity}, at least one row of samples is needed")
    return flat, int(every), int(capacity)


LBM_MAX_BODIES = 64


def _forces_args(every, capacity, bodies, n_bodies, nx, ny) -> tuple[int, int, int, np.ndarray | None]:
    """Engine.set_forces' argument checks (no device needed): (every, capacity, n_bodies, int32 labels [ny*nx] or None).
    Whether a blocked cell's label lies outside 0 .. n_bodies - 1 is the engine's check: it holds the obstacle mask."""
    every, capacity = _every_capacity("set_forces", every, capacity, "row")
    labels = None
    if bodies is not None:
        try:
            labels = np.asarray(bodies)
        except (TypeError, ValueError):
            raise LbmError(f"set_forces: bodies must be an integer array of shape ({ny}, {nx}) (got {bodies!r})"[:300]) from None
        if labels.dtype.kind not in "iu" or labels.size != nx * ny or labels.shape not in ((ny, nx), (ny * nx,)):
            raise LbmError(f"set_forces: bodies must be an integer array of shape ({ny}, {nx}) (got {bodies!r})"[:300])
        if labels.size and (labels.min() < -2147483648 or labels.max() > 2147483647):
            raise LbmError("set_forces: body labels must fit 32 bits")
        labels = np.ascontiguousarray(labels.reshape(-1), dtype=np.int32)
    if n_bodies is None:
        n_bodies = 1 if labels is None or labels.size == 0 else max(1, int(labels.max()) + 1)
    if isinstance(n_bodies, bool) or not isinstance(n_bodies, (int, np.integer)):
        raise LbmError(f"set_forces: n_bodies must be an integer (got {n_bodies!r})")
    if every > 0 and not 1 <= int(n_bodies) <= LBM_MAX_BODIES:
        raise LbmError(f"set_forces: {int(n_bodies)} bodies, between 1 and LBM_MAX_BODIES = {LBM_MAX_BODIES} are possible")
    return int(every), int(capacity), int(n_bodies), labels


def _batch_forces_args(every, capacity, bodies, n_bodies, members, nx, ny) -> tuple[int, int, int, np.ndarray | None]:
    """Batch.set_forces' argument checks (no device needed): _forces_args for every member's label map; (every, capacity,
    n_bodies, int32 labels [members, ny*nx] or None), n_bodies by default the largest any member needs."""
    if bodies is None:
        return _forces_args(every, capacity, None, n_bodies, nx, ny)
    try:
        maps = list(bodies)
    except TypeError:
        raise LbmError(f"set_forces: bodies must be one integer array of shape ({ny}, {nx}) per member (got {bodies!r})"[:300]) from None
    if len(maps) != members:
        raise LbmError(f"set_forces: {len(maps)} label maps for {members} members")
    checked = [_forces_args(every, capacity, m, n_bodies, nx, ny) for m in maps]
    every, capacity = checked[0][:2]
    n_bodies = max(c[2] for c in checked)
    return every, capacity, n_bodies, np.ascontiguousarray(np.stack([c[3] for c in checked]), dtype=np.int32)


def write_forces(path: str, steps, rows) -> None:
    """forces.dat of the command line (LBM_FORCES): '%d:\t%.12E\t%.12E\n' = tt, F_x, F_y, one line per sample, the forces
    summed over the bodies in body order; `steps` int[n], `rows` float64 [n, n_bodies, 2] (Engine.forces)."""
    rows = np.asarray(rows, dtype=np.float64)
    steps = np.asarray(steps).ravel()
    if rows.ndim != 3 or rows.shape[2] != 2 or rows.shape[0] != steps.size:
        raise LbmError(f"write_forces: rows must be [{steps.size}, n_bodies, 2] (got shape {rows.shape})")
    with open(path, "w") as fh:
        for tt, row in zip(steps.tolist(), rows):
            fx = fy = 0.0
            for b in range(row.shape[0]):
                fx += float(row[b, 0])
                fy += float(row[b, 1])
            fh.write("%d:\t%.12E\t%.12E\n" % (tt, fx, fy))


# lbm_stats_row of include/lbm_hip.h, 56 bytes
STATS_DTYPE = np.dtype([("mass", "<f8"), ("mom_x", "<f8"), ("mom_y", "<f8"), ("sum_u_sq", "<f8"), ("nonfinite", "<i8"),
                        ("max_u", "<f4"), ("max_x", "<i4"), ("max_y", "<i4"), ("reserved", "<i4")])


def _stats_args(every, capacity) -> tuple[int, int]:
    """Engine.set_stats' argument checks (no device needed): (every, capacity)."""
    return _every_capacity("set_stats", every, capacity, "row")


def write_stats(path: str, steps, rows) -> None:
    """stats.dat of the command line (LBM_STATS): one line per row, tt, a colon, then tab-separated mass, mom_x, mom_y,
    sum_u_sq and max_u as '%.12E' and max_x, max_y and nonfinite as '%d'; `steps` int[n], `rows` STATS_DTYPE[n]
    (Engine.stats)."""
    rows = np.asarray(rows)
    steps = np.asarray(steps).ravel()
    if rows.dtype != STATS_DTYPE or rows.ndim != 1 or rows.shape[0] != steps.size:
        raise LbmError(f"write_stats: rows must be {steps.size} rows of STATS_DTYPE (got shape {rows.shape}, dtype {rows.dtype})")
    with open(path, "w") as fh:
        for tt, r in zip(steps.tolist(), rows):
            fh.write("%d:\t%.12E\t%.12E\t%.12E\t%.12E\t%.12E\t%d\t%d\t%d\n" % (
                tt, float(r["mass"]), float(r["mom_x"]), float(r["mom_y"]), float(r["sum_u_sq"]), float(r["max_u"]),
                int(r["max_x"]), int(r["max_y"]), int(r["nonfinite"])))


# lbm_enstrophy_row of include/lbm_hip.h, 40 bytes
ENSTROPHY_DTYPE = np.dtype([("enstrophy", "<f8"), ("circulation", "<f8"), ("nonfinite", "<i8"), ("max_abs_w", "<f4"),
                            ("max_x", "<i4"), ("max_y", "<i4"), ("fluid", "<i4")])


def _enstrophy_args(every, capacity) -> tuple[int, int]:
    """Engine.set_enstrophy's argument checks (no device needed): (every, capacity)."""
    return _every_capacity("set_enstrophy", every, capacity, "row")


def write_enstrophy(path: str, steps, rows) -> None:
    """One line per row in write_stats' style: tt, a colon, then tab-separated enstrophy, circulation and max_abs_w as
    '%.12E' and max_x, max_y, fluid and nonfinite as '%d'; `steps` int[n], `rows` ENSTROPHY_DTYPE[n] (Engine.enstrophy)."""
    rows = np.asarray(rows)
    steps = np.asarray(steps).ravel()
    if rows.dtype != ENSTROPHY_DTYPE or rows.ndim != 1 or rows.shape[0] != steps.size:
        raise LbmError(f"write_enstrophy: rows must be {steps.size} rows of ENSTROPHY_DTYPE (got shape {rows.shape}, dtype {rows.dtype})")
    with open(path, "w") as fh:
        for tt, r in zip(steps.tolist(), rows):
            fh.write("%d:\t%.12E\t%.12E\t%.12E\t%d\t%d\t%d\t%d\n" % (
                tt, float(r["enstrophy"]), float(r["circulation"]), float(r["max_abs_w"]), int(r["max_x"]), int(r["max_y"]),
                int(r["fluid"]), int(r["nonfinite"])))


# lbm_stress_row of include/lbm_hip.h, 40 bytes
STRESS_DTYPE = np.dtype([("sum_q", "<f8"), ("sum_txy", "<f8"), ("nonfinite", "<i8"), ("max_q", "<f4"),
                         ("max_x", "<i4"), ("max_y", "<i4"), ("fluid", "<i4")])


def write_stress_rows(path: str, steps, rows) -> None:
    """One line per row in write_enstrophy's style: tt, a colon, then tab-separated sum_q, sum_txy and max_q as '%.12E'
    and max_x, max_y, fluid and nonfinite as '%d'; `steps` int[n], `rows` STRESS_DTYPE[n] (Engine.stress_rows)."""
    rows = np.asarray(rows)
    steps = np.asarray(steps).ravel()
    if rows.dtype != STRESS_DTYPE or rows.ndim != 1 or rows.shape[0] != steps.size:
        raise LbmError(f"write_stress_rows: rows must be {steps.size} rows of STRESS_DTYPE (got shape {rows.shape}, dtype {rows.dtype})")
    with open(path, "w") as fh:
        for tt, r in zip(steps.tolist(), rows):
            fh.write("%d:\t%.12E\t%.12E\t%.12E\t%d\t%d\t%d\t%d\n" % (
                tt, float(r["sum_q"]), float(r["sum_txy"]), float(r["max_q"]), int(r["max_x"]), int(r["max_y"]),
                int(r["fluid"]), int(r["nonfinite"])))


def _tracer_args(setter, xy, lead, every, capacity) -> tuple[np.ndarray, int, int]:
    """set_tracers' argument checks (no device needed): `xy` real numbers of shape lead + (n, 2), as contiguous float64;
    capacity 0 is allowed (no ring).  The library refuses positions outside the grid."""
    every, capacity = _every_capacity(setter, every, capacity, None)
    xy = np.asarray(xy)
    if xy.dtype.kind not in "fiu":
        raise LbmError(f"{setter}: xy must hold real numbers (got dtype {xy.dtype})")
    if xy.ndim != len(lead) + 2 or xy.shape[:len(lead)] != tuple(lead) or xy.shape[-1] != 2:
        want = "(" + ", ".join([str(m) for m in lead] + ["n", "2"]) + ")"
        raise LbmError(f"{setter}: xy must have shape {want}: positions (x, y) (got shape {xy.shape})")
    if xy.shape[-2] > MAX_TRACERS:
        raise LbmError(f"{setter}: {xy.shape[-2]} tracers, at most LBM_MAX_TRACERS = {MAX_TRACERS} are possible")
    return np.ascontiguousarray(xy, dtype=np.float64), every, capacity


MAX_TRACERS = 1 << 24    # LBM_MAX_TRACERS of include/lbm_hip.h


def write_tracers(path: str, steps, rows) -> None:
    """One line per row in write_stress_rows' style: tt, a colon, then tab-separated x and y of every tracer in the
    caller's order as '%.17E' (every double survives; a lost tracer reads NAN); `steps` int[rows], `rows`
    float64[rows, n, 2] (Engine.tracer_rows)."""
    rows = np.asarray(rows)
    steps = np.asarray(steps).ravel()
    if rows.dtype != np.float64 or rows.ndim != 3 or rows.shape[0] != steps.size or rows.shape[2] != 2:
        raise LbmError(f"write_tracers: rows must be float64 of shape ({steps.size}, n, 2) (got shape {rows.shape}, dtype {rows.dtype})")
    with open(path, "w") as fh:
        for tt, r in zip(steps.tolist(), rows):
            fh.write("%d:" % tt + "".join("\t%.17E\t%.17E" % (float(x), float(y)) for x, y in r) + "\n")


def tracer_seeds(obstacles, spacing: int) -> np.ndarray:
    """Start positions for set_tracers, float64 (n, 2): the centres (x, y) of the fluid cells among every `spacing`-th cell
    of every `spacing`-th row of the map `obstacles` (ny, nx), row-major.  In this order neighbouring tracers read
    neighbouring cells, which the kernel's loads then share; a shuffled cloud costs a cache line per cell."""
    if isinstance(spacing, bool) or not isinstance(spacing, (int, np.integer)) or spacing < 1:
        raise LbmError(f"tracer_seeds: spacing must be a positive integer (got {spacing!r})")
    ob = np.asarray(obstacles)
    if ob.ndim != 2:
        raise LbmError(f"tracer_seeds: obstacles must be a map of shape (ny, nx) (got shape {ob.shape})")
    ys, xs = np.nonzero(ob[::spacing, ::spacing] == 0)
    return np.stack([xs * int(spacing), ys * int(spacing)], axis=1).astype(np.float64)


def _strain_factor(who: str, omega) -> float:
    """c = 3 omega / (2 (1 - omega)) of S_ab = -c t_ab: the stored lattice is post-collision, its non-equilibrium part
    (1 - omega) times the pre-collision one.  Refuses omega outside (0, 2) and omega == 1."""
    omega = float(omega)
    if not 0.0 < omega < 2.0:
        raise ValueError(f"{who}: omega {omega!r} lies outside (0, 2)")
    if omega == 1.0:
        raise ValueError(f"{who}: at omega == 1 the stored lattice is pure equilibrium and carries no stress: "
                         "its second moment is rounding noise and the factor 1 / (1 - omega) does not exist")
    return 3.0 * omega / (2.0 * (1.0 - omega))


def strain_rate(stress: dict, omega: float) -> dict:
    """The strain-rate tensor of Engine.stress()'s planes, float64: {"S_xx", "S_xy", "S_yy"}, S_ab = -c t_ab with
    c = 3 omega / (2 (1 - omega)); `omega` is the one the lattice was advanced with."""
    c = _strain_factor("strain_rate", omega)
    return {"S_" + ab: -c * np.asarray(stress["t" + ab], dtype=np.float64) for ab in ("xx", "xy", "yy")}


def dissipation(rows, omega: float) -> np.ndarray:
    """The viscous dissipation 2 nu S:S summed over the finite fluid cells, per row of Engine.stress_rows, float64:
    2 nu c^2 sum_q with nu = (1 / omega - 1 / 2) / 3 (lattice units, per unit density)."""
    c = _strain_factor("dissipation", omega)
    nu = (1.0 / float(omega) - 0.5) / 3.0
    return 2.0 * nu * c * c * np.asarray(rows["sum_q"], dtype=np.float64)


def shear_rate_max(rows, omega: float) -> np.ndarray:
    """The largest shear rate sqrt(2 S:S) of a finite fluid cell, per row of Engine.stress_rows, float64:
    |c| sqrt(2 max_q), at the row's (max_x, max_y)."""
    c = _strain_factor("shear_rate_max", omega)
    return abs(c) * np.sqrt(2.0 * np.asarray(rows["max_q"], dtype=np.float64))


# lbm_psi_row of include/lbm_hip.h, 48 bytes
PSI_DTYPE = np.dtype([("psi_min", "<f8"), ("psi_max", "<f8"), ("nonfinite", "<i8"), ("min_x", "<i4"), ("min_y", "<i4"),
                      ("max_x", "<i4"), ("max_y", "<i4"), ("fluid", "<i4"), ("reserved", "<i4")])


def _psi_args(every, capacity) -> tuple[int, int]:
    """Engine.set_psi's argument checks (no device needed): (every, capacity)."""
    return _every_capacity("set_psi", every, capacity, "row")


def write_psi_rows(path: str, steps, rows) -> None:
    """One line per row in write_enstrophy's style: tt, a colon, then tab-separated psi_min and psi_max as '%.12E' and
    min_x, min_y, max_x, max_y, fluid and nonfinite as '%d'; `steps` int[n], `rows` PSI_DTYPE[n] (Engine.psi_rows)."""
    rows = np.asarray(rows)
    steps = np.asarray(steps).ravel()
    if rows.dtype != PSI_DTYPE or rows.ndim != 1 or rows.shape[0] != steps.size:
        raise LbmError(f"write_psi_rows: rows must be {steps.size} rows of PSI_DTYPE (got shape {rows.shape}, dtype {rows.dtype})")
    with open(path, "w") as fh:
        for tt, r in zip(steps.tolist(), rows):
            fh.write("%d:\t%.12E\t%.12E\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
                tt, float(r["psi_min"]), float(r["psi_max"]), int(r["min_x"]), int(r["min_y"]), int(r["max_x"]), int(r["max_y"]),
                int(r["fluid"]), int(r["nonfinite"])))


def write_psi(path: str, psi) -> None:
    """The field Engine.psi() gives, one 'x y psi' line per cell, rows from y = 0, psi as '%.12E': the input a contour
    plot needs."""
    psi = np.asarray(psi)
    if psi.dtype != np.float64 or psi.ndim != 2:
        raise LbmError(f"write_psi: psi must be a float64 array of shape (ny, nx) (got shape {psi.shape}, dtype {psi.dtype})")
    with open(path, "w") as fh:
        for y in range(psi.shape[0]):
            for x, v in enumerate(psi[y].tolist()):
                fh.write("%d %d %.12E\n" % (x, y, v))


# lbm_profile_line of include/lbm_hip.h, 48 bytes
PROFILE_DTYPE = np.dtype([("sum_rho", "<f8"), ("sum_jx", "<f8"), ("sum_jy", "<f8"), ("sum_ux", "<f8"), ("sum_uy", "<f8"),
                          ("fluid", "<i4"), ("nonfinite", "<i4")])
PROFILE_ROWS = 1          # LBM_PROFILE_ROWS
PROFILE_COLUMNS = 2       # LBM_PROFILE_COLUMNS
_PROFILE_AXES = {"rows": PROFILE_ROWS, "columns": PROFILE_COLUMNS}


def _profile_args(every, capacity, axes) -> tuple[int, int, int]:
    """Engine.set_profiles' argument checks (no device needed): (every, capacity, axes as LBM_PROFILE_* bits)."""
    every, capacity = _every_capacity("set_profiles", every, capacity, "record")
    if isinstance(axes, bool):
        raise LbmError(f"set_profiles: axes must be 1, 2, 3 or a subset of ('rows', 'columns') (got {axes!r})")
    if isinstance(axes, (int, np.integer)):
        bits = int(axes)
    elif isinstance(axes, str):
        raise LbmError(f"set_profiles: axes must be 1, 2, 3 or a subset of ('rows', 'columns') (got {axes!r}; a single axis is ('{axes}',))")
    else:
        try:
            names = list(axes)
        except TypeError:
            raise LbmError(f"set_profiles: axes must be 1, 2, 3 or a subset of ('rows', 'columns') (got {axes!r})") from None
        bits = 0
        for a in names:
            if not isinstance(a, str) or a not in _PROFILE_AXES:
                raise LbmError(f"set_profiles: unknown axis {a!r}; the axes are 'rows' and 'columns'")
            bits |= _PROFILE_AXES[a]
    if not 1 <= bits <= 3:
        raise LbmError(f"set_profiles: axes {axes!r} select nothing the engine records; 1 (rows), 2 (columns) or 3 (both) are possible")
    return int(every), int(capacity), bits


def _read_profiles(reader, lib, handle, max_records, axes, members, nx, ny) -> tuple[np.ndarray, dict]:
    """What Engine.profiles and Batch.profiles share: the waiting records through `reader`, split into the selected axes;
    members: () or (n_members,)."""
    if max_records is not None and (isinstance(max_records, bool) or not isinstance(max_records, (int, np.integer)) or max_records < 0):
        raise LbmError(f"profiles: max_records must be a non-negative integer or None (got {max_records!r})")
    n = ctypes.c_int()
    _check(lib, reader(handle, 0, None, None, ctypes.byref(n)))  # records waiting
    max_records = n.value if max_records is None else min(int(max_records), n.value)
    n_rows = ny if axes & PROFILE_ROWS else 0
    n_columns = nx if axes & PROFILE_COLUMNS else 0
    lines = np.zeros((int(max_records),) + tuple(members) + (max(1, n_rows + n_columns),), dtype=PROFILE_DTYPE)
    steps = np.empty(int(max_records), dtype=np.int32)
    _check(lib, reader(handle, int(max_records), lines.ctypes.data, steps.ctypes.data, ctypes.byref(n)))
    lines = lines[:n.value]
    out = {}
    if axes & PROFILE_ROWS:
        out["rows"] = lines[..., :n_rows].copy()
    if axes & PROFILE_COLUMNS:
        out["columns"] = lines[..., n_rows:n_rows + n_columns].copy()
    return steps[:n.value].copy(), out


def profile_means(lines) -> dict:
    """The means a profile is plotted as, of lines of PROFILE_DTYPE (any shape: one axis of a record, a stack of records,
    or the [cy, cx] boxes of a coarse frame, Engine.coarse), in float64: u_x, u_y, rho and j_x as sum / fluid, pressure as
    c_sq * rho (c_sq = 1/3); NaN where a line has no finite fluid cell (fluid == 0)."""
    lines = np.asarray(lines)
    fluid = np.asarray(lines["fluid"], dtype=np.float64)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for key, field in (("u_x", "sum_ux"), ("u_y", "sum_uy"), ("rho", "sum_rho"), ("j_x", "sum_jx")):
            out[key] = np.where(fluid == 0.0, np.nan, np.asarray(lines[field], dtype=np.float64) / fluid)
    out["pressure"] = out["rho"] * (1.0 / 3.0)
    return out


def write_profile(path: str, lines) -> None:
    """One text line per profile line of `lines` (PROFILE_DTYPE[n]: the rows or the columns of one record): its index,
    then tab-separated sum_rho, sum_jx, sum_jy, sum_ux and sum_uy as '%.12E' and fluid and nonfinite as '%d'."""
    lines = np.asarray(lines)
    if lines.dtype != PROFILE_DTYPE or lines.ndim != 1:
        raise LbmError(f"write_profile: lines must be one axis of one record, PROFILE_DTYPE[n] (got shape {lines.shape}, dtype {lines.dtype})")
    with open(path, "w") as fh:
        for i, r in enumerate(lines):
            fh.write("%d\t%.12E\t%.12E\t%.12E\t%.12E\t%.12E\t%d\t%d\n" % (
                i, float(r["sum_rho"]), float(r["sum_jx"]), float(r["sum_jy"]), float(r["sum_ux"]), float(r["sum_uy"]),
                int(r["fluid"]), int(r["nonfinite"])))


COARSE_MAX_BOX = 256      # LBM_COARSE_MAX_BOX


def _coarse_args(every, capacity, box, setter="set_coarse_frames") -> tuple[int, int, int, int]:
    """Engine.set_coarse_frames' argument checks (no device needed): (every, capacity, bx, by).  `box` is a pair of
    integers (bx, by) or one integer b for (b, b), each side in [1, COARSE_MAX_BOX]; the grid's sides are the engine's to
    check."""
    every, capacity = _every_capacity(setter, every, capacity, "frame")
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)  # noqa: E731
    if is_int(box):
        sides = (box, box)
    elif isinstance(box, (str, bytes)) or isinstance(box, bool):
        raise LbmError(f"{setter}: box must be a pair of integers (bx, by) or one integer (got {box!r})")
    else:
        try:
            sides = tuple(box)
        except TypeError:
            raise LbmError(f"{setter}: box must be a pair of integers (bx, by) or one integer (got {box!r})") from None
        if len(sides) != 2:
            raise LbmError(f"{setter}: box must be a pair of integers (bx, by) or one integer (got {box!r}: {len(sides)} values)")
        if not all(is_int(v) for v in sides):
            raise LbmError(f"{setter}: box must be a pair of integers (bx, by) or one integer (got {box!r})")
    for name, v in zip(("bx", "by"), sides):
        if not 1 <= int(v) <= COARSE_MAX_BOX:
            raise LbmError(f"{setter}: box side {name} must lie in [1, {COARSE_MAX_BOX}] (got {v})")
    return every, capacity, int(sides[0]), int(sides[1])


def _coarse_shape(nx, ny, bx, by) -> tuple[int, int]:
    """(cy, cx) of the coarse grid of bx x by boxes on nx x ny cells"""
    return -(-ny // by), -(-nx // bx)


def _read_coarse_frames(reader, lib, handle, max_frames, box, members, nx, ny) -> tuple[np.ndarray, np.ndarray]:
    """What Engine.coarse_frames and Batch.coarse_frames share: the waiting frames through `reader`; members: () or
    (n_members,); box: what this object armed, None: nothing (no frame waits)."""
    if max_frames is not None and (isinstance(max_frames, bool) or not isinstance(max_frames, (int, np.integer)) or max_frames < 0):
        raise LbmError(f"coarse_frames: max_frames must be a non-negative integer or None (got {max_frames!r})")
    shape = _coarse_shape(nx, ny, *box) if box else (1, 1)
    steps, frames = _drain_rows(reader, lib, handle, "coarse_frames", max_frames, tuple(members) + shape, PROFILE_DTYPE, np.zeros)
    return steps, frames if box else frames[:0]


def write_coarse_state(path: str, frame) -> None:
    """One coarse frame (PROFILE_DTYPE[cy, cx]: Engine.coarse, or one frame of Engine.coarse_frames) in final_state.dat's
    line format (write_final_state), one line per box, Y outer / X inner: 'X Y u_x u_y u pressure obstacle' with the box
    indices as coordinates, the box means of u_x and u_y (profile_means) and their magnitude, the mean of rho * c_sq as
    pressure, all rounded to float, and obstacle 1 where the box has no finite fluid cell (fluid == 0; its values are 0)."""
    frame = np.asarray(frame)
    if frame.dtype != PROFILE_DTYPE or frame.ndim != 2:
        raise LbmError(f"write_coarse_state: frame must be one frame, PROFILE_DTYPE[cy, cx] (got shape {frame.shape}, dtype {frame.dtype})")
    empty = frame["fluid"] == 0
    m = profile_means(frame)
    ux, uy, pr = (np.where(empty, 0.0, m[k]) for k in ("u_x", "u_y", "pressure"))
    fields = {"u_x": ux.astype(np.float32), "u_y": uy.astype(np.float32), "u": np.sqrt(ux * ux + uy * uy).astype(np.float32),
              "pressure": pr.astype(np.float32)}
    write_final_state(path, fields, empty.astype(np.int32))


# lbm_residual_row of include/lbm_hip.h, 40 bytes
RESIDUAL_DTYPE = np.dtype([("sum_du_sq", "<f8"), ("sum_u_sq", "<f8"), ("nonfinite", "<i8"), ("max_du", "<f4"), ("max_x", "<i4"),
                           ("max_y", "<i4"), ("span", "<i4")])


def _residual_args(every, capacity) -> tuple[int, int]:
    """Engine.set_residual's argument checks (no device needed): (every, capacity)."""
    return _every_capacity("set_residual", every, capacity, "row")


def residual_l2(rows) -> np.ndarray:
    """The relative L2 residual of rows of RESIDUAL_DTYPE (any shape), sqrt(sum_du_sq / sum_u_sq) in float64: 0.0 where
    both sums are 0 (a fluid at rest that stays at rest), inf where only sum_u_sq is."""
    rows = np.asarray(rows)
    du = np.asarray(rows["sum_du_sq"], dtype=np.float64)
    u = np.asarray(rows["sum_u_sq"], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where((du == 0.0) & (u == 0.0), 0.0, du / u)
    return np.sqrt(ratio)


def write_residuals(path: str, steps, rows) -> None:
    """One line per row in write_stats' style: tt, a colon, then tab-separated the relative L2 residual (residual_l2),
    sum_du_sq, sum_u_sq and max_du as '%.12E' and max_x, max_y, span and nonfinite as '%d'; `steps` int[n], `rows`
    RESIDUAL_DTYPE[n] (Engine.residuals)."""
    rows = np.asarray(rows)
    steps = np.asarray(steps).ravel()
    if rows.dtype != RESIDUAL_DTYPE or rows.ndim != 1 or rows.shape[0] != steps.size:
        raise LbmError(f"write_residuals: rows must be {steps.size} rows of RESIDUAL_DTYPE (got shape {rows.shape}, dtype {rows.dtype})")
    l2 = residual_l2(rows)
    with open(path, "w") as fh:
        for tt, r, v in zip(steps.tolist(), rows, l2.tolist()):
            fh.write("%d:\t%.12E\t%.12E\t%.12E\t%.12E\t%d\t%d\t%d\t%d\n" % (
                tt, v, float(r["sum_du_sq"]), float(r["sum_u_sq"]), float(r["max_du"]),
                int(r["max_x"]), int(r["max_y"]), int(r["span"]), int(r["nonfinite"])))


def _mean_args(every) -> int:
    """Engine.set_mean's argument checks (no device needed)."""
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)):
        raise LbmError(f"set_mean: every must be an integer (got {every!r})")
    if not 0 <= int(every) <= 2147483647:
        raise LbmError(f"set_mean: every must lie in [0, 2^31) (got {every})")
    return int(every)


def _mean_order_arg(order) -> int:
    """Engine.set_mean_order's check of `order` (no device needed)."""
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or int(order) not in (1, 2):
        raise LbmError(f"set_mean_order: order must be 1 (sums) or 2 (sums and sums of products) (got {order!r})")
    return int(order)


MOMENT_FIELDS = ("u_x u_x", "u_y u_y", "u_x u_y", "pressure pressure")


def fluctuations_of(sums: dict, sums2: dict, n: int) -> dict:
    """What Engine.fluctuations returns for the sums of Engine.mean_sums and Engine.moment_sums over n samples, all
    float64: with m = S1 / n and q = S2 / n,
      var_u_x = max(q_xx - m_x^2, 0), var_u_y, var_pressure likewise; cov_u_x_u_y = q_xy - m_x m_y (the Reynolds shear
      stress <u'v'>); rms_u_x, rms_u_y, rms_pressure their square roots; tke = 0.5 (var_u_x + var_u_y); samples = n.
    E[x^2] - E[x]^2 in float64 resolves a variance down to about 1e-16 of x^2 (the rounding of q and of m^2); a smaller
    one comes out as rounding noise of that size or, where negative, as 0 through the clamp.  Velocities are near 0.05,
    so variances below about 1e-19 are not resolved: ample for a flow that oscillates visibly."""
    if n == 0:
        raise LbmError("fluctuations: no sample has been taken since the mean fields were armed")
    m = {k: np.asarray(sums[k], dtype=np.float64) / float(n) for k in ("u_x", "u_y", "pressure")}
    q = {k: np.asarray(sums2[k], dtype=np.float64) / float(n) for k in MOMENT_FIELDS}
    out = {"var_u_x": np.maximum(q["u_x u_x"] - m["u_x"] * m["u_x"], 0.0),
           "var_u_y": np.maximum(q["u_y u_y"] - m["u_y"] * m["u_y"], 0.0),
           "cov_u_x_u_y": q["u_x u_y"] - m["u_x"] * m["u_y"],
           "var_pressure": np.maximum(q["pressure pressure"] - m["pressure"] * m["pressure"], 0.0)}
    for k in ("u_x", "u_y", "pressure"):
        out["rms_" + k] = np.sqrt(out["var_" + k])
    out["tke"] = 0.5 * (out["var_u_x"] + out["var_u_y"])
    out["samples"] = n
    return out


def write_rms_state(path: str, fluct: dict, obstacles: np.ndarray) -> None:
    """rms_state.dat of the command line (LBM_MEAN_ORDER=2): final_state.dat's line format,
    'x y rms_u_x rms_u_y cov_u_x_u_y rms_pressure obstacle' with '%.12E', from Engine.fluctuations rounded to float."""
    cols = ("rms_u_x", "rms_u_y", "cov_u_x_u_y", "rms_pressure")
    write_final_state(path, {k: np.asarray(fluct[c], dtype=np.float64).astype(np.float32)
                             for k, c in zip(("u_x", "u_y", "u", "pressure"), cols)}, np.asarray(obstacles))


def write_mean_state(path: str, mean: dict, obstacles: np.ndarray) -> None:
    """mean_state.dat of the command line: final_state.dat's line format, 'x y u_x u_y u pressure obstacle' with
    '%.12E', from the mean fields (Engine.mean) rounded to float."""
    write_final_state(path, {k: np.asarray(mean[k], dtype=np.float64).astype(np.float32) for k in ("u_x", "u_y", "u", "pressure")},
                      np.asarray(obstacles))


def write_probes(path: str, cells, steps, samples) -> None:
    """probes.dat of the command line: '%d %d %d %.12E %.12E %.12E %.12E\n' = tt x y u_x u_y u pressure, one line per
    sample and probe, sample-major; `steps` int[n], `samples` float32 [n, n_probes, 4] (Engine.probes)."""
    cells = [(int(x), int(y)) for x, y in cells]
    samples = np.asarray(samples, dtype=np.float32)
    steps = np.asarray(steps).ravel()
    if samples.ndim != 3 or samples.shape[1:] != (len(cells), 4) or samples.shape[0] != steps.size:
        raise LbmError(f"write_probes: samples must be [{steps.size}, {len(cells)}, 4] (got shape {samples.shape})")
    with open(path, "w") as fh:
        for tt, row in zip(steps.tolist(), samples):
            fh.write("".join("%d %d %d %.12E %.12E %.12E %.12E\n" % (tt, x, y, *map(float, v))
                             for (x, y), v in zip(cells, row)))


def _steady_args(max_steps, check_every, tol, patience) -> tuple[int, int, float, int]:
    """run_until's argument checks (no device needed)."""
    for name, v, lo in (("max_steps", max_steps, 0), ("check_every", check_every, 1), ("patience", patience, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise LbmError(f"run_until: {name} must be an integer (got {v!r})")
        if not lo <= int(v) <= 2147483647:
            raise LbmError(f"run_until: {name} must lie in [{lo}, 2^31) (got {v})")
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)):
        raise LbmError(f"run_until: tol must be a number (got {tol!r})")
    if not float(tol) >= 0.0:
        raise LbmError(f"run_until: tol must be a non-negative number (got {tol})")
    return int(max_steps), int(check_every), float(tol), int(patience)


def _until_history_arg(history, max_steps: int, check_every: int) -> int:
    """run_until_residual's history argument (no device needed): the capacity in rows; None: one per possible check."""
    if history is None:
        return max_steps // check_every
    if isinstance(history, bool) or not isinstance(history, (int, np.integer)):
        raise LbmError(f"run_until: history must be an integer or None (got {history!r})")
    if not 0 <= int(history) <= 2147483647:
        raise LbmError(f"run_until: history must lie in [0, 2^31) (got {history})")
    return min(int(history), max_steps // check_every)


class _BatchResidualSteady(list):
    """Batch.run_until_residual's result: the members' dicts, with the batch's `history` attached once."""
    history = None


def write_animation_frame(path: str, frame: np.ndarray, tt: int) -> None:
    """write_animation_data() (SerialCode/d2q9-bgk.c:802-849): '# nx=%d ny=%d timestep=%d' then one '%.6E' line per
    cell, jj outer / ii inner; `frame` is float32 [ny, nx] |u| with 0 for blocked cells (Engine.frames)."""
    frame = np.asarray(frame, dtype=np.float32)
    if frame.ndim != 2:
        raise LbmError(f"write_animation_frame: frame must be [ny, nx] (got shape {frame.shape})")
    ny, nx = frame.shape
    with open(path, "w") as fh:
        fh.write("# nx=%d ny=%d timestep=%d\n" % (nx, ny, int(tt)))
        fh.write("".join("%.6E\n" % v for v in frame.ravel().tolist()))


def write_final_state(path: str, fields: dict, obstacles: np.ndarray) -> None:
    """'%d %d %.12E %.12E %.12E %.12E %d\\n', jj outer / ii inner (:679-723)."""
    ny, nx = obstacles.shape
    with open(path, "w") as fh:
        for jj in range(ny):
            ux, uy, u, pr, ob = (fields["u_x"][jj], fields["u_y"][jj], fields["u"][jj],
                                 fields["pressure"][jj], obstacles[jj])
            fh.write("".join("%d %d %.12E %.12E %.12E %.12E %d\n" %
                             (ii, jj, ux[ii], uy[ii], u[ii], pr[ii], ob[ii]) for ii in range(nx)))


def write_state_frame(path: str, fields: dict, obstacles: np.ndarray, window) -> None:
    """One field frame in final_state.dat's line format (write_final_state) for the cells of `window` = (x0, y0, nx, ny):
    global 'ii jj', jj outer / ii inner.  `fields` holds the four fields over the window, [window ny, window nx] each
    (one frame of Engine.field_frames); `obstacles` is the whole grid's map."""
    x0, y0, wnx, wny = (int(v) for v in window)
    obstacles = np.asarray(obstacles)
    planes = [np.asarray(fields[k], dtype=np.float32) for k in FIELD_NAMES]
    if any(p.shape != (wny, wnx) for p in planes):
        raise LbmError(f"write_state_frame: every field must be [{wny}, {wnx}] (got {[p.shape for p in planes]})")
    if x0 < 0 or y0 < 0 or y0 + wny > obstacles.shape[0] or x0 + wnx > obstacles.shape[1]:
        raise LbmError(f"write_state_frame: the window {tuple(window)} leaves the {obstacles.shape[1]} x {obstacles.shape[0]} grid")
    with open(path, "w") as fh:
        for j in range(wny):
            ux, uy, u, pr = (p[j] for p in planes)
            ob = obstacles[y0 + j]
            fh.write("".join("%d %d %.12E %.12E %.12E %.12E %d\n" %
                             (x0 + i, y0 + j, ux[i], uy[i], u[i], pr[i], ob[x0 + i]) for i in range(wnx)))


# ------------------------------------------------------------------------------------------------
# the acceptance rule of the reference's check/check.py (:83-99, :136-148)
# ------------------------------------------------------------------------------------------------
def check_rule(ref: np.ndarray, sim: np.ndarray) -> dict:
    """max over entries of 100*(ref-sim)/sim, as check.py computes it (diff/(ref-diff))."""
    ref = np.asarray(ref, dtype=np.float64).ravel()
    sim = np.asarray(sim, dtype=np.float64).ravel()
    if ref.size != sim.size:
        raise LbmError("Different number of steps in av_vels files")
    diff = ref - sim
    with np.errstate(divide="ignore", invalid="ignore"):
        pct = 100.0 * (diff / (ref - diff))
    k = int(np.argmax(np.abs(pct)))
    return {"index": k, "max_diff": float(diff[k]), "max_diff_pcnt": float(pct[k]),
            "sim_val": float(sim[k]), "ref_val": float(ref[k]), "total": float(np.abs(diff).sum())}


def check_passes(ref: np.ndarray, sim: np.ndarray, tolerance_pct: float = 1.0) -> bool:
    d = check_rule(ref, sim)
    return bool(np.isfinite(d["max_diff_pcnt"]) and abs(d["max_diff_pcnt"]) <= tolerance_pct)
