"""The ledger of what every entry point of include/lbm_hip.h that takes an lbm_ctx* or an lbm_batch* does once a resident
launch of that owner has given up (the rule stands at lbm_sync in the header): REFUSED -- it fails with the words below
and touches nothing -- or ALLOWED.  tests/test_give_up_calls.py holds this table against the header's prototypes without a
device, so a new entry point fails there until someone decides what it does after a give-up; tests/test_gpu_give_up.py makes
every call of the table on a failed owner.  The lbm_double_* family has no resident kernel and is not listed.

An entry is (verdict, call[, "ring"]): call(o) makes the call on o, an Engine (a BatchMember too) for the lbm_ctx* entries
and a Batch for the lbm_batch* ones, through the binding's method where it has one, else through ctypes (raw); a failure
is an LbmError with the library's message.  Every call's own arguments are in order for the 128 x 16 lattice of the GPU
suite, so on a healthy owner none of them is refused for its arguments.  "ring": a ring reader, whose *n_read a refusal
sets to 0 (ring_read makes that call)."""
import ctypes

import numpy as np

REFUSED, ALLOWED = "refused", "allowed"

# the first report, from the call that sees the status word (lbm_sync's words since the resident kernel exists) ...
FIRST_REPORT = "the resident kernel gave up waiting for a neighbouring band after 200 ms"
# ... and every later call on the failed owner, word for word
LATER_REFUSAL = ("{name}: an earlier launch of the resident kernel gave up: the lattice and the records of this context or "
                 "batch are invalid, and it stays failed until it is destroyed")

# the six that still work, and no others
ALLOWED_CALLS = {"lbm_destroy", "lbm_destroy_batch", "lbm_get_info", "lbm_batch_get_info", "lbm_batch_member", "lbm_rccl_info"}


def refusal(name):
    return LATER_REFUSAL.format(name=name)


def raw(o, name, *args):
    """the library's `name` on o's handle; raises as the binding does"""
    from conftest import load_package
    if getattr(o.lib, name)(o.handle, *args) != 0:
        raise load_package().LbmError(o.lib.lbm_last_error().decode())


def batch_member_handle(o):
    """lbm_batch_member itself (Batch.member keeps the handles it has fetched)"""
    from conftest import load_package
    h = o.lib.lbm_batch_member(o.handle, len(o) - 1)
    if not h:
        raise load_package().LbmError(o.lib.lbm_last_error().decode())
    return h


def ring_read(o, name):
    """(status, *n_read, the first word of out) of the ring reader `name` asked for four records into a buffer of sentinels"""
    n, steps = ctypes.c_int(-7), (ctypes.c_int * 4)(*([-7] * 4))
    out = np.full(1 << 16, -7.0, dtype=np.float64)
    status = getattr(o.lib, name)(o.handle, 4, out.ctypes.data, steps, ctypes.byref(n))
    return status, n.value, float(out[0]), steps[0]


def _tracers(o):
    lead = (len(o),) if hasattr(o, "member") else ()
    return np.full(lead + (1, 2), 1.5)


CTX_CALLS = {
    "lbm_rccl_info": (ALLOWED, lambda o: o.rccl_info()),
    "lbm_destroy": (ALLOWED, lambda o: o.close()),
    "lbm_get_info": (ALLOWED, lambda o: o.info()),
    "lbm_set_halo_mode": (REFUSED, lambda o: o.set_halo_mode("sync")),
    "lbm_read_halo_log": (REFUSED, lambda o: o.halo_log(1)),
    "lbm_run": (REFUSED, lambda o: o.run(3)),
    "lbm_sync": (REFUSED, lambda o: o.sync()),
    "lbm_run_timed": (REFUSED, lambda o: o.run_timed(3)),
    "lbm_read_av_vels": (REFUSED, lambda o: o.av_vels(1)),
    "lbm_read_cells": (REFUSED, lambda o: o.cells()),
    "lbm_read_final_state": (REFUSED, lambda o: o.final_state()),
    "lbm_av_velocity": (REFUSED, lambda o: o.av_velocity()),
    "lbm_total_density": (REFUSED, lambda o: o.total_density()),
    "lbm_calc_reynolds": (REFUSED, lambda o: o.reynolds()),
    "lbm_set_frames": (REFUSED, lambda o: o.set_frames(1, 4)),
    "lbm_read_frames": (REFUSED, lambda o: o.frames(), "ring"),
    "lbm_set_probes": (REFUSED, lambda o: o.set_probes([(1, 1)], 1, 4)),
    "lbm_read_probes": (REFUSED, lambda o: o.probes(), "ring"),
    "lbm_set_mean": (REFUSED, lambda o: o.set_mean(1)),
    "lbm_read_mean": (REFUSED, lambda o: o.mean_sums()),
    "lbm_set_mean_order": (REFUSED, lambda o: o.set_mean_order(1, 2)),
    "lbm_read_mean2": (REFUSED, lambda o: o.moment_sums()),
    "lbm_set_field_frames": (REFUSED, lambda o: o.set_field_frames(1, 4)),
    "lbm_read_field_frames": (REFUSED, lambda o: o.field_frames(), "ring"),
    "lbm_set_forces": (REFUSED, lambda o: o.set_forces(1, 4)),
    "lbm_read_forces": (REFUSED, lambda o: o.forces(), "ring"),
    "lbm_forces_links": (REFUSED, lambda o: o.force_links()),
    "lbm_run_until": (REFUSED, lambda o: raw(o, "lbm_run_until", 8, 4, ctypes.c_double(0.0), 1, ctypes.byref(_steady(o)))),
    "lbm_set_stats": (REFUSED, lambda o: o.set_stats(1, 4)),
    "lbm_read_stats": (REFUSED, lambda o: o.stats(), "ring"),
    "lbm_set_residual": (REFUSED, lambda o: o.set_residual(1, 4)),
    "lbm_read_residual": (REFUSED, lambda o: o.residuals(), "ring"),
    "lbm_run_until_residual": (REFUSED, lambda o: raw(o, "lbm_run_until_residual", 8, 4, ctypes.c_double(0.0), 1,
                                                      ctypes.byref(_residual_steady(o)), None, 0)),
    "lbm_set_profiles": (REFUSED, lambda o: o.set_profiles(1, 4)),
    "lbm_read_profiles": (REFUSED, lambda o: o.profiles(), "ring"),
    "lbm_read_coarse": (REFUSED, lambda o: o.coarse(4)),
    "lbm_set_coarse_frames": (REFUSED, lambda o: o.set_coarse_frames(1, 4, 4)),
    "lbm_read_coarse_frames": (REFUSED, lambda o: o.coarse_frames(), "ring"),
    "lbm_read_vorticity": (REFUSED, lambda o: o.vorticity()),
    "lbm_set_enstrophy": (REFUSED, lambda o: o.set_enstrophy(1, 4)),
    "lbm_read_enstrophy": (REFUSED, lambda o: o.enstrophy(), "ring"),
    "lbm_read_stress": (REFUSED, lambda o: o.stress()),
    "lbm_set_stress": (REFUSED, lambda o: o.set_stress(1, 4)),
    "lbm_read_stress_rows": (REFUSED, lambda o: o.stress_rows(), "ring"),
    "lbm_read_psi": (REFUSED, lambda o: o.psi()),
    "lbm_set_psi": (REFUSED, lambda o: o.set_psi(1, 4)),
    "lbm_read_psi_rows": (REFUSED, lambda o: o.psi_rows(), "ring"),
    "lbm_set_tracers": (REFUSED, lambda o: o.set_tracers(_tracers(o), 1, 4)),
    "lbm_read_tracers": (REFUSED, lambda o: o.tracer_rows(), "ring"),
    "lbm_tracers_now": (REFUSED, lambda o: o.tracers()),
}

BATCH_CALLS = {
    "lbm_batch_member": (ALLOWED, batch_member_handle),
    "lbm_batch_run": (REFUSED, lambda o: o.run(3)),
    "lbm_batch_run_until": (REFUSED, lambda o: o.run_until(8, 4, 0.0, 1)),
    "lbm_batch_sync": (REFUSED, lambda o: o.sync()),
    "lbm_batch_get_info": (ALLOWED, lambda o: o.info()),
    "lbm_destroy_batch": (ALLOWED, lambda o: o.close()),
    "lbm_batch_set_forces": (REFUSED, lambda o: o.set_forces(1, 4)),
    "lbm_batch_read_forces": (REFUSED, lambda o: o.forces(), "ring"),
    "lbm_batch_forces_links": (REFUSED, lambda o: o.force_links()),
    "lbm_batch_set_stats": (REFUSED, lambda o: o.set_stats(1, 4)),
    "lbm_batch_read_stats": (REFUSED, lambda o: o.stats(), "ring"),
    "lbm_batch_set_residual": (REFUSED, lambda o: o.set_residual(1, 4)),
    "lbm_batch_read_residual": (REFUSED, lambda o: o.residuals(), "ring"),
    "lbm_batch_run_until_residual": (REFUSED, lambda o: o.run_until_residual(8, 4, 0.0, 1)),
    "lbm_batch_set_profiles": (REFUSED, lambda o: o.set_profiles(1, 4)),
    "lbm_batch_read_profiles": (REFUSED, lambda o: o.profiles(), "ring"),
    "lbm_batch_set_coarse_frames": (REFUSED, lambda o: o.set_coarse_frames(1, 4, 4)),
    "lbm_batch_read_coarse_frames": (REFUSED, lambda o: o.coarse_frames(), "ring"),
    "lbm_batch_set_enstrophy": (REFUSED, lambda o: o.set_enstrophy(1, 4)),
    "lbm_batch_read_enstrophy": (REFUSED, lambda o: o.enstrophy(), "ring"),
    "lbm_batch_set_stress": (REFUSED, lambda o: o.set_stress(1, 4)),
    "lbm_batch_read_stress_rows": (REFUSED, lambda o: o.stress_rows(), "ring"),
    "lbm_batch_set_psi": (REFUSED, lambda o: o.set_psi(1, 4)),
    "lbm_batch_read_psi_rows": (REFUSED, lambda o: o.psi_rows(), "ring"),
    "lbm_batch_set_tracers": (REFUSED, lambda o: o.set_tracers(_tracers(o), 1, 4)),
    "lbm_batch_read_tracers": (REFUSED, lambda o: o.tracer_rows(), "ring"),
    "lbm_batch_tracers_now": (REFUSED, lambda o: o.tracers()),
}


# lbm_run_until and lbm_run_until_residual through ctypes: a BatchMember's methods of those names never reach the library
def _steady(o):
    from conftest import load_package
    return load_package()._CSteadyResult()


def _residual_steady(o):
    from conftest import load_package
    return load_package()._CResidualSteadyResult()


def refused(calls):
    """[(name, call)] of the table's refused entries"""
    return [(name, entry[1]) for name, entry in calls.items() if entry[0] == REFUSED]


def ring_readers(calls):
    return [name for name, entry in calls.items() if len(entry) > 2 and entry[2] == "ring"]
