"""Animation frames without a device: the Python twin of the host program's frame writer (write_animation_data,
SerialCode/d2q9-bgk.c:802-849), the frame-step arithmetic the GPU tests use, and Engine.set_frames' argument checks."""
import numpy as np
import pytest


def frame_steps(start, total, every):
    """Global steps tt in [start, total) after which a frame is recorded."""
    return [tt for tt in range(start, total) if tt % every == 0]


def split_calls(calls, every):
    """`calls` (from step 0) cut after every frame step: the lbm_run calls the per-pass paths behave like."""
    out, done = [], 0
    for n in calls:
        end = done + n
        cuts = [tt + 1 for tt in frame_steps(done, end, every)] + [end]
        for c in cuts:
            if c > done:
                out.append(c - done)
                done = c
    return out


def test_frame_steps_and_split_calls():
    assert frame_steps(0, 301, 100) == [0, 100, 200, 300]
    assert frame_steps(130, 431, 100) == [200, 300, 400]
    assert split_calls([301], 100) == [1, 100, 100, 100]
    assert split_calls([50, 251], 100) == [1, 49, 51, 100, 100]
    assert sum(split_calls([57, 203], 25)) == 260


def test_write_animation_frame_matches_the_reference_format(lbm, tmp_path):
    frame = np.array([[0.0, 1.5e-3, np.float32(1e-40)],
                      [np.float32(3.4e38), -0.0, 0.123456789]], dtype=np.float32)
    path = tmp_path / "velocity_magnitude_000100.dat"
    lbm.write_animation_frame(str(path), frame, 100)
    want = ("# nx=3 ny=2 timestep=100\n"
            "0.000000E+00\n"
            "1.500000E-03\n"
            "9.999946E-41\n"
            "3.400000E+38\n"
            "-0.000000E+00\n"
            "1.234568E-01\n")
    assert path.read_text() == want


def test_write_animation_frame_rejects_non_2d(lbm, tmp_path):
    with pytest.raises(lbm.LbmError, match="ny, nx"):
        lbm.write_animation_frame(str(tmp_path / "x.dat"), np.zeros(4, np.float32), 0)


@pytest.mark.parametrize("every,capacity,msg", [(-1, 4, "every"), (10, 0, "capacity"), (1.5, 4, "integer"),
                                                (10, -3, "capacity"), (True, 4, "integer"), (10, 2 ** 31, "capacity")])
def test_set_frames_checks_arguments_without_a_device(lbm, every, capacity, msg):
    with pytest.raises(lbm.LbmError, match=msg):
        lbm._frame_args(every, capacity)
    assert lbm._frame_args(0, 0) == (0, 0)
    assert lbm._frame_args(np.int64(100), 8) == (100, 8)


def test_frames_binding_is_exported(lbm):
    lib = lbm.load_library()
    assert lib.lbm_set_frames.restype is not None and lib.lbm_read_frames.restype is not None
    assert hasattr(lbm.Engine, "set_frames") and hasattr(lbm.Engine, "frames")
    assert issubclass(lbm.BatchMember, lbm.Engine)
