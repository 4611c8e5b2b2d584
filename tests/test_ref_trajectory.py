"""Reference trajectories, CPU part: the entry points exist (declared in include/tinympc_hip.h, exported by the built library,
bound by the Python mirror, present in the Julia module), and the window rule as tinympc.ref_window states it in numpy —
x_ref[k] = x_traj[min(cursor + k, L - 1)] — which the GPU part (tests/test_ref_trajectory_gpu.py) and the host-stepped arms of
scripts/trajectory_loop_rate.py share.  Every test fails without the feature: neither the symbols nor the helper exist there."""
import ctypes
import os
import re

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.test_ref_sequence import quadrotor_tracking_refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = ("tinympc_set_ref_trajectory", "tinympc_set_ref_cursor", "tinympc_ref_cursor", "tinympc_ref_trajectory_mode")
GLOBAL = ("set_ref_trajectory", "set_ref_cursor", "ref_cursor")


def test_header_declares_and_python_binds():
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    for sym in HANDLE + GLOBAL:
        assert re.search(r"\bint %s\(" % sym, header), sym
    assert "A sharded solver" in header and "takes no trajectory" in header
    from tinympc_julia_amd import tinympc
    for sym in HANDLE + GLOBAL:
        assert sym in tinympc.SIGNATURES, sym
    for name in ("set_ref_trajectory", "set_ref_cursor", "ref_cursor", "ref_trajectory_mode"):
        assert hasattr(tinympc.BatchSolver, name), name
    for name in GLOBAL + ("ref_window",):
        assert callable(getattr(t, name)), name
    julia = open(os.path.join(ROOT, "tinympc-julia_amd", "julia", "TinyMPC.jl")).read()
    for name in GLOBAL:
        assert "function %s(" % name in julia, name


def test_built_library_exports_the_entry_points(hip_lib):
    raw = ctypes.CDLL(t.LIB_PATH)
    for sym in HANDLE + GLOBAL:
        assert hasattr(raw, sym), sym
        assert getattr(hip_lib, sym).restype is ctypes.c_int      # (bound by load_library)
    # without a solver the global forms fail cleanly
    hip_lib.cleanup_solver()
    assert hip_lib.set_ref_cursor(0) == -1 and hip_lib.ref_cursor() == -1
    assert b"not initialized" in hip_lib.tinympc_last_error()


def test_ref_window_rule():
    rng = np.random.default_rng(0)
    traj = rng.standard_normal((3, 7))
    for cursor in (0, 2, 6, 7, 40):
        w = t.ref_window(traj, cursor, 5)
        assert w.shape == (3, 5) and w.dtype == traj.dtype
        for k in range(5):
            assert np.array_equal(w[:, k], traj[:, min(cursor + k, 6)]), (cursor, k)
    # beyond the end: the last row, whatever the cursor — a one-row trajectory is a constant reference
    assert np.array_equal(t.ref_window(traj, 6, 4), np.repeat(traj[:, 6:7], 4, axis=1))
    assert np.array_equal(t.ref_window(traj, 1000, 4), np.repeat(traj[:, 6:7], 4, axis=1))
    assert np.array_equal(t.ref_window(traj[:, :1], 3, 6), np.repeat(traj[:, :1], 6, axis=1))
    # per instance: every instance's own window; a copy, not a view
    traj3 = rng.standard_normal((2, 4, 5)).astype(np.float32)
    w3 = t.ref_window(traj3, 2, 6)
    assert w3.shape == (2, 6, 5) and w3.dtype == np.float32 and w3.flags.f_contiguous
    for b in range(5):
        assert np.array_equal(w3[:, :, b], t.ref_window(traj3[:, :, b], 2, 6))
    w3[:] = 0.0
    assert np.abs(traj3).min() > 0.0
    assert t.ref_window(traj, 3, 0).shape == (3, 0)
    for bad in (lambda: t.ref_window(traj[:, :0], 0, 3), lambda: t.ref_window(traj, -1, 3), lambda: t.ref_window(traj[0], 0, 3)):
        with pytest.raises(ValueError):
            bad()


def test_windows_of_one_trajectory_are_the_shifted_sequence():
    """tests/test_ref_sequence.py builds the quadrotor tracking references step by step, every step's set shifted by one knot:
    that sequence is the windows of ONE trajectory of N + steps - 1 rows — step 0's knots, then the last knot of every later
    step — at the cursors 0 .. steps-1, to the bit"""
    N, steps = 10, 7
    xs, us = quadrotor_tracking_refs(N, steps)
    x_traj = np.concatenate([xs[:, :, 0], xs[:, -1, 1:]], axis=1)
    u_traj = np.concatenate([us[:, :, 0], us[:, -1, 1:]], axis=1)
    assert x_traj.shape == (12, N + steps - 1) and u_traj.shape == (4, N + steps - 2)
    assert np.any(np.diff(x_traj[0]) != 0.0), "the reference does not move"
    seq_x = np.stack([t.ref_window(x_traj, c, N) for c in range(steps)], axis=2)
    seq_u = np.stack([t.ref_window(u_traj, c, N - 1) for c in range(steps)], axis=2)
    assert np.array_equal(seq_x, xs) and np.array_equal(seq_u, us)
    # a trajectory cut short holds its last row: from the step at which the window passes the end on, the sequences differ
    # exactly in the knots past the end
    short = np.stack([t.ref_window(x_traj[:, :N + 2], c, N) for c in range(steps)], axis=2)
    assert np.array_equal(short[:, :, :3], xs[:, :, :3]) and not np.array_equal(short[:, :, 3], xs[:, :, 3])
    assert np.array_equal(short[:, -1, 6], x_traj[:, N + 1])
