"""Per-instance closed-loop metrics, CPU part: the entry points exist (declared in include/tinympc_hip.h, exported by the built
library, bound by the Python mirror, present in the Julia module); tinympc_host_rollout_metrics — csrc/metrics.h compiled for the
host, the text the device kernel compiles — against a numpy fp64 restatement of the rule written here; continuation (3 + 2 steps
into the same accumulators are 5 steps); and the refusals that need no device.

The rule, per step: e = x - xr, v = u - ur in fp64 of the fp32 values; cost_x += sum qw e^2, cost_u += sum rw v^2, peak_err and
final_err from max |e|, x_viol_max from max(x - x_hi, x_lo - x, 0), a step counts as out when any row is strictly outside, as
saturated when any u >= u_hi or <= u_lo, first_viol = 1 + index of the first step out, iters += |it|, maxiter_steps counts it < 0.

Tolerances: slots 0 and 3..10 are counts, maxima and comparisons of exactly representable values — a difference of two widened
fp32 values is one correctly rounded fp64 subtraction on either side — and must be EXACT.  Slots 1, 2 are fp64 sums of at most
37 * 12 non-negative terms, each off by a few ulp and the sum by at most about 450 * 2^-53 = 5e-14 relative in any order:
|delta| <= 1e-12 * max(1, value), a factor of 20 over that (the bound tests/test_noise.py uses).
Every test fails without the feature: neither the symbols nor the helpers exist there."""
import ctypes
import os
import re

import numpy as np
import pytest

import tinympc_julia_amd as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = ("tinympc_set_rollout_metrics", "tinympc_reset_rollout_metrics", "tinympc_rollout_metrics_mode", "tinympc_get_rollout_metrics",
          "tinympc_get_rollout_summary", "tinympc_host_rollout_metrics")
GLOBAL = ("set_rollout_metrics", "reset_rollout_metrics", "get_rollout_metrics", "get_rollout_summary")
NAMES = ("steps", "cost_x", "cost_u", "peak_err", "final_err", "x_viol_max", "x_viol_steps", "first_viol", "u_sat_steps", "iters", "maxiter_steps")
SUMS, EXACT = (1, 2), (0, 3, 4, 5, 6, 7, 8, 9, 10)
SUM_TOL = 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# the rule, restated (vectorised over the steps; nothing of the library in it)
# ---------------------------------------------------------------------------------------------------------------------------
def restated(x, u, it, qw, rw, xr=None, ur=None, x_lo=None, x_hi=None, u_lo=None, u_hi=None, acc=None):
    """x (steps, nx), u (steps, nu), it (steps,) signed; targets like x / u or None; returns the 11 slots, continuing acc"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    u = np.asarray(u, dtype=np.float32).astype(np.float64)
    it = np.asarray(it, dtype=np.int64)
    steps = it.size
    e = x - (0.0 if xr is None else np.asarray(xr, dtype=np.float32).astype(np.float64))
    v = u - (0.0 if ur is None else np.asarray(ur, dtype=np.float32).astype(np.float64))
    err = np.abs(e).max(axis=1) if steps else np.zeros(0)
    viol, out = np.zeros(steps), np.zeros(steps, dtype=bool)
    if x_hi is not None:
        viol, out = np.maximum(viol, (x - x_hi).max(axis=1)), out | (x > x_hi).any(axis=1)
    if x_lo is not None:
        viol, out = np.maximum(viol, (x_lo - x).max(axis=1)), out | (x < x_lo).any(axis=1)
    sat = np.zeros(steps, dtype=bool)
    if u_hi is not None:
        sat |= (u >= u_hi).any(axis=1)
    if u_lo is not None:
        sat |= (u <= u_lo).any(axis=1)
    a = np.zeros(11) if acc is None else np.array(acc, dtype=np.float64)
    had = a[0]
    r = a.copy()
    r[0] = had + steps
    r[1] = a[1] + float((np.asarray(qw) * e * e).sum())
    r[2] = a[2] + float((np.asarray(rw) * v * v).sum())
    if steps:
        r[3] = max(a[3], err.max())
        r[4] = err[-1]
        r[5] = max(a[5], viol.max())
    r[6] = a[6] + out.sum()
    if a[7] == 0.0 and out.any():
        r[7] = had + 1 + int(np.argmax(out))
    r[8] = a[8] + sat.sum()
    r[9] = a[9] + np.abs(it).sum()
    r[10] = a[10] + (it < 0).sum()
    return r


def check_slots(got, want, tag, scale=None):
    """exact slots bit for bit, the two sums within SUM_TOL * max(1, scale or value); arrays (..., 11)"""
    got, want = np.asarray(got), np.asarray(want)
    for k in EXACT:
        assert np.array_equal(got[..., k], want[..., k]), f"{tag}: slot {k} ({NAMES[k]}): {got[..., k]} vs {want[..., k]}"
    for k in SUMS:
        bound = SUM_TOL * np.maximum(1.0, np.abs(want[..., k]) if scale is None else scale[..., k])
        d = np.abs(got[..., k] - want[..., k])
        print(f"{tag}: slot {k} ({NAMES[k]}): worst |delta| / bound = {np.max(d / bound):.3e}")
        assert np.all(d <= bound), f"{tag}: slot {k} ({NAMES[k]}): worst {np.max(d / bound):.3e} of the bound"


def random_log(rng, nx, nu, steps):
    x = rng.normal(0.0, 1.0, (steps, nx)).astype(np.float32)
    u = rng.uniform(-0.6, 0.6, (steps, nu)).astype(np.float32)
    u[rng.uniform(size=u.shape) < 0.2] = np.float32(0.5)        # (some controls exactly on the limit: >= counts them)
    u[rng.uniform(size=u.shape) < 0.1] = np.float32(-0.5)
    it = rng.integers(1, 40, steps).astype(np.int32) * rng.choice(np.array([1, -1], dtype=np.int32), steps)
    xr = rng.normal(0.0, 1.0, (steps, nx)).astype(np.float32)
    ur = rng.normal(0.0, 0.1, (steps, nu)).astype(np.float32)
    cfg = dict(qw=rng.uniform(0.0, 10.0, nx), rw=rng.uniform(0.0, 2.0, nu), x_lo=np.full(nx, -1.0) - rng.uniform(0.0, 0.5, nx),
               x_hi=np.full(nx, 1.0) + rng.uniform(0.0, 0.5, nx), u_lo=np.full(nu, -0.5), u_hi=np.full(nu, 0.5))
    return x, u, it, xr, ur, cfg


# ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_python_binds():
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    for sym in HANDLE + GLOBAL:
        assert re.search(r"\bint %s\(" % sym, header), sym
    assert "#define TMPC_METRIC_COUNT 11" in header
    for name in NAMES:
        assert re.search(r"\b%s\b" % name, header), name
    from tinympc_julia_amd import tinympc
    for sym in HANDLE + GLOBAL:
        assert sym in tinympc.SIGNATURES, sym
    assert tinympc.METRIC_NAMES == NAMES and t.METRIC_NAMES == NAMES
    for name in ("set_rollout_metrics", "reset_rollout_metrics", "rollout_metrics_mode", "get_rollout_metrics", "get_rollout_summary",
                 "host_rollout_metrics"):
        assert hasattr(tinympc.BatchSolver, name), name
    for name in GLOBAL + ("host_rollout_metrics", "summary_dict"):
        assert callable(getattr(t, name)), name
    julia = open(os.path.join(ROOT, "tinympc-julia_amd", "julia", "TinyMPC.jl")).read()
    for name in GLOBAL:
        assert "function %s(" % name in julia, name


def test_built_library_exports_the_entry_points(hip_lib):
    raw = ctypes.CDLL(t.LIB_PATH)
    for sym in HANDLE + GLOBAL:
        assert hasattr(raw, sym), sym
        assert getattr(hip_lib, sym).restype is ctypes.c_int
    # without a solver the global forms fail cleanly, and a null handle is refused
    hip_lib.cleanup_solver()
    buf = np.zeros(44)
    assert hip_lib.reset_rollout_metrics() == -1 and hip_lib.get_rollout_summary(buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -1
    assert b"not initialized" in hip_lib.tinympc_last_error()
    assert hip_lib.set_rollout_metrics(1, None, 0, None, 0, None, None, None, None) == -1
    assert hip_lib.tinympc_set_rollout_metrics(None, 1, None, None, None, None, None, None) == -1
    assert hip_lib.tinympc_rollout_metrics_mode(None) == -1 and hip_lib.tinympc_reset_rollout_metrics(None) == -1


SIDES = [(), ("x_lo",), ("x_hi",), ("u_lo",), ("u_hi",), ("x_lo", "x_hi", "u_lo", "u_hi")]


@pytest.mark.parametrize("targets", [True, False], ids=["targets", "no-targets"])
@pytest.mark.parametrize("steps", [1, 5, 37])
@pytest.mark.parametrize("nx, nu", [(4, 1), (5, 2), (12, 4)])
def test_host_rule_against_the_restatement(hip_lib, nx, nu, steps, targets):
    rng = np.random.default_rng(1000 * nx + 10 * steps + int(targets))
    x, u, it, xr, ur, cfg = random_log(rng, nx, nu, steps)
    if not targets:
        xr = ur = None
    seen = np.zeros(11, dtype=bool)
    for dropped in SIDES:                      # each limit side NULL in turn, none, and all four
        c = {k: (None if k in dropped else v) for k, v in cfg.items()}
        got = t.host_rollout_metrics(x, u, it, xr=xr, ur=ur, **c)
        want = restated(x, u, it, xr=xr, ur=ur, **c)
        check_slots(got, want, f"nx={nx} nu={nu} steps={steps} without {dropped}")
        assert got[0] == steps
        if "x_lo" in dropped and "x_hi" in dropped:
            assert got[5] == 0 and got[6] == 0 and got[7] == 0
        if "u_lo" in dropped and "u_hi" in dropped:
            assert got[8] == 0
        seen |= got > 0
    if steps >= 5:                              # (not vacuous: every slot is non-zero in some configuration)
        assert seen.all(), seen


@pytest.mark.parametrize("nx, nu", [(4, 1), (12, 4)])
def test_three_plus_two_steps_are_five(hip_lib, nx, nu):
    rng = np.random.default_rng(77 + nx)
    x, u, it, xr, ur, cfg = random_log(rng, nx, nu, 5)
    cfg["x_hi"] = np.maximum(cfg["x_hi"], x[:3].max(axis=0))      # the first three steps stay inside ...
    cfg["x_lo"] = np.minimum(cfg["x_lo"], x[:3].min(axis=0))
    x[3, 0] = np.float32(cfg["x_hi"][0] + 1.0)                      # ... and step 3 is the first one out: first_viol = 4, counted across the calls
    whole = t.host_rollout_metrics(x, u, it, xr=xr, ur=ur, **cfg)
    part = t.host_rollout_metrics(x[:3], u[:3], it[:3], xr=xr[:3], ur=ur[:3], **cfg)
    assert part[0] == 3 and part[7] == 0
    both = t.host_rollout_metrics(x[3:], u[3:], it[3:], xr=xr[3:], ur=ur[3:], acc=part, **cfg)
    check_slots(both, whole, f"3 + 2 steps, nx={nx}")
    check_slots(both, restated(x[3:], u[3:], it[3:], xr=xr[3:], ur=ur[3:], acc=restated(x[:3], u[:3], it[:3], xr=xr[:3], ur=ur[:3], **cfg), **cfg),
                f"3 + 2 steps restated, nx={nx}")
    assert both[0] == 5 and both[7] == 4 and both[4] == whole[4]
    # zero steps leave the accumulators alone
    assert np.array_equal(t.host_rollout_metrics(x[:0], u[:0], it[:0], acc=whole, **cfg), whole)


def test_refusals_that_need_no_device(hip_lib):
    rng = np.random.default_rng(5)
    x, u, it, xr, ur, cfg = random_log(rng, 4, 1, 3)
    for bad, word in ((dict(qw=np.array([1.0, -1.0, 1.0, 1.0])), "negative"), (dict(rw=np.array([-0.5])), "negative"),
                      (dict(x_lo=np.array([0.0, 2.0, 0.0, 0.0]), x_hi=np.ones(4)), "x_lo > x_hi"),
                      (dict(u_lo=np.array([1.0]), u_hi=np.array([0.5])), "u_lo > u_hi")):
        with pytest.raises(t.TinyMPCError, match=word):
            t.host_rollout_metrics(x, u, it, **dict(cfg, **bad))
    with pytest.raises(t.TinyMPCError, match="expected 4 values"):
        t.host_rollout_metrics(x, u, it, **dict(cfg, qw=np.ones(3)))
    with pytest.raises(t.TinyMPCError, match="shapes"):
        t.host_rollout_metrics(x, u, it, xr=xr[:2], **cfg)
    dp = ctypes.POINTER(ctypes.c_double)
    acc = np.zeros(11)
    # the raw call: null logs, null weights, null accumulators
    f = hip_lib.tinympc_host_rollout_metrics
    xp, up, ip = x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), u.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), it.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    q, r = cfg["qw"].ctypes.data_as(dp), cfg["rw"].ctypes.data_as(dp)
    assert f(4, 1, 3, xp, up, ip, None, None, q, r, None, None, None, None, acc.ctypes.data_as(dp)) == 0 and acc[0] == 3
    assert f(4, 1, 3, None, up, ip, None, None, q, r, None, None, None, None, acc.ctypes.data_as(dp)) == -1
    assert f(4, 1, 3, xp, up, ip, None, None, None, r, None, None, None, None, acc.ctypes.data_as(dp)) == -1
    assert f(4, 1, 3, xp, up, ip, None, None, q, r, None, None, None, None, None) == -1
    assert f(0, 1, 3, xp, up, ip, None, None, q, r, None, None, None, None, acc.ctypes.data_as(dp)) == -1
    assert acc[0] == 3      # (a refused call writes nothing)


def test_summary_dict():
    s = np.arange(44, dtype=np.float64).reshape(11, 4)
    d = t.summary_dict(s)
    assert tuple(d) == NAMES and d["cost_x"] == dict(sum=4.0, min=5.0, max=6.0, count=7.0) and d["maxiter_steps"]["count"] == 43.0
