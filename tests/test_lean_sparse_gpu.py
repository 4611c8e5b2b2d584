"""The lean kernel's sparse form (csrc/admm_lean.hip.h, SP != 0): the sweeps on the model's own sparse A and B in the plain
coordinates.  Every instance against the fp64 oracle at FP32_TOL, residuals included, with the form the launch took read
back through the test hook tmpc_lean_last_form; the same inputs on the dense sweeps (TINYMPC_HIP_LEAN_DENSE=1) give the same
iteration counts and solved flags and states / controls within 1e-6.  (At tolerance 1e-30 an instance stops where its
residuals are exactly zero — a fixed point of the fp64 rollout to the last bit, which the two groupings reach at different
iterations: there the counts may differ, the solutions may not.)  Models inside the built-in cartpole pattern take the
sparse kernels; a unit that is not exactly 1 or a nonzero outside the pattern keeps the dense form."""
import ctypes
import os

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.util import FP32_TOL, nrel_batch, parity_every_instance

pytestmark = pytest.mark.gpu

LF_PLAIN, LF_HB, LF_SPARSE = 1, 2, 3
FIXED = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=100, check_termination=1)


def _form(bs):
    lib = ctypes.CDLL(t.LIB_PATH)
    f = lib.tmpc_lean_last_form
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                  ctypes.POINTER(ctypes.c_int)]
    sp, cs, cd, form = ctypes.c_ulonglong(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert f(bs.h, ctypes.byref(sp), ctypes.byref(cs), ctypes.byref(cd), ctypes.byref(form)) == 0
    return form.value, sp.value, cs.value, cd.value


def _solve(prob, x0, kw, monkeypatch, dense=False, state_bound=None):
    if dense:
        monkeypatch.setenv("TINYMPC_HIP_LEAN_DENSE", "1")
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=x0.shape[1])
    bs.update_settings(**kw)
    xmin, xmax = prob.x_min, prob.x_max
    if state_bound is not None:
        xmin, xmax = np.full_like(prob.x_min, -state_bound), np.full_like(prob.x_max, state_bound)
    bs.set_bound_constraints(xmin, xmax, prob.u_min, prob.u_max)
    bs.set_warm_start(False)
    bs.set_x0(x0)
    bs.solve()
    out = (bs.last_launch_name, _form(bs), bs.get_solution(), bs.get_status())
    bs.close()
    if dense:
        monkeypatch.delenv("TINYMPC_HIP_LEAN_DENSE")
    return out


def _check(oracle_built, monkeypatch, prob, x0, kw, form, dense_form, state_bound=None, tag=""):
    name, (f, _, cs, cd), sol, st = _solve(prob, x0, kw, monkeypatch, state_bound=state_bound)
    assert name == f"lean<4,1,{prob.N}>"
    assert f == form, (tag, f, cs, cd)
    if form == LF_SPARSE:
        assert cs < cd
    p = prob
    if state_bound is not None:
        p = t.problems.Problem(prob.name, prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
        p.x_min, p.x_max = np.full_like(prob.x_min, -state_bound), np.full_like(prob.x_max, state_bound)
        p.u_min, p.u_max = prob.u_min, prob.u_max
    ref = oracle_built.solve_batch("orc64", p, x0, nthreads=min(16, len(os.sched_getaffinity(0))), **kw)

    def make(b=None):
        o = oracle_built.CpuSolver("orc64", p.A, p.B, p.Q, p.R, p.rho, p.N)
        o.update_settings(**kw)
        o.set_bound_constraints(p.x_min, p.x_max, p.u_min, p.u_max)
        return o
    # (fp32 state against the fp64 oracle: a residual within rounding of the tolerance may stop an instance one check apart —
    # every such instance is checked against the oracle run with the GPU's exit imposed.  At 1e-30 an instance stops at its
    # exact fixed point, which the fp32 state reaches many iterations before the fp64 oracle: the solutions are compared
    # directly, instance by instance)
    live = kw["abs_pri_tol"] > 0
    zero_tol = live and kw["abs_pri_tol"] < 1e-20
    if zero_tol:
        for key, r in (("states", ref["x"]), ("controls", ref["u"])):
            err = np.abs(sol[key] - r).max(axis=(0, 1)) / np.maximum(np.abs(r).max(axis=(0, 1)), 1e-30)
            assert err.max() <= FP32_TOL, f"{tag}: {key} off by {err.max():.3e} (instance {int(err.argmax())})"
    else:
        parity_every_instance(sol, st, ref, make, x0, kw, p.rho, min_same=0.97 if live else 1.0, tag=tag)
    eq = st["iter"] == ref["iter"]
    dres = np.abs(st["residuals"][eq] - ref["res"][eq]).max(axis=0) / np.maximum(1.0, np.abs(ref["res"][eq]).max(axis=0))
    assert dres.max() <= FP32_TOL, f"{tag}: residuals (pri_x, dua_x, pri_u, dua_u) off by {dres}"
    # the same inputs on the dense sweeps
    dname, (df, _, _, _), dsol, dst = _solve(prob, x0, kw, monkeypatch, dense=True, state_bound=state_bound)
    assert dname == name and df == dense_form, (tag, df)
    if not zero_tol:
        assert np.array_equal(st["iter"], dst["iter"]) and np.array_equal(st["solved"], dst["solved"])
    assert nrel_batch(sol["states"], dsol["states"]).max() <= 1e-6
    assert nrel_batch(sol["controls"], dsol["controls"]).max() <= 1e-6


def test_headline(hip_lib, oracle_built, monkeypatch):
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(65536, seed=61)
    _check(oracle_built, monkeypatch, prob, x0, FIXED, LF_SPARSE, LF_HB, tag="headline")


@pytest.mark.parametrize("tol", [1e-30, 1e-3])
def test_check_live(hip_lib, oracle_built, monkeypatch, tol):
    kw = dict(abs_pri_tol=tol, abs_dua_tol=tol, max_iter=100, check_termination=1)
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(20480, seed=62)
    _check(oracle_built, monkeypatch, prob, x0, kw, LF_SPARSE, LF_PLAIN, tag=f"live {tol}")


def test_state_bound(hip_lib, oracle_built, monkeypatch):
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(20480, seed=63)
    _check(oracle_built, monkeypatch, prob, x0, FIXED, LF_SPARSE, LF_PLAIN, state_bound=0.6, tag="state bound")


def test_two_wavefronts_per_simd(hip_lib, oracle_built, monkeypatch):
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(131072, seed=64)
    _check(oracle_built, monkeypatch, prob, x0, FIXED, LF_SPARSE, LF_PLAIN, tag="two-wave")


def test_zero_inside_the_pattern(hip_lib, oracle_built, monkeypatch):
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(20480, seed=65)
    prob.A = prob.A.copy()
    prob.A[0, 1] = 0.0
    prob.A[2, 3] = 0.012
    _check(oracle_built, monkeypatch, prob, x0, FIXED, LF_SPARSE, LF_HB, tag="zero inside")


def test_unit_not_exact_keeps_dense(hip_lib, oracle_built, monkeypatch):
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(20480, seed=66)
    prob.A = prob.A.copy()
    prob.A[0, 0] = 1.0 + 1e-9
    _check(oracle_built, monkeypatch, prob, x0, FIXED, LF_HB, LF_HB, tag="1 + 1e-9")


def test_nonzero_outside_the_pattern_keeps_dense(hip_lib, oracle_built, monkeypatch):
    monkeypatch.setenv("TINYMPC_HIP_NO_JIT", "1")
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(20480, seed=67)
    prob.A = prob.A.copy()
    prob.A[3, 0] = 0.002
    _check(oracle_built, monkeypatch, prob, x0, FIXED, LF_HB, LF_HB, tag="outside")
