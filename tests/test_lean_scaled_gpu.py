"""The lean kernel's scaled sparse form on the GPU (csrc/admm_lean.hip.h: SCL; csrc/linst_4_1_20_scaled.hip): the sweeps on the
diagonally scaled cartpole model, 25 fp64 per knot for 27.  Cartpole N = 20 with u_bound = 0.5, 20 480 + 193 instances (81
workgroups, the last one ragged: the 512-register kernels), TINYMPC_HIP_GROUP=1.  Whether a launch ran a scaled kernel is
read back through the test hook tmpc_lean_last_scaled.
  1. the fixed-iteration solve: every instance against the fp64 oracle at FP32_TOL, residuals included;
  2. fixed-iteration against tolerance-terminated at tolerance 1e-30: the same bits (the sweeps are shared);
  3. against the unscaled sparse kernels (TINYMPC_HIP_LEAN_UNSCALED=1): 1e-6, the bound the sparse and the dense form are held
     to; at tolerance 1e-3 the same iteration counts and solved flags;
  4. a model with a chosen entry zeroed (A01 = 0) keeps the unscaled kernel and the oracle parity.
The 256-register (two wavefronts per SIMD) scaled kernel is not built — it spills — so there is no case at 65 536 + 193."""
import ctypes
import os

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.util import FP32_TOL, nrel_batch, parity_every_instance

pytestmark = pytest.mark.gpu

B = 20480 + 193
FIXED = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=100, check_termination=1)


def _scaled(bs):
    f = ctypes.CDLL(t.LIB_PATH).tmpc_lean_last_scaled
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p]
    return f(bs.h)


def _solve(monkeypatch, prob, x0, kw, unscaled=False):
    monkeypatch.setenv("TINYMPC_HIP_GROUP", "1")
    if unscaled:
        monkeypatch.setenv("TINYMPC_HIP_LEAN_UNSCALED", "1")
    else:
        monkeypatch.delenv("TINYMPC_HIP_LEAN_UNSCALED", raising=False)
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=x0.shape[1])
    bs.update_settings(**kw)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(False)
    bs.set_x0(x0)
    bs.solve()
    out = (bs.last_launch_name, _scaled(bs), bs.get_solution(), bs.get_status())
    bs.close()
    monkeypatch.delenv("TINYMPC_HIP_LEAN_UNSCALED", raising=False)
    return out


def _oracle_parity(oracle_built, prob, x0, kw, sol, st, tag):
    ref = oracle_built.solve_batch("orc64", prob, x0, nthreads=min(16, len(os.sched_getaffinity(0))), **kw)

    def make(b=None):
        o = oracle_built.CpuSolver("orc64", prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
        o.update_settings(**kw)
        o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        return o
    parity_every_instance(sol, st, ref, make, x0, kw, prob.rho, min_same=1.0, tag=tag)
    eq = st["iter"] == ref["iter"]
    dres = np.abs(st["residuals"][eq] - ref["res"][eq]).max(axis=0) / np.maximum(1.0, np.abs(ref["res"][eq]).max(axis=0))
    print(f"{tag}: residuals (pri_x, dua_x, pri_u, dua_u) off by {dres}")
    assert dres.max() <= FP32_TOL, f"{tag}: residuals (pri_x, dua_x, pri_u, dua_u) off by {dres}"


@pytest.fixture(scope="module")
def cartpole():
    return t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(B, seed=93)


@pytest.fixture(scope="module")
def fixed_scaled(hip_lib, cartpole):
    """the scaled fixed-iteration solve, shared by the cases that compare against it"""
    mp = pytest.MonkeyPatch()
    try:
        return _solve(mp, cartpole[0], cartpole[1], FIXED)
    finally:
        mp.undo()


def test_fixed_iterations_against_the_oracle(hip_lib, oracle_built, cartpole, fixed_scaled):
    name, scaled, sol, st = fixed_scaled
    assert name == "lean<4,1,20>" and scaled == 1
    _oracle_parity(oracle_built, cartpole[0], cartpole[1], FIXED, sol, st, "scaled")


def test_fixed_equals_live_bit_for_bit(hip_lib, monkeypatch, cartpole, fixed_scaled):
    _, _, sol, _ = fixed_scaled
    kw = dict(abs_pri_tol=1e-30, abs_dua_tol=1e-30, max_iter=100, check_termination=1)
    name, scaled, lsol, lst = _solve(monkeypatch, cartpole[0], cartpole[1], kw)
    assert name == "lean<4,1,20>" and scaled == 1
    print("iterations of the tolerance-terminated solve:", np.unique(lst["iter"]))
    assert np.array_equal(sol["states"], lsol["states"])
    assert np.array_equal(sol["controls"], lsol["controls"])


def test_scaled_against_unscaled(hip_lib, monkeypatch, cartpole, fixed_scaled):
    prob, x0 = cartpole
    _, _, sol, st = fixed_scaled
    uname, uscaled, usol, ust = _solve(monkeypatch, prob, x0, FIXED, unscaled=True)
    assert uname == "lean<4,1,20>" and uscaled == 0
    ex, eu = nrel_batch(sol["states"], usol["states"]).max(), nrel_batch(sol["controls"], usol["controls"]).max()
    same = np.mean(sol["states"] == usol["states"]), np.mean(sol["controls"] == usol["controls"])
    print(f"scaled against unscaled: states {ex:.3e} ({same[0]:.4f} bit-identical), controls {eu:.3e} ({same[1]:.4f} bit-identical)")
    assert ex <= 1e-6 and eu <= 1e-6
    kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1)
    _, s1, lsol, lst = _solve(monkeypatch, prob, x0, kw)
    _, s0, lusol, lust = _solve(monkeypatch, prob, x0, kw, unscaled=True)
    assert s1 == 1 and s0 == 0
    print(f"tolerance 1e-3: {int((lst['iter'] != lust['iter']).sum())} iteration counts differ, iterations {lst['iter'].min()}..{lst['iter'].max()}")
    assert np.array_equal(lst["iter"], lust["iter"]) and np.array_equal(lst["solved"], lust["solved"])
    assert nrel_batch(lsol["states"], lusol["states"]).max() <= 1e-6 and nrel_batch(lsol["controls"], lusol["controls"]).max() <= 1e-6


def test_chosen_entry_zero_keeps_the_unscaled_kernel(hip_lib, oracle_built, monkeypatch):
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(B, seed=94)
    prob.A = prob.A.copy()
    prob.A[0, 1] = 0.0
    name, scaled, sol, st = _solve(monkeypatch, prob, x0, FIXED)
    assert name == "lean<4,1,20>" and scaled == 0
    _oracle_parity(oracle_built, prob, x0, FIXED, sol, st, "A01 = 0")
