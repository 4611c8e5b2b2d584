"""The scaled sparse kernels with C folded into the costate's scale, on the GPU (csrc/admm_lean.hip.h: FOLD): d_k = c r~_k +
B^' pv_{k+1} with no product by C, 24 fp64 per knot for 25.  Cartpole N = 20 — the only shape the scaled kernels are built for
— with u_bound = 0.5 (the clamp is live), TINYMPC_HIP_GROUP=1; 289 instances are one full workgroup and a ragged wavefront of
33, 64 a single wavefront.  Whether a launch ran a scaled kernel is read back through the test hook tmpc_lean_last_scaled.
  a. 100 fixed iterations: every instance against the fp64 oracle at FP32_TOL (1e-5), residuals included;
  b. fixed-iteration against tolerance-terminated at tolerance 1e-30: the same bits (the sweeps, and so the fold, are shared);
  c. against the unscaled sparse kernel (TINYMPC_HIP_LEAN_UNSCALED=1) at tolerance 1e-3 with a check at every iteration: the
     same iteration counts and solved flags, states and controls within 1e-6;
  d. a single wavefront: as a."""
import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.test_lean_scaled_gpu import FIXED, _oracle_parity, _solve
from tests.util import nrel_batch

pytestmark = pytest.mark.gpu

B = 256 + 33


@pytest.fixture(scope="module")
def cartpole():
    return t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(B, seed=95)


@pytest.fixture(scope="module")
def fixed_folded(hip_lib, cartpole):
    """the fixed-iteration solve, shared by the cases that compare against it"""
    mp = pytest.MonkeyPatch()
    try:
        return _solve(mp, cartpole[0], cartpole[1], FIXED)
    finally:
        mp.undo()


def test_fixed_iterations_against_the_oracle(hip_lib, oracle_built, cartpole, fixed_folded):
    name, scaled, sol, st = fixed_folded
    assert name == "lean<4,1,20>" and scaled == 1
    assert np.abs(sol["controls"]).max() > 0.4                     # (the clamp is live)
    _oracle_parity(oracle_built, cartpole[0], cartpole[1], FIXED, sol, st, "folded, 289 instances")


def test_fixed_equals_live_bit_for_bit(hip_lib, monkeypatch, cartpole, fixed_folded):
    _, _, sol, _ = fixed_folded
    kw = dict(abs_pri_tol=1e-30, abs_dua_tol=1e-30, max_iter=100, check_termination=1)
    name, scaled, lsol, lst = _solve(monkeypatch, cartpole[0], cartpole[1], kw)
    assert name == "lean<4,1,20>" and scaled == 1
    assert np.array_equal(sol["states"], lsol["states"])
    assert np.array_equal(sol["controls"], lsol["controls"])


def test_folded_against_unscaled_at_tolerance(hip_lib, monkeypatch, cartpole):
    prob, x0 = cartpole
    kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1)
    name, s1, sol, st = _solve(monkeypatch, prob, x0, kw)
    uname, s0, usol, ust = _solve(monkeypatch, prob, x0, kw, unscaled=True)
    assert name == "lean<4,1,20>" and uname == "lean<4,1,20>" and s1 == 1 and s0 == 0
    ex, eu = nrel_batch(sol["states"], usol["states"]).max(), nrel_batch(sol["controls"], usol["controls"]).max()
    print(f"tolerance 1e-3: {int((st['iter'] != ust['iter']).sum())} iteration counts differ, iterations "
          f"{st['iter'].min()}..{st['iter'].max()}; states {ex:.3e}, controls {eu:.3e}")
    assert np.array_equal(st["iter"], ust["iter"]) and np.array_equal(st["solved"], ust["solved"])
    assert ex <= 1e-6 and eu <= 1e-6


def test_single_wavefront(hip_lib, oracle_built, monkeypatch):
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(64, seed=96)
    name, scaled, sol, st = _solve(monkeypatch, prob, x0, FIXED)
    assert name == "lean<4,1,20>" and scaled == 1
    _oracle_parity(oracle_built, prob, x0, FIXED, sol, st, "folded, 64 instances")
