"""The lean kernel's in-kernel closed loop (csrc/admm_lean.hip.h, MPC = true) behind TINYMPC_HIP_LEAN_LOOP=1 beside
TINYMPC_HIP_LEAN_WS=1: mpc_rollout(steps) of the one-lane-per-instance cartpole entry as ONE launch of "lean<4,1,20>" that
keeps every lane's workspace on chip between the steps, instead of the chain of `steps` workspace-carrying launches and
plant updates (tests/test_lean_ws_gpu.py::test_mpc_rollout_chain) whose arithmetic it repeats step by step.
 * routing by the two switches, read back through the test hook tmpc_last_rollout_launches (solve-kernel launches of the last
   mpc_rollout: `steps` for a chain, 1 for any in-kernel loop, -1 before any rollout);
 * the loop against the fp64 oracle loop on a sample (log, last solution, final workspace) and against the chain on every
   instance — check_termination 1 and 10, full and ragged batch, with and without a state bound;
 * the instances of a wavefront do not leave a step together: iteration counts differ within wavefronts, and with
   check_termination 10 converged and max_iter exits mix at iteration 10 — every lane keeps the workspace of its own exit;
 * no cross-talk between the lanes of a wavefront or between wavefronts;
 * an exit at iteration 1 (the loaded v, z, d handed on untouched), 60 steps;
 * one and two steps, a host-stepped solve behind the loop, a second loop, shared references, per-knot input bounds;
 * what keeps the chain (a reference sequence) or the quad kernel (a horizon beyond the LDS budget); another horizon through
   specialisation.
Limits: FP32_TOL for logs and solutions, test_lean_ws_gpu's 2e-5 (d, z, v) / 4e-5 (g, y) of max(|ref|, 1e-2) for the workspace,
at least 0.9 of a sample on the oracle's own iteration counts and of the batch on the chain's (the floor
test_mpc_rollout_chain holds the chain to against the quad kernel's loop)."""
import ctypes
import math

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.test_lean_ws_gpu import (B_G1, B_RAGGED, LEAN, QUAD, WS_KEYS, _cartpole, _lim, _rollout_vs_oracle, _solver,
                                    jit_on)  # noqa: F401  (jit_on: a fixture)
from tests.util import FP32_TOL, nrel_batch

pytestmark = pytest.mark.gpu

STEPS = 15


def _switches(monkeypatch, ws, loop):
    for name, on in (("TINYMPC_HIP_LEAN_WS", ws), ("TINYMPC_HIP_LEAN_LOOP", loop)):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)


def _launches(bs):
    f = ctypes.CDLL(t.LIB_PATH).tmpc_last_rollout_launches
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p]
    return f(bs.h)


def _kw(ct):
    return dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=10, check_termination=ct)


def _rollout(monkeypatch, prob, B, kw, x0, steps, loop, xref=None, name=LEAN):
    """one mpc_rollout with TINYMPC_HIP_LEAN_WS and, for `loop`, TINYMPC_HIP_LEAN_LOOP: the solver (left open) and what it left"""
    _switches(monkeypatch, True, loop)
    bs = _solver(prob, B, kw, xref=xref)
    bs.set_x0(x0)
    assert _launches(bs) == -1
    log = bs.mpc_rollout(steps)
    assert bs.last_launch_name.startswith(name), bs.last_launch_name
    assert _launches(bs) == (1 if loop else steps), _launches(bs)
    return dict(bs=bs, log=log, sol=bs.get_solution(), st=bs.get_status(), ws=bs.get_workspace(), status=bs.solve_status())


def _same_as_chain(a, c, tag, floor=0.9):
    """loop `a` against chain `c` on every instance: (iter, solved) of all steps agree on at least `floor` of the batch (the
    share is printed and returned); on those instances log, last solution and workspace agree, and the status is equal"""
    la, lc = a["log"], c["log"]
    agree = np.all((la["iter"] == lc["iter"]) & (la["solved"] == lc["solved"]), axis=0)
    agree &= (a["st"]["iter"] == c["st"]["iter"]) & (a["st"]["solved"] == c["st"]["solved"])
    print(f"{tag}: loop and chain agree on the iteration counts of all steps on {agree.mean():.5f} of the batch")
    assert agree.mean() >= floor, (tag, agree.mean())
    den_u, den_x = np.abs(lc["u"]).max(axis=(0, 1)), np.abs(lc["x"]).max(axis=(0, 1))
    eu = (np.abs(la["u"] - lc["u"]).max(axis=(0, 1)) / den_u)[agree].max()
    ex = (np.abs(la["x"] - lc["x"]).max(axis=(0, 1)) / den_x)[agree].max()
    sx = nrel_batch(a["sol"]["states"], c["sol"]["states"])[agree].max()
    su = nrel_batch(a["sol"]["controls"], c["sol"]["controls"])[agree].max()
    print(f"{tag}: worst differences on them: log u {eu:.2e} x {ex:.2e}, last solution x {sx:.2e} u {su:.2e}")
    assert max(eu, ex, sx, su) <= FP32_TOL, (tag, eu, ex, sx, su)
    for key in WS_KEYS:
        scale = max(np.abs(c["ws"][key]).max(), 1e-2)
        err = np.abs(a["ws"][key] - c["ws"][key])[:, :, agree].max()
        assert err <= _lim(key) * scale, (tag, key, err / scale)
    assert a["status"] == c["status"] and a["log"]["status"] == c["log"]["status"], (tag, a["status"], c["status"])
    return agree.mean()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. routing
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws,loop,name,launches", [(False, False, QUAD, 1), (True, False, LEAN, 5), (True, True, LEAN, 1), (False, True, QUAD, 1)],
                         ids=["none", "ws", "ws+loop", "loop_alone"])
def test_routing(hip_lib, monkeypatch, ws, loop, name, launches):
    """the loop needs both switches; a plain solve() goes where it goes without TINYMPC_HIP_LEAN_LOOP"""
    _switches(monkeypatch, ws, loop)
    prob, x0 = _cartpole(u_bound=0.8), t.problems.cartpole_x0(B_G1, seed=31)
    bs = _solver(prob, B_G1, _kw(1))
    bs.set_x0(x0)
    assert _launches(bs) == -1
    bs.solve()
    assert bs.kernel_name == QUAD and bs.last_launch_name == name
    bs.mpc_rollout(5)
    assert bs.kernel_name == QUAD and bs.last_launch_name == name, bs.last_launch_name
    assert _launches(bs) == launches, _launches(bs)
    bs.solve()
    assert bs.last_launch_name == name
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2.-4. the loop against the oracle and against the chain
# ---------------------------------------------------------------------------------------------------------------------------
CASES = [(B_G1, 1, False), (B_G1, 10, False), (B_G1, 1, True), (B_G1, 10, True), (B_RAGGED, 1, False), (B_RAGGED, 10, True)]
CASE_IDS = [f"B{B}-ct{ct}-{'state_bound' if sb else 'free'}" for B, ct, sb in CASES]
_RUNS = {}


def _run(monkeypatch, B, ct, sb, loop):
    key = (B, ct, sb, loop)
    if key not in _RUNS:
        prob, x0 = _cartpole(sb, u_bound=0.8), t.problems.cartpole_x0(B, seed=31)
        _RUNS[key] = _rollout(monkeypatch, prob, B, _kw(ct), x0, STEPS, loop)
    return _RUNS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_runs():
    yield
    for r in _RUNS.values():
        r["bs"].close()
    _RUNS.clear()


def _sample(B):
    if B == B_RAGGED:                                            # ... with the whole ragged wavefront
        return np.r_[0:24, 12000:12012, 20480:B_RAGGED]
    return np.r_[0:24, 12000:12012, B - 12:B]


@pytest.mark.parametrize("B,ct,sb", CASES, ids=CASE_IDS)
def test_loop_vs_oracle(hip_lib, oracle_built, monkeypatch, B, ct, sb):
    """cartpole u_bound 0.8, cartpole_x0(seed=31), tolerance 1e-3, max_iter 10, 15 steps — test_mpc_rollout_chain's inputs:
    applied controls, plant states, the last solution and the final workspace against the fp64 oracle's loop on a sample"""
    prob, x0 = _cartpole(sb, u_bound=0.8), t.problems.cartpole_x0(B, seed=31)
    r = _run(monkeypatch, B, ct, sb, True)
    _rollout_vs_oracle(oracle_built, prob, _kw(ct), x0, STEPS, r["bs"], r["log"], _sample(B), f"loop B={B} ct={ct} sb={sb}")
    if sb:
        assert np.abs(r["ws"]["g"]).max() > 1e-4, "the state bound never acted"


@pytest.mark.parametrize("B,ct,sb", CASES, ids=CASE_IDS)
def test_loop_vs_chain_every_instance(hip_lib, monkeypatch, B, ct, sb):
    """the loop does the chain's arithmetic: the expected share of equal iteration counts is 1.0.
    Measured on an MI355X: 1.00000 in all six cases."""
    a, c = _run(monkeypatch, B, ct, sb, True), _run(monkeypatch, B, ct, sb, False)
    _same_as_chain(a, c, f"B={B} ct={ct} sb={sb}")


@pytest.mark.parametrize("ct", [1, 10])
def test_both_kinds_of_step_end_occur(hip_lib, monkeypatch, ct):
    """the lanes of a wavefront do not leave a step together: a loop that kept the state on chip only for wavefronts that
    converge as one would never run on these inputs"""
    log = _run(monkeypatch, B_G1, ct, False, True)["log"]
    it, so = log["iter"].reshape(STEPS, -1, 64), log["solved"].reshape(STEPS, -1, 64)
    ragged = (it != it[:, :, :1]) | (so != so[:, :, :1])
    print(f"ct={ct}: wavefronts with unequal (iter, solved), per step: {ragged.any(axis=2).sum(axis=1)} of {it.shape[1]}")
    print(f"ct={ct}: wavefronts 0 and 1, per step: {ragged[:, :2].any(axis=2).tolist()}")
    assert ragged.any(axis=2).any(axis=1).all(), "a step in which every wavefront left with equal (iter, solved)"
    if ct == 10:
        assert np.all(it == 10)
        mixed = so.any(axis=2) & ~so.all(axis=2)                # converged and max_iter exits at iteration 10 in one wavefront
        print(f"ct=10: wavefronts mixing both exits at iteration 10, per step: {mixed.sum(axis=1)}")
        assert mixed.any(axis=1).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. no cross-talk
# ---------------------------------------------------------------------------------------------------------------------------
def test_no_cross_talk(hip_lib, oracle_built, monkeypatch):
    """every lane of a wavefront gets the same x0, every wavefront another one: the log is bit-identical within a wavefront
    (the staged stores and loads of y, d and the rows of v, z belong to their lanes), one lane per sampled wavefront holds
    the oracle comparison"""
    B = B_RAGGED
    prob, kw = _cartpole(u_bound=0.8), _kw(1)
    nw = math.ceil(B / 64)
    x0 = np.asfortranarray(np.repeat(t.problems.cartpole_x0(nw, seed=31), 64, axis=1)[:, :B])
    r = _rollout(monkeypatch, prob, B, kw, x0, STEPS, True)
    log, first = r["log"], (np.arange(B) // 64) * 64
    for key in ("x", "u", "iter", "solved"):
        assert np.array_equal(log[key], log[key][..., first]), key
    assert np.array_equal(r["sol"]["controls"], r["sol"]["controls"][..., first])
    for key in WS_KEYS:
        assert np.array_equal(r["ws"][key], r["ws"][key][..., first]), key
    assert len(np.unique(log["x"][0, 0, ::64])) > nw // 2         # ... and the wavefronts differ
    pick = np.array([5, 64 + 63, 64 * 100 + 17, 64 * 255 + 40, 64 * 319, 20480 + 32])
    _rollout_vs_oracle(oracle_built, prob, kw, x0, STEPS, r["bs"], log, pick, "one x0 per wavefront")
    r["bs"].close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. an exit at iteration 1
# ---------------------------------------------------------------------------------------------------------------------------
def test_sixty_steps_reach_the_exit_at_iteration_one(hip_lib, oracle_built, monkeypatch):
    """test_mpc_rollout_chain_sixty_steps on the loop: a lane that converges at iteration 1 hands the loaded v, z, d on
    untouched (its row was never written, its d stored as loaded)"""
    prob, kw = _cartpole(u_bound=0.8), _kw(1)
    x0 = t.problems.cartpole_x0(B_G1, seed=41)
    r = _rollout(monkeypatch, prob, B_G1, kw, x0, 60, True)
    first_exit = _rollout_vs_oracle(oracle_built, prob, kw, x0, 60, r["bs"], r["log"], np.arange(256), "loop, 60 steps")
    assert first_exit >= 1, "the sample holds no closed loop with an exit at iteration 1"
    assert np.any((r["log"]["iter"][:, :64] == 1) & (r["log"]["solved"][:, :64] == 1))
    r["bs"].close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. edges
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 2])
def test_one_and_two_steps(hip_lib, monkeypatch, steps):
    prob, x0 = _cartpole(u_bound=0.8), t.problems.cartpole_x0(B_RAGGED, seed=31)
    a = _rollout(monkeypatch, prob, B_RAGGED, _kw(1), x0, steps, True)
    c = _rollout(monkeypatch, prob, B_RAGGED, _kw(1), x0, steps, False)
    _same_as_chain(a, c, f"{steps} step(s)")
    a["bs"].close(); c["bs"].close()


def test_solve_and_second_loop_behind_the_loop(hip_lib, monkeypatch):
    """mpc_rollout(5), then a solve() from the plant state and the workspace the loop left, then a second mpc_rollout(5) on
    the same solver — against the chain doing the same"""
    prob, x0 = _cartpole(u_bound=0.8), t.problems.cartpole_x0(B_RAGGED, seed=31)
    a = _rollout(monkeypatch, prob, B_RAGGED, _kw(1), x0, 5, True)
    c = _rollout(monkeypatch, prob, B_RAGGED, _kw(1), x0, 5, False)
    share = _same_as_chain(a, c, "first loop")
    for r in (a, c):
        bs = r["bs"]
        bs.solve()
        assert bs.last_launch_name == LEAN
        r.update(sol=bs.get_solution(), st=bs.get_status(), ws=bs.get_workspace(), status=bs.solve_status())
        # (the plant state the loop left: without a state bound knot 0 of the solution is x0 itself)
        assert np.array_equal(r["sol"]["states"][:, 0, :], r["log"]["x"][:, -1, :])
    assert np.array_equal(a["sol"]["states"][:, 0, :], c["sol"]["states"][:, 0, :])
    share = min(share, _same_as_chain(a, c, "solve() behind the loop"))
    for r, n in ((a, 1), (c, 5)):
        bs = r["bs"]
        log = bs.mpc_rollout(5)
        assert bs.last_launch_name == LEAN and _launches(bs) == n
        r.update(log=log, sol=bs.get_solution(), st=bs.get_status(), ws=bs.get_workspace(), status=bs.solve_status())
    share = min(share, _same_as_chain(a, c, "second loop"))
    assert share >= 0.9
    a["bs"].close(); c["bs"].close()


@pytest.mark.parametrize("case", ["shared_refs", "knot_bounds", "knot_bounds+state_bound+shared_refs"])
def test_shared_references_and_knot_bounds(hip_lib, monkeypatch, case):
    """references that are constant over the loop and per-knot input bounds are staged once, ahead of the step loop"""
    prob = _cartpole("state_bound" in case, u_bound=0.8)
    if "knot_bounds" in case:
        rng = np.random.default_rng(5)
        prob.u_max = np.asfortranarray(0.2 + 0.5 * rng.random((1, 19)))
        prob.u_min = np.asfortranarray(-(0.2 + 0.5 * rng.random((1, 19))))
    xref = None
    if "shared_refs" in case:
        xref = np.zeros((4, 20), order="F")
        xref[0] = 0.05
    x0 = t.problems.cartpole_x0(B_RAGGED, seed=31)
    a = _rollout(monkeypatch, prob, B_RAGGED, _kw(1), x0, 5, True, xref=xref)
    c = _rollout(monkeypatch, prob, B_RAGGED, _kw(1), x0, 5, False, xref=xref)
    _same_as_chain(a, c, case)
    a["bs"].close(); c["bs"].close()


def test_fixed_iteration_loop(hip_lib, monkeypatch):
    """tolerances 0: the tolerance-terminated loop kernel does the fixed-iteration arithmetic, every lane leaves at max_iter"""
    prob, x0 = _cartpole(u_bound=0.8), t.problems.cartpole_x0(B_RAGGED, seed=31)
    kw = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=10, check_termination=1)
    a = _rollout(monkeypatch, prob, B_RAGGED, kw, x0, 5, True)
    c = _rollout(monkeypatch, prob, B_RAGGED, kw, x0, 5, False)
    assert np.all(a["log"]["iter"] == 10) and not a["log"]["solved"].any()
    _same_as_chain(a, c, "fixed iterations", floor=1.0)
    a["bs"].close(); c["bs"].close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. fallbacks
# ---------------------------------------------------------------------------------------------------------------------------
def test_reference_sequence_keeps_the_chain(hip_lib, oracle_built, monkeypatch):
    """per-step references are re-staged launch by launch: with both switches the loop stays the chain of `steps` launches and
    holds tests/test_ref_sequence_gpu.py::test_chain_on_lean's comparison with the oracle's tracking loop"""
    from tests.test_ref_sequence import cartpole_tracking_refs
    from tests.test_ref_sequence_gpu import TOL10, _check_vs_oracle
    from tests.test_ref_sequence_gpu import _solver as _seq_solver
    _switches(monkeypatch, True, True)
    monkeypatch.setenv("TINYMPC_HIP_GROUP", "1")
    N, B, steps = 20, 130, 8
    prob = t.problems.cartpole(N, u_bound=0.5)
    x0 = t.problems.cartpole_x0(B, seed=17)
    xs, us = cartpole_tracking_refs(N, steps)
    bs = _seq_solver(prob, B, TOL10, xs, us)
    bs.set_x0(x0)
    log = bs.mpc_rollout(steps)
    assert bs.last_launch_name == LEAN and _launches(bs) == steps
    _check_vs_oracle(oracle_built, "cartpole20-tol", prob, TOL10, x0, xs, us, steps, bs, log, 0.85, "lean chain, both switches")
    bs.set_ref_sequence(None, None)                              # ... and without the sequence the same solver takes the loop
    bs.mpc_rollout(steps)
    assert bs.last_launch_name == LEAN and _launches(bs) == 1
    bs.close()


def test_horizon_beyond_the_lds_budget_stays_on_quad(hip_lib, monkeypatch, jit_on):
    _switches(monkeypatch, True, True)
    prob, x0 = _cartpole(N=30), t.problems.cartpole_x0(B_G1, seed=54)
    bs = _solver(prob, B_G1, _kw(1))
    bs.set_x0(x0)
    bs.mpc_rollout(3)
    assert bs.last_launch_name == "quad<4,1,30,g1>" and _launches(bs) == 1
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 9. specialisation
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [10, 12])
def test_other_horizon_through_specialisation(hip_lib, oracle_built, monkeypatch, jit_on, N):
    """N = 12 has no built-in lean kernel: the one loop variant the launch needs is compiled (LV_MPC).  N = 10 has a built-in
    lean entry for one-shot solves only, so its closed loop is the quad kernel's in-kernel loop — one launch either way"""
    prob, x0 = _cartpole(N=N, u_bound=0.8), t.problems.cartpole_x0(B_RAGGED, seed=31)
    r = _rollout(monkeypatch, prob, B_RAGGED, _kw(1), x0, 6, True, name="lean<4,1,12>" if N == 12 else "quad<4,1,10,")
    _rollout_vs_oracle(oracle_built, prob, _kw(1), x0, 6, r["bs"], r["log"], np.r_[0:24, 20480:B_RAGGED], f"N={N} specialised")
    r["bs"].close()
