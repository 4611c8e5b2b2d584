"""The lean kernel's fixed-iteration variants iterate in controller-Hessenberg coordinates x = T x^ (csrc/admm_lean.hip.h,
HB): every instance against the fp64 oracle and against the quad kernel, on random (4,1) families — complex eigenvalues
and uncontrollable pairs included — with the residual iteration at several places, shared references, and beyond one
wavefront per SIMD."""
import os

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.util import FP32_TOL, nrel_batch, parity_every_instance

pytestmark = pytest.mark.gpu

B1 = 20480            # one lane per instance from 20 480 instances up; one wavefront per SIMD (the 512-register form)
FIXED = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=100, check_termination=1)


def _family(kind, seed):
    p = t.problems.cartpole(20, u_bound=0.5)
    rng = np.random.default_rng(seed)
    if kind == "perturbed":
        p.A = p.A + 0.02 * rng.standard_normal((4, 4))
        p.B = p.B + 0.02 * rng.standard_normal((4, 1))
    elif kind == "complex":                                   # a lightly damped oscillator beside the cart
        th = rng.uniform(0.2, 0.6)
        A = np.eye(4)
        A[0, 1] = 0.05
        A[2:, 2:] = 0.99 * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        A[0, 2] = 0.01
        Q, _ = np.linalg.qr(rng.standard_normal((4, 4)))
        p.A, p.B = Q @ A @ Q.T, Q @ np.array([[0.0], [0.05], [0.03], [0.0]])
    elif kind == "uncontrollable":                            # a stable rotation block the input never reaches
        th = rng.uniform(0.2, 0.6)
        A = np.zeros((4, 4))
        A[:2, :2] = [[1.0, 0.05], [0.0, 1.0]]
        A[2:, 2:] = 0.95 * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        A[:2, 2:] = 0.02 * rng.standard_normal((2, 2))
        Q, _ = np.linalg.qr(rng.standard_normal((4, 4)))
        p.A, p.B = Q @ A @ Q.T, Q @ np.array([[0.001], [0.05], [0.0], [0.0]])
    return p


def _solve(prob, x0, kw, xr=None, ur=None, no_lean=False, monkeypatch=None):
    if no_lean:
        monkeypatch.setenv("TINYMPC_HIP_NO_LEAN", "1")
    B = x0.shape[1]
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    bs.update_settings(**kw)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(False)
    if xr is not None:
        bs.set_x_ref(xr)
        bs.set_u_ref(ur)
    bs.set_x0(x0)
    bs.solve()
    out = (bs.last_launch_name, bs.get_solution(), bs.get_status())
    bs.close()
    if no_lean:
        monkeypatch.delenv("TINYMPC_HIP_NO_LEAN")
    return out


def _oracle(oracle_built, prob, kw, xr=None, ur=None):
    def make(b=None):
        o = oracle_built.CpuSolver("orc64", prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
        o.update_settings(**kw)
        o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        if xr is not None:
            o.set_x_ref(xr)
            o.set_u_ref(ur)
        return o
    return make


def _residuals_match(st, ref):
    dres = np.abs(st["residuals"] - ref["res"]).max(axis=0) / np.maximum(1.0, np.abs(ref["res"]).max(axis=0))
    assert dres.max() <= FP32_TOL, f"residuals (pri_x, dua_x, pri_u, dua_u) off by {dres}"


@pytest.mark.parametrize("kind", ["perturbed", "complex", "uncontrollable"])
def test_random_families_vs_oracle_and_quad(hip_lib, oracle_built, monkeypatch, kind):
    prob, x0 = _family(kind, seed=len(kind)), t.problems.cartpole_x0(B1, seed=51)
    ref = oracle_built.solve_batch("orc64", prob, x0, nthreads=len(os.sched_getaffinity(0)), **FIXED)
    name, sol, st = _solve(prob, x0, FIXED)
    assert name == "lean<4,1,20>"
    parity_every_instance(sol, st, ref, _oracle(oracle_built, prob, FIXED), x0, FIXED, prob.rho, min_same=1.0, tag=f"hb {kind}")
    _residuals_match(st, ref)
    qname, qsol, qst = _solve(prob, x0, FIXED, no_lean=True, monkeypatch=monkeypatch)
    assert qname == "quad<4,1,20,g1>"
    assert nrel_batch(sol["states"], qsol["states"]).max() <= 4e-6
    assert nrel_batch(sol["controls"], qsol["controls"]).max() <= 4e-6
    assert np.array_equal(st["iter"], qst["iter"])


@pytest.mark.parametrize("max_iter", [1, 47])
@pytest.mark.parametrize("ct", [1, 10])
def test_residual_iteration_placement(hip_lib, oracle_built, max_iter, ct):
    """the residual iteration (the only one that maps x^ back inside the loop) at the first iteration, at 39 of 47, at 46
    of 47, or nowhere (one iteration, checks every 10): the reported residuals are the oracle's to fp32 rounding"""
    kw = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=max_iter, check_termination=ct)
    prob, x0 = _family("complex", seed=3), t.problems.cartpole_x0(B1, seed=52)
    ref = oracle_built.solve_batch("orc64", prob, x0, nthreads=len(os.sched_getaffinity(0)), **kw)
    name, sol, st = _solve(prob, x0, kw)
    assert name == "lean<4,1,20>"
    parity_every_instance(sol, st, ref, _oracle(oracle_built, prob, kw), x0, kw, prob.rho, min_same=1.0, tag=f"hb {max_iter}/{ct}")
    assert np.all(st["iter"] == max_iter) and not st["solved"].any()
    _residuals_match(st, ref)


def test_shared_references_without_state_bound(hip_lib, oracle_built):
    prob, x0 = _family("uncontrollable", seed=8), t.problems.cartpole_x0(B1, seed=53)
    rng = np.random.default_rng(17)
    xr = np.asfortranarray(0.1 * rng.standard_normal((4, 20)))
    ur = np.asfortranarray(0.05 * rng.standard_normal((1, 19)))
    ref = oracle_built.solve_batch("orc64", prob, x0, xref=xr, uref=ur, nthreads=len(os.sched_getaffinity(0)), **FIXED)
    name, sol, st = _solve(prob, x0, FIXED, xr, ur)
    assert name == "lean<4,1,20>"
    parity_every_instance(sol, st, ref, _oracle(oracle_built, prob, FIXED, xr, ur), x0, FIXED, prob.rho, min_same=1.0, tag="hb shared refs")
    _residuals_match(st, ref)


def test_two_wavefronts_per_simd_against_quad(hip_lib, monkeypatch):
    """batch 131 072: the 256-register form (two wavefronts per SIMD) beside the Hessenberg one, against the quad kernel"""
    prob, x0 = _family("perturbed", seed=9), t.problems.cartpole_x0(131072, seed=54)
    name, sol, st = _solve(prob, x0, FIXED)
    assert name == "lean<4,1,20>"
    qname, qsol, _ = _solve(prob, x0, FIXED, no_lean=True, monkeypatch=monkeypatch)
    assert qname == "quad<4,1,20,g1>"
    assert nrel_batch(sol["states"], qsol["states"]).max() <= 4e-6
    assert nrel_batch(sol["controls"], qsol["controls"]).max() <= 4e-6
