"""The lean kernel's epilogue and launch (csrc/admm_lean.hip.h, csrc/lean_entry.hip.h, Solver::launch_pass): the final store in
16-byte pieces through LDS (store_wave_wide, csrc/admm_quad.hip.h), the status fold with its swaps issued together, and a
profiled solve whose timing events ride in the kernel's own dispatch packet.

Every instance against the fp64 oracle at FP32_TOL (tests/util.parity_every_instance), over batches that leave the last
wavefront / workgroup ragged, wavefronts of which only a part converges (the predicated store), the calling patterns with a
store path of their own (a finite state bound, per-knot input bounds, shared references, the dense controller-Hessenberg
sweeps, two wavefronts per SIMD) and horizons specialised at the first solve.  The same solve with profiling off, with the
events attached to the dispatch and with TINYMPC_HIP_EVENT_MARKERS (separate event records) must give the same bits.

(The solver sizes its output buffers to the batch exactly and hands out no larger view of them, so bytes beyond the batch are
not visible to a test; what a ragged wavefront may have written of ANOTHER instance inside the batch is — every instance is
compared.)"""
import copy
import os
import time

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.util import FP32_TOL, parity_every_instance

pytestmark = pytest.mark.gpu

FIXED = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=100, check_termination=1)
TOL = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1)
NT = min(16, len(os.sched_getaffinity(0)))


def _solve(prob, x0, kw, xr=None, ur=None, profiling=False, use_async=False):
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=x0.shape[1])
    bs.update_settings(**kw)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(False)
    if xr is not None:
        bs.set_x_ref(xr)
        bs.set_u_ref(ur)
    bs.set_x0(x0)
    bs.set_profiling(profiling)
    t0 = time.perf_counter()
    if use_async:
        bs.solve_async()
        status = bs.solve_status()
    else:
        status = bs.solve()
    wall_ms = 1e3 * (time.perf_counter() - t0)
    out = dict(name=bs.last_launch_name, status=status, sol=bs.get_solution(), st=bs.get_status(), k_ms=bs.kernel_elapsed_ms(),
               wall_ms=wall_ms)
    bs.close()
    return out


def _same_bits(a, b, tag):
    for key in ("states", "controls"):
        assert np.array_equal(a["sol"][key], b["sol"][key]), f"{tag}: {key} differ"
    for key in ("iter", "solved", "residuals"):
        assert np.array_equal(a["st"][key], b["st"][key]), f"{tag}: {key} differ"
    assert a["status"] == b["status"]


def _against_oracle(oracle_built, prob, x0, kw, out, xr=None, ur=None, min_same=1.0, tag=""):
    ref = oracle_built.solve_batch("orc64", prob, x0, xref=xr, uref=ur, nthreads=NT, **kw)

    def make(b=None):
        o = oracle_built.CpuSolver("orc64", prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
        o.update_settings(**kw)
        o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        if xr is not None:
            o.set_x_ref(xr)
            o.set_u_ref(ur)
        return o
    parity_every_instance(out["sol"], out["st"], ref, make, x0, kw, prob.rho, xref=xr, uref=ur, min_same=min_same, tag=tag)
    assert out["status"] == int(np.any(out["st"]["solved"] == 0))
    return ref


@pytest.mark.parametrize("B", [1, 63, 65, 255, 257, 20517, 65536])
def test_ragged_batches_and_launch_forms(hip_lib, oracle_built, monkeypatch, B):
    """fixed iterations (the benchmark's setting): plain launch, events attached to the dispatch, separate event records"""
    if B < 20480:
        monkeypatch.setenv("TINYMPC_HIP_GROUP", "1")            # one lane per instance at any batch: the lean kernel's entry
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(B, seed=71)
    plain = _solve(prob, x0, FIXED)
    assert plain["name"] == "lean<4,1,20>"
    assert plain["k_ms"] == -1.0
    assert np.all(plain["st"]["iter"] == 100) and not plain["st"]["solved"].any()
    _against_oracle(oracle_built, prob, x0, FIXED, plain, tag=f"batch {B}")
    attached = _solve(prob, x0, FIXED, profiling=True, use_async=True)
    _same_bits(plain, attached, f"batch {B}, attached events")
    assert 0.0 < attached["k_ms"] < attached["wall_ms"], attached
    monkeypatch.setenv("TINYMPC_HIP_EVENT_MARKERS", "1")
    markers = _solve(prob, x0, FIXED, profiling=True, use_async=True)
    _same_bits(plain, markers, f"batch {B}, event markers")
    assert 0.0 < markers["k_ms"] < markers["wall_ms"], markers


@pytest.mark.parametrize("B", [257, 20517])
def test_part_of_a_wavefront_converges(hip_lib, oracle_built, monkeypatch, B):
    """tolerance 1e-3 and an iteration limit at the median exit: about half of every wavefront stores at its convergence,
    inside the loop, the rest in the final store under the wavefront's mask"""
    if B < 20480:
        monkeypatch.setenv("TINYMPC_HIP_GROUP", "1")
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(B, seed=72)
    full = oracle_built.solve_batch("orc64", prob, x0, nthreads=NT, **TOL)
    kw = dict(TOL, max_iter=int(np.median(full["iter"])))
    out = _solve(prob, x0, kw)
    assert out["name"] == "lean<4,1,20>"
    s = out["st"]["solved"][:B // 64 * 64].reshape(-1, 64)
    assert ((s.min(axis=1) == 0) & (s.max(axis=1) == 1)).any(), "no wavefront with both kinds of instance"
    _against_oracle(oracle_built, prob, x0, kw, out, min_same=0.97, tag=f"part converged, batch {B}")
    _same_bits(out, _solve(prob, x0, kw, profiling=True, use_async=True), "part converged, attached events")
    # every instance converges before the limit: nothing is left for the final store of most wavefronts
    out = _solve(prob, x0, TOL)
    _against_oracle(oracle_built, prob, x0, TOL, out, min_same=0.97, tag=f"tol, batch {B}")


@pytest.mark.parametrize("case", ["state_bound", "knot_input_bounds", "shared_refs", "dense", "two_wavefronts_per_simd"])
@pytest.mark.parametrize("setting", ["fixed", "tol"])
def test_store_paths_of_the_other_patterns(hip_lib, oracle_built, monkeypatch, case, setting):
    B = 131072 if case == "two_wavefronts_per_simd" else 20480 + 37
    kw = FIXED if setting == "fixed" else dict(TOL, max_iter=40)
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(B, seed=73)
    prob = copy.copy(prob)
    xr = ur = None
    if case == "state_bound":
        prob.x_max, prob.x_min = prob.x_max.copy(), prob.x_min.copy()
        prob.x_max[0, :], prob.x_min[0, :] = 0.6 * np.abs(x0[0]).max(), -0.6 * np.abs(x0[0]).max()
    if case == "knot_input_bounds":
        rng = np.random.default_rng(6)
        prob.u_max = np.asfortranarray(0.2 + 0.5 * rng.random((1, 19)))
        prob.u_min = np.asfortranarray(-(0.2 + 0.5 * rng.random((1, 19))))
    if case == "shared_refs":
        rng = np.random.default_rng(7)
        xr, ur = 0.1 * rng.standard_normal((4, 20)), 0.05 * rng.standard_normal((1, 19))
    if case == "dense":
        monkeypatch.setenv("TINYMPC_HIP_LEAN_DENSE", "1")
    out = _solve(prob, x0, kw, xr, ur)
    assert out["name"] == "lean<4,1,20>"
    _against_oracle(oracle_built, prob, x0, kw, out, xr, ur, min_same=0.97 if setting == "tol" else 1.0, tag=f"{case} {setting}")
    _same_bits(out, _solve(prob, x0, kw, xr, ur, profiling=True, use_async=True), f"{case} {setting}, attached events")


@pytest.fixture
def jit_on(monkeypatch, tmp_path_factory):
    monkeypatch.delenv("TINYMPC_HIP_NO_JIT", raising=False)
    # one cache for the test session (a unit is compiled once), outside the home directory
    cache = os.environ.get("TINYMPC_TEST_JIT_CACHE") or str(tmp_path_factory.getbasetemp() / "lean_epilogue_jit_cache")
    os.makedirs(cache, exist_ok=True)
    monkeypatch.setenv("TINYMPC_HIP_CACHE", os.path.abspath(cache))


@pytest.mark.parametrize("shape", ["cartpole_N12", "cartpole_N30", "family_3_2_16", "family_3_2_28"])
def test_horizons_specialised_at_the_first_solve(hip_lib, oracle_built, jit_on, shape):
    """units jit.cpp compiles carry the same launch signature and epilogue: nx N = 48 stores 24 floats per pass, 120 stores 40;
    (3, 2, 16) has an even number of controls per instance (the flat control image at an even stride); (3, 2, 28) has 54 of
    them: the predicated control staging, 56 KB, is then the larger part of the workgroup's LDS"""
    B = 20480 + 91
    if shape.startswith("cartpole"):
        N = int(shape.split("N")[1])
        prob, x0 = t.problems.cartpole(N, u_bound=0.5), t.problems.cartpole_x0(B, seed=74)
        nx, nu = 4, 1
    else:
        nx, nu, N = (int(v) for v in shape.split("_")[1:])
        rng = np.random.default_rng(17)
        A = np.eye(nx) + 0.2 * rng.standard_normal((nx, nx)) / np.sqrt(nx)
        A *= 0.97 / np.abs(np.linalg.eigvals(A)).max()
        prob = t.problems.Problem("rand", A, 0.5 * rng.standard_normal((nx, nu)), np.diag(rng.uniform(0.5, 5.0, nx)),
                                  np.diag(rng.uniform(0.5, 3.0, nu)), float(rng.uniform(0.5, 2.0)), N)
        prob.x_min, prob.x_max = np.full((nx, N), -1e17), np.full((nx, N), 1e17)
        prob.u_min, prob.u_max = np.full((nu, N - 1), -0.4), np.full((nu, N - 1), 0.4)
        x0 = np.asfortranarray(rng.uniform(-0.5, 0.5, (nx, B)))
    for tag, kw in (("fixed", dict(FIXED, max_iter=60, check_termination=10)), ("tol", dict(TOL, max_iter=30))):
        out = _solve(prob, x0, kw, profiling=True, use_async=True)
        assert out["name"] == f"lean<{nx},{nu},{N}>", out["name"]
        assert 0.0 < out["k_ms"] < out["wall_ms"]
        _against_oracle(oracle_built, prob, x0, kw, out, min_same=0.95, tag=f"{shape} {tag}")


def test_status_after_async_solves_in_both_modes(hip_lib):
    """solve_async + the getters' wait: with profiling on the wait is on the launch's own stop event, with it off on the
    event recorded behind the launch; switching back and forth on one solver, kernel_elapsed_ms follows the mode"""
    B = 20480
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(B, seed=75)
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(False)
    bs.set_x0(x0)
    seen = []
    for profiling, kw in ((False, FIXED), (True, TOL), (False, TOL), (True, FIXED), (True, FIXED)):
        bs.update_settings(**kw)
        bs.set_profiling(profiling)
        t0 = time.perf_counter()
        bs.solve_async()
        st = bs.get_status()                                    # (waits for the launch)
        wall_ms = 1e3 * (time.perf_counter() - t0)
        status = bs.solve_status()
        assert bs.last_launch_name == "lean<4,1,20>"
        if kw is FIXED:
            assert status == 1 and np.all(st["iter"] == 100) and not st["solved"].any()
        else:
            assert status == int(np.any(st["solved"] == 0)) and st["iter"].min() < 100
        k_ms = bs.kernel_elapsed_ms()
        if profiling:
            assert 0.0 < k_ms < wall_ms, (k_ms, wall_ms)
            assert 0.0 < bs.kernel_elapsed_ms(2) < wall_ms * 4
        else:
            assert k_ms == -1.0
        seen.append((kw is FIXED, st, bs.get_solution()))
    bs.close()
    for a in seen:
        for b in seen:
            if a[0] == b[0]:
                assert np.array_equal(a[1]["iter"], b[1]["iter"]) and np.array_equal(a[2]["states"], b[2]["states"])
                assert np.array_equal(a[2]["controls"], b[2]["controls"]) and np.array_equal(a[1]["residuals"], b[1]["residuals"])
