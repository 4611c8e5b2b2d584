"""Precision 2 on the stream kernel's fp64-state form (csrc/admm_streamg.hip.h, ST = double; "stream4<NX,NU;f64>") behind
TINYMPC_HIP_STREAM_F64=1: scratch, knot buffers, slacks, duals, residual comparisons and the kept workspace in doubles, for the
shapes and calling patterns the lean kernel's fp64 form does not take — quadrotor and rocket, cones / the affine term / linear
rows, warm-started and workspace-kept solves.

The bars are tests/test_precision2_gpu.py's: inputs through _f32, the oracle is orc64, 1e-6 on solution and workspace,
iteration counts and solved flags exact, residuals within 1e-6 * max(1, |ref|).  A stream workgroup holds 64 instances, so
every batch here is ragged and spans more than one workgroup; (4,1) has one row per lane and idle input lanes, (6,3) masked
rows, (12,4) three rows per lane.  Each sample's mix of converged and max_iter exits was taken from the CPU oracle and is
asserted, so that neither exit drops out of the sample unnoticed."""
import os
import sys

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.util import FP32_TOL, load_golden, nrel, nrel_batch, problem_of

pytestmark = pytest.mark.gpu
TIGHT = 1e-6
KW3 = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, check_termination=1)


def _f32(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float32).astype(np.float64))


@pytest.fixture
def stream_f64(monkeypatch):
    monkeypatch.setenv("TINYMPC_HIP_STREAM_F64", "1")


def _solver(prob, B, kw, warm):
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    bs.update_settings(**kw)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(warm)
    bs.set_precision(2)
    return bs


def _check_cold(bs, ref, name):
    sol, st = bs.get_solution(), bs.get_status()
    assert bs.kernel_name == name and bs.last_launch_name == name
    assert np.array_equal(st["iter"], ref["iter"]) and np.array_equal(st["solved"], ref["solved"])
    ex, eu = nrel_batch(sol["states"], ref["x"]).max(), nrel_batch(sol["controls"], ref["u"]).max()
    er = np.abs(st["residuals"] - ref["res"]).max()
    print(f"{name}: x {ex:.3e} u {eu:.3e} residuals {er:.3e}")
    assert ex <= TIGHT and eu <= TIGHT
    assert er <= 1e-6 * max(1.0, np.abs(ref["res"]).max())


# ---- the quadrotor one-shot sample, shared by the parity test and the comparison with generic<f64> ----
QUAD_N, QUAD_B = 10, 171
QUAD_KW = dict(max_iter=60, **KW3)
_quad_cache = {}


def _quad_cold(oracle_built, state_bounds):
    if state_bounds not in _quad_cache:
        prob = t.problems.quadrotor(QUAD_N)
        if state_bounds:
            prob.x_min, prob.x_max = np.full((12, QUAD_N), -0.5), np.full((12, QUAD_N), 0.5)
        x0 = _f32(t.problems.quadrotor_x0(QUAD_B, seed=4))
        ref = oracle_built.solve_batch("orc64", prob, x0, nthreads=len(os.sched_getaffinity(0)), **QUAD_KW)
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _quad_cache[state_bounds] = (prob, x0, ref)
    return _quad_cache[state_bounds]


# ---- 1. routing ----
def _shape_case(shape):
    if shape == (12, 4):
        return t.problems.quadrotor(10), t.problems.quadrotor_x0(70, seed=4)
    if shape == (6, 3):
        return t.problems.rocket(10), t.problems.rocket_x0(70, seed=5)
    return t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(70, seed=1)


@pytest.mark.parametrize("shape", [(12, 4), (6, 3), (4, 1)], ids=lambda s: f"{s[0]}_{s[1]}")
def test_switch_routes_precision2_to_the_stream_kernel(hip_lib, stream_f64, shape):
    prob, x0 = _shape_case(shape)
    bs = _solver(prob, 70, dict(max_iter=5, **KW3), warm=True)
    bs.set_x0(_f32(x0))
    bs.solve()
    name = f"stream4<{shape[0]},{shape[1]};f64>"
    assert bs.kernel_name == name and bs.last_launch_name == name and bs.effective_precision == 2
    with pytest.raises(t.TinyMPCError):                 # the fused closed loop stays refused at precision 2
        bs.mpc_rollout(3)
    # back to the default precision on the same solver: the family a fresh solver of the shape gets
    bs.set_precision(0)
    bs.solve()
    fresh = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=70)
    fresh.update_settings(max_iter=5, **KW3)
    fresh.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    fresh.set_warm_start(True)
    fresh.set_x0(_f32(x0))
    fresh.solve()
    assert bs.kernel_name == fresh.kernel_name and "f64" not in bs.kernel_name and bs.effective_precision == 0
    fresh.close()
    bs.close()


def test_switch_off_and_adaptive_rho_stay_on_the_generic_kernel(hip_lib, monkeypatch):
    prob, x0 = _shape_case((12, 4))
    monkeypatch.delenv("TINYMPC_HIP_STREAM_F64", raising=False)
    bs = _solver(prob, 70, dict(max_iter=5, **KW3), warm=True)
    bs.set_x0(_f32(x0))
    bs.solve()
    assert bs.kernel_name == "generic<f64>" and bs.last_launch_name == "generic<f64>"
    bs.close()
    monkeypatch.setenv("TINYMPC_HIP_STREAM_F64", "1")
    bs = _solver(prob, 70, dict(max_iter=5, **KW3), warm=True)
    bs.set_adaptive_rho(True)
    bs.set_x0(_f32(x0))
    bs.solve()
    assert bs.kernel_name == "generic<f64>" and bs.last_launch_name == "generic<f64>"
    bs.set_adaptive_rho(False)                          # ... and without it, the same solver is routed to the stream kernel
    bs.solve()
    assert bs.kernel_name == "stream4<12,4;f64>" and bs.last_launch_name == "stream4<12,4;f64>"
    bs.close()


# ---- 2. cold one-shot solves, both exits (the OS form) ----
CART_B, CART_KW = 130, dict(max_iter=100, **KW3)
_cart_cache = []


def _cart_cold(oracle_built):
    if not _cart_cache:
        prob = t.problems.cartpole(20, u_bound=0.5)
        x0 = _f32(t.problems.cartpole_x0(CART_B, seed=1))
        ref = oracle_built.solve_batch("orc64", prob, x0, nthreads=len(os.sched_getaffinity(0)), **CART_KW)
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cart_cache.append((prob, x0, ref))
    return _cart_cache[0]


def test_cold_one_shot_cartpole(hip_lib, oracle_built, stream_f64):
    prob, x0, ref = _cart_cold(oracle_built)
    assert ref["solved"].sum() == 66 and ref["iter"].min() == 4 and ref["iter"].max() == 100
    bs = _solver(prob, CART_B, CART_KW, warm=False)
    bs.set_x0(x0)
    bs.solve()
    _check_cold(bs, ref, "stream4<4,1;f64>")
    bs.close()


def test_lean_kernel_keeps_its_launches(hip_lib, oracle_built, stream_f64, monkeypatch, tmp_path):
    """with specialisation on, the cold one-shot solve of a shape the lean kernel holds still runs on lean<...;f64> (the family
    reported is the stream form); a kept workspace, and rows added afterwards — which the lean kernel does not take — go to
    the stream kernel on the very next launch"""
    monkeypatch.delenv("TINYMPC_HIP_NO_JIT", raising=False)
    monkeypatch.setenv("TINYMPC_HIP_CACHE", os.environ.get("TINYMPC_TEST_JIT_CACHE") or str(tmp_path))   # (one small unit: 2 s)
    prob, x0, ref = _cart_cold(oracle_built)
    bs = _solver(prob, CART_B, CART_KW, warm=False)
    bs.set_x0(x0)
    bs.solve()
    assert bs.kernel_name == "stream4<4,1;f64>" and bs.last_launch_name == "lean<4,1,20;f64>", (bs.kernel_name, bs.last_launch_name)
    sol, st = bs.get_solution(), bs.get_status()
    assert np.array_equal(st["iter"], ref["iter"]) and np.array_equal(st["solved"], ref["solved"])
    assert nrel_batch(sol["states"], ref["x"]).max() <= TIGHT and nrel_batch(sol["controls"], ref["u"]).max() <= TIGHT
    bs.set_warm_start(True)
    bs.solve()
    assert bs.last_launch_name == "stream4<4,1;f64>"
    bs.set_warm_start(False)
    g = load_golden("X3_cartpole_linear_rows")
    bs.set_linear_constraints(np.array(g["lin"]["Ax"][:1]), np.array(g["lin"]["bx"][:1]), np.array(g["lin"]["Au"][1:]), np.array(g["lin"]["bu"][1:]))
    bs.solve()
    assert bs.kernel_name == "stream4<4,1;f64>" and bs.last_launch_name == "stream4<4,1;f64>"
    assert not np.array_equal(bs.get_solution()["controls"], sol["controls"])     # (the rows took effect)
    bs.close()


@pytest.mark.parametrize("state_bounds,n_conv", [(True, 5), (False, 117)], ids=["state_bounds", "input_bounds_only"])
def test_cold_one_shot_quadrotor(hip_lib, oracle_built, stream_f64, state_bounds, n_conv):
    prob, x0, ref = _quad_cold(oracle_built, state_bounds)
    assert ref["solved"].sum() == n_conv and (ref["iter"][ref["solved"] == 0] == QUAD_KW["max_iter"]).all()
    bs = _solver(prob, QUAD_B, QUAD_KW, warm=False)
    bs.set_x0(x0)
    bs.solve()
    _check_cold(bs, ref, "stream4<12,4;f64>")
    bs.close()


# ---- 3. workspace kept, host-stepped closed loop (the non-OS form) ----
@pytest.mark.parametrize("case", ["quadrotor_state_bounds", "rocket_cones_fdyn"])
def test_workspace_kept_closed_loop(hip_lib, oracle_built, stream_f64, case):
    """tests/test_precision2_gpu.py::test_workspace_kept_closed_loop_in_fp64 on the stream kernel: one persistent oracle per
    instance; solution, iteration count, solved flag and the workspace (d, y, g, v, z) after every solve.  The rocket case
    converges on every instance at every step: the converged exit's workspace (v, z one iteration old, admm.cpp:181-197)."""
    B = 70
    if case == "quadrotor_state_bounds":
        N, steps, name = 10, 4, "stream4<12,4;f64>"
        prob = t.problems.quadrotor(N)
        prob.x_min, prob.x_max = np.full((12, N), -0.5), np.full((12, N), 0.5)
        x0 = _f32(t.problems.quadrotor_x0(B, seed=8))
        kw = dict(max_iter=40, **KW3)
        fdyn, cones, xr, ur = None, None, None, None
    else:
        N, steps, name = 10, 5, "stream4<6,3;f64>"
        prob = t.problems.rocket(N)
        x0 = _f32(t.problems.rocket_x0(B, seed=5))
        kw = dict(abs_pri_tol=2e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1)
        fdyn, cones = prob.fdyn, ([0], [3], [0.25], [0], [3], [0.5])
        xr, ur = t.problems.rocket_refs(N)

    def configure(o):
        o.update_settings(**kw)
        o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        if fdyn is not None:
            o.set_fdyn(fdyn)
            o.set_cone_constraints(*cones)
            o.set_x_ref(xr)
            o.set_u_ref(ur)
        return o
    bs = configure(t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B))
    bs.set_warm_start(True)
    bs.set_precision(2)
    orcs = [configure(oracle_built.CpuSolver("orc64", prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)) for _ in range(B)]
    f = fdyn if fdyn is not None else np.zeros(prob.nx)
    x = x0.copy()
    worst = dict(x=0.0, u=0.0, d=0.0, y=0.0, g=0.0, v=0.0, z=0.0)
    for k in range(steps):
        bs.set_x0(x)
        bs.solve()
        assert bs.kernel_name == name and bs.last_launch_name == name
        sol, st, ws = bs.get_solution(), bs.get_status(), bs.get_workspace()
        xn = np.zeros_like(x)
        conv, iters = 0, []
        for b in range(B):
            o = orcs[b]
            o.set_x0(x[:, b])
            o.solve()
            r = o.get_solution()
            assert st["iter"][b] == r["iter"] and st["solved"][b] == r["solved"], f"step {k} instance {b}: {st['iter'][b]} vs {r['iter']}"
            conv += r["solved"]
            iters.append(r["iter"])
            ex_, eu_ = nrel(sol["states"][:, :, b], r["x"]), nrel(sol["controls"][:, :, b], r["u"])
            worst["x"], worst["u"] = max(worst["x"], ex_), max(worst["u"], eu_)
            assert ex_ <= TIGHT and eu_ <= TIGHT, f"step {k} instance {b}: x {ex_:.3e} u {eu_:.3e}"
            sv = o.get_state()
            for key in ("d", "y", "g", "v", "z"):
                e_ = np.abs(ws[key][:, :, b] - sv[key]).max() / max(np.abs(sv[key]).max(), 1e-2)
                worst[key] = max(worst[key], e_)
                assert e_ <= TIGHT, f"step {k} instance {b} workspace {key}: {e_:.3e}"
            xn[:, b] = _f32(prob.A @ x[:, b] + prob.B @ r["u"][:, 0] + f)      # (what set_x0 hands the kernel: fp32)
        if case == "rocket_cones_fdyn":
            assert conv == B and min(iters) >= 12 and max(iters) <= 68, (k, conv, min(iters), max(iters))
        else:
            assert conv == 2, (k, conv)                                         # both exits at every step
        x = xn
    print(case, {k_: f"{v_:.2e}" for k_, v_ in worst.items()})
    if case == "quadrotor_state_bounds":
        assert np.abs(bs.get_workspace()["g"]).max() > 1.0                      # duals far above the trajectory's scale
    for o in orcs:
        o.close()
    bs.close()


# ---- 4. constraints added after the first solve ----
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "workspace_kept"])
def test_linear_rows_added_after_the_first_solve(hip_lib, oracle_built, stream_f64, warm):
    """which EXT form launches follows the constraints at every launch: a box-only solve, then one state row and one input row
    (tests/golden/X3_cartpole_linear_rows.json's problem and rows), and the second solve runs the linear-row form — compared
    with oracles taken through the same sequence.  The second solve reads per-instance references."""
    g = load_golden("X3_cartpole_linear_rows")
    prob = problem_of(g)
    nx, nu, N, B = prob.nx, prob.nu, prob.N, 130
    Ax, bx = np.array(g["lin"]["Ax"][:1]), np.array(g["lin"]["bx"][:1])
    Au, bu = np.array(g["lin"]["Au"][1:]), np.array(g["lin"]["bu"][1:])
    rng = np.random.default_rng(11)
    x0 = _f32(np.array(g["x0"])[:, None] * (1.0 + 0.2 * rng.uniform(-1, 1, (nx, B))))
    xr = _f32(0.02 * rng.standard_normal((nx, N, B)))
    ur = _f32(0.02 * rng.standard_normal((nu, N - 1, B)))
    kw = dict(max_iter=80, **KW3)
    bs = _solver(prob, B, kw, warm=warm)
    orcs = []
    for b in range(B):
        o = oracle_built.CpuSolver("orc64", prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
        o.update_settings(**kw)
        o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        orcs.append(o)
    bound_x = bound_u = 0
    for k in range(2):
        if k == 1:
            bs.set_linear_constraints(Ax, bx, Au, bu)
            bs.set_x_ref(xr)
            bs.set_u_ref(ur)
        bs.set_x0(x0)
        bs.solve()
        assert bs.kernel_name == "stream4<4,1;f64>" and bs.last_launch_name == "stream4<4,1;f64>"
        sol, st = bs.get_solution(), bs.get_status()
        for b in range(B):
            o = orcs[b]
            if k == 1:
                o.set_linear_constraints(Ax, bx, Au, bu)
                o.set_x_ref(xr[:, :, b])
                o.set_u_ref(ur[:, :, b])
            if not warm:
                o.reset()
            o.set_x0(x0[:, b])
            o.solve()
            r = o.get_solution()
            assert st["iter"][b] == r["iter"] and st["solved"][b] == r["solved"], f"solve {k} instance {b}: {st['iter'][b]} vs {r['iter']}"
            ex_, eu_ = nrel(sol["states"][:, :, b], r["x"]), nrel(sol["controls"][:, :, b], r["u"])
            assert ex_ <= TIGHT and eu_ <= TIGHT, f"solve {k} instance {b}: x {ex_:.3e} u {eu_:.3e}"
            assert np.abs(st["residuals"][b] - r["res"]).max() <= 1e-6 * max(1.0, np.abs(r["res"]).max())
            if k == 1:     # the rows bind: the unconstrained solve of the same instance crossed them
                bound_x += bool((Ax @ first[b][0]).max() > bx[0])
                bound_u += bool((Au @ first[b][1]).max() > bu[0])
        if k == 0:
            first = [(sol["states"][:, :, b].copy(), sol["controls"][:, :, b].copy()) for b in range(B)]
    assert bound_x > B // 2 and bound_u > B // 2, (bound_x, bound_u)
    for o in orcs:
        o.close()
    bs.close()


# ---- 5. the seeds that missed ----
@pytest.mark.parametrize("seed", [1109, 1125, 1003, 1017])
def test_fuzz_seeds_that_missed(hip_lib, oracle_built, stream_f64, seed):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import fuzz_mfmat
    name, pattern, ok = fuzz_mfmat.one(seed, precision=2, tol=FP32_TOL)
    assert name == "stream4<6,3;f64>" and ok, (seed, pattern, name)


# ---- 6. against generic<f64> of the same library ----
def test_agrees_with_the_generic_kernel(hip_lib, oracle_built, monkeypatch):
    """same inputs, switch off and on: iteration counts and flags equal, solutions within TIGHT (not bit-equal: the mat-vec
    sums are ordered by lane in the stream kernel)"""
    prob, x0, ref = _quad_cold(oracle_built, True)
    out = {}
    for on in (False, True):
        if on:
            monkeypatch.setenv("TINYMPC_HIP_STREAM_F64", "1")
        else:
            monkeypatch.delenv("TINYMPC_HIP_STREAM_F64", raising=False)
        bs = _solver(prob, QUAD_B, QUAD_KW, warm=False)
        bs.set_x0(x0)
        bs.solve()
        assert bs.last_launch_name == ("stream4<12,4;f64>" if on else "generic<f64>")
        out[on] = (bs.get_solution(), bs.get_status())
        bs.close()
    (sa, ta), (sb, tb) = out[False], out[True]
    assert np.array_equal(ta["iter"], tb["iter"]) and np.array_equal(ta["solved"], tb["solved"])
    assert 0 < ta["solved"].sum() < QUAD_B
    assert nrel_batch(sb["states"], sa["states"]).max() <= TIGHT and nrel_batch(sb["controls"], sa["controls"]).max() <= TIGHT
    assert np.abs(ta["residuals"] - tb["residuals"]).max() <= 1e-6 * max(1.0, np.abs(ta["residuals"]).max())
