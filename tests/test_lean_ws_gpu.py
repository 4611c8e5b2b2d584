"""The lean kernel's workspace-keeping form (csrc/admm_lean.hip.h, WS = true) behind TINYMPC_HIP_LEAN_WS=1: warm-started /
kept-workspace solves and mpc_rollout of the one-lane-per-instance cartpole entry on "lean<4,1,20>" instead of
"quad<4,1,20,g1>" — the reference's default calling pattern (solve() goes on from the d, y, g, v, z the previous solve left,
admm.cpp:111-115; examples/cartpole_example_mpc.jl:35-51).
 * routing: on with the switch for every calling pattern the lean kernel takes cold, unchanged without it, unchanged for
   what the lean kernel never took; another horizon through specialisation;
 * the workspace itself after every solve of a host-stepped closed loop — both exits of solve(): at max_iter the slack of
   the last iteration and the d of the backward pass behind it (admm.cpp:195-205), at convergence the PREVIOUS iteration's
   v, z, d (:181-193), at iteration 1 the loaded ones untouched — against persistent fp64 oracles on a sample and against
   the quad kernel on every instance;
 * fixed-iteration solves (max_iter 1: the first iteration is the residual iteration; dense sweeps: Hessenberg coordinates);
 * the reference's own closed loops (tests/golden/G5*) inside a full batch;
 * mpc_rollout as a chain of workspace-carrying launches with the plant state in fp64;
 * one solver going back and forth between cold and warm solves.
Limits: FP32_TOL for solutions; 2e-5 (d, z, v) and 4e-5 (g, y) of max(|ref|, 1e-2) for workspace arrays — what
tests/test_lean_gpu.py::test_kept_workspace_one_lane_per_instance holds the quad kernel's workspace to (the duals integrate
the trajectory's per-iteration fp32 rounding)."""
import ctypes
import os

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.util import FP32_TOL, cm, load_golden, nrel, nrel_batch, problem_of

pytestmark = pytest.mark.gpu

B_G1 = 24576                    # one lane per instance from 20 480 instances up (select_quad_kernel)
B_RAGGED = 20480 + 33           # the last wavefront has 33 instances
LEAN, QUAD = "lean<4,1,20>", "quad<4,1,20,g1>"
LF_PLAIN, LF_HB, LF_SPARSE = 1, 2, 3
WS_KEYS = ("d", "y", "z", "g", "v")
SAMPLE = np.r_[0:128, 4090:4218, 20480:20480 + 33]      # includes the ragged wavefront


def _lim(key):
    return 4e-5 if key in ("g", "y") else 2e-5


def _switch(monkeypatch, on):
    if on:
        monkeypatch.setenv("TINYMPC_HIP_LEAN_WS", "1")
    else:
        monkeypatch.delenv("TINYMPC_HIP_LEAN_WS", raising=False)


def _form(bs):
    f = ctypes.CDLL(t.LIB_PATH).tmpc_lean_last_form
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                  ctypes.POINTER(ctypes.c_int)]
    sp, cs, cd, form = ctypes.c_ulonglong(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert f(bs.h, ctypes.byref(sp), ctypes.byref(cs), ctypes.byref(cd), ctypes.byref(form)) == 0
    return form.value


def _cartpole(state_bound=False, N=20, u_bound=0.5):
    prob = t.problems.cartpole(N, u_bound=u_bound)
    if state_bound:
        prob.x_min, prob.x_max = prob.x_min.copy(), prob.x_max.copy()
        prob.x_min[0, :], prob.x_max[0, :] = -0.3, 0.3
    return prob


def _solver(prob, B, kw, warm=True, xref=None):
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    bs.update_settings(**kw)
    if prob.has_bounds():
        bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if xref is not None:
        bs.set_x_ref(xref)                                      # (2-D: one reference for the whole batch)
    bs.set_warm_start(warm)
    return bs


def _oracle(oracle_built, prob, kw, xref=None):
    o = oracle_built.CpuSolver("orc64", prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
    o.update_settings(**kw)
    if prob.has_bounds():
        o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if xref is not None:
        o.set_x_ref(xref)
    return o


def _oracle_step(o, x, it_g, so_g):
    """one solve of a persistent oracle from plant state x.  Returns (solution, workspace, the oracle's OWN (iter, solved),
    replayed): where the GPU's termination decision differs, the oracle's state is restored and the step replayed with the
    GPU's decision imposed (CpuSolver.set_forced_exit), so that no instance is dropped"""
    before = o.get_state()
    o.set_x0(x)
    o.solve()
    r = o.get_solution()
    own = (int(r["iter"]), int(r["solved"]))
    replayed = own != (int(it_g), int(so_g))
    if replayed:
        o.set_state(before["d"], before["y"], before["g"], before["v"], before["z"])
        o.set_forced_exit(int(it_g) if so_g else -1)
        o.set_x0(x)
        o.solve()
        o.set_forced_exit(0)
        r = o.get_solution()
        assert (int(r["iter"]), int(r["solved"])) == (int(it_g), int(so_g))
    return r, o.get_state(), own, replayed


def _closed_loop(prob, B, kw, x0, steps, name, xs=None, xref=None):
    """host-stepped closed loop; xs: the x0 sequence to feed (default: this run's own).  [(sol, status, workspace, x0)]"""
    bs = _solver(prob, B, kw, xref=xref)
    x, out = x0.copy(), []
    for k in range(steps):
        if xs is not None:
            x = xs[k]
        bs.set_x0(x)
        bs.solve()
        assert bs.last_launch_name == name, (k, bs.last_launch_name)
        sol, st, ws = bs.get_solution(), bs.get_status(), bs.get_workspace()
        out.append((sol, st, ws, x.copy()))
        x = np.asfortranarray(prob.A @ x + prob.B @ sol["controls"][:, 0, :])
    bs.close()
    return out


def _against_oracle(oracle_built, prob, kw, run, pick, tag, cap=0.03, want_exits=None, xref=None):
    """a run of _closed_loop against persistent oracles on the instances `pick`: solution and workspace at every step.
    Returns the oracles' own (iter, solved) per step and instance and the replayed share per step."""
    steps = len(run)
    own = np.zeros((steps, len(pick), 2), dtype=int)
    rep = np.zeros((steps, len(pick)), dtype=bool)
    for j, b in enumerate(pick):
        o = _oracle(oracle_built, prob, kw, xref=xref)
        for k in range(steps):
            sol, st, ws, xk = run[k]
            r, sv, own[k, j], rep[k, j] = _oracle_step(o, xk[:, b], st["iter"][b], st["solved"][b])
            ex, eu = nrel(sol["states"][:, :, b], r["x"]), nrel(sol["controls"][:, :, b], r["u"])
            assert ex <= FP32_TOL and eu <= FP32_TOL, (tag, b, k, ex, eu)
            for key in WS_KEYS:
                scale = max(np.abs(sv[key]).max(), 1e-2)
                err = np.abs(ws[key][:, :, b] - sv[key]).max()
                assert err <= _lim(key) * scale, (tag, b, k, key, err / scale, int(st["iter"][b]), int(st["solved"][b]))
        o.close()
    share = rep.mean(axis=1)
    print(f"{tag}: replayed share per step {share}")
    assert share.max() <= cap, (tag, share)
    if want_exits is not None:
        conv = own[:, :, 1].mean(axis=1)
        print(f"{tag}: converged share per step (oracle) {conv}")
        assert conv.min() >= want_exits and (1.0 - conv).min() >= want_exits, (tag, conv)   # both exits of solve() occur
    return own, share


# ---------------------------------------------------------------------------------------------------------------------------
# 3. routing
# ---------------------------------------------------------------------------------------------------------------------------
FIXED = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=10, check_termination=1)
TOL = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1)


@pytest.mark.parametrize("on", [True, False], ids=["switch_on", "switch_off"])
def test_routing(hip_lib, monkeypatch, on):
    _switch(monkeypatch, on)
    x0 = t.problems.cartpole_x0(B_G1, seed=51)
    want = LEAN if on else QUAD
    for kw in (FIXED, TOL):
        for sb in (False, True):
            prob = _cartpole(sb)
            bs = _solver(prob, B_G1, kw)
            bs.set_x0(x0)
            for refs in ("zero", "shared"):
                if refs == "shared":
                    xr = np.zeros((4, 20), order="F"); xr[0] = 0.05
                    bs.set_x_ref(xr)
                bs.solve()
                assert bs.kernel_name == QUAD and bs.last_launch_name == want, (kw, sb, refs, bs.last_launch_name)
                if on and refs == "zero":
                    assert _form(bs) == LF_SPARSE      # the default cartpole pattern: the entry's sparse kernels
                bs.solve()                             # ... and warm
                assert bs.last_launch_name == want
            bs.close()


def test_routing_out_of_scope_stays(hip_lib, monkeypatch):
    """what the lean kernel never took goes where it goes today with the switch on"""
    _switch(monkeypatch, True)
    prob, x0 = _cartpole(), t.problems.cartpole_x0(B_G1, seed=52)
    bs = _solver(prob, B_G1, TOL)
    bs.set_x0(x0)
    bs.solve()
    assert bs.last_launch_name == LEAN
    xr = np.zeros((4, 20, B_G1), order="F"); xr[0] = 0.1       # per-instance references
    bs.set_x_ref(xr)
    bs.solve()
    assert bs.last_launch_name == QUAD
    bs.set_x_ref(np.zeros((4, 20), order="F"))
    bs.solve()
    assert bs.last_launch_name == LEAN
    for p in (1, 2):                                            # fp32 recurrences; fp64 state
        bs.set_precision(p)
        bs.solve()
        assert bs.last_launch_name != LEAN, (p, bs.last_launch_name)
    bs.set_precision(0)
    bs.solve()
    assert bs.last_launch_name == LEAN
    bs.set_compaction(20)                                       # chunked / compacted solves carry an index list
    bs.solve()
    assert bs.last_launch_name == QUAD
    bs.set_compaction(0)
    bs.solve()
    assert bs.last_launch_name == LEAN
    c = bs.get_cache_terms()                                    # a cache whose AmBKt is not (A - B Kinf)'
    bs.set_cache_terms(c["Kinf"], c["Pinf"], c["Quu_inv"], c["AmBKt"] * (1.0 + 1e-6))
    bs.solve()
    assert bs.last_launch_name == QUAD
    bs.set_cache_terms(c["Kinf"], c["Pinf"], c["Quu_inv"], c["AmBKt"])
    bs.solve()
    assert bs.last_launch_name == LEAN
    bs.set_adaptive_rho(True)
    bs.solve()
    assert bs.last_launch_name != LEAN, bs.last_launch_name
    bs.close()
    # the switch is read at creation and again on request
    _switch(monkeypatch, False)
    b2 = _solver(prob, B_G1, TOL)
    b2.set_x0(x0)
    b2.solve()
    assert b2.last_launch_name == QUAD
    _switch(monkeypatch, True)
    b2.reload_switches()
    b2.solve()
    assert b2.last_launch_name == LEAN
    b2.close()


@pytest.fixture
def jit_on(monkeypatch, tmp_path_factory):
    monkeypatch.delenv("TINYMPC_HIP_NO_JIT", raising=False)
    # one cache for the whole test session (a unit is compiled once), outside the home directory
    cache = os.environ.get("TINYMPC_TEST_JIT_CACHE") or str(tmp_path_factory.getbasetemp() / "jit_cache")
    os.makedirs(cache, exist_ok=True)
    monkeypatch.setenv("TINYMPC_HIP_CACHE", os.path.abspath(cache))
    return os.path.abspath(cache)


def test_other_horizon_stays_where_it_is_without_specialisation(hip_lib, monkeypatch):
    """N = 12 has no built-in kernel of any on-chip family: with specialisation off (the suite's default) it goes where it
    goes today, without an error"""
    _switch(monkeypatch, True)
    prob, x0 = _cartpole(N=12), t.problems.cartpole_x0(B_G1, seed=53)
    bs = _solver(prob, B_G1, TOL)
    bs.set_x0(x0)
    for _ in range(2):
        bs.solve()
        assert bs.last_launch_name == bs.kernel_name == "stream4<4,1>", bs.last_launch_name
    bs.close()


def test_other_horizon_through_specialisation(hip_lib, oracle_built, monkeypatch, jit_on):
    """N = 12 has no built-in lean kernel: with specialisation on, the one WS variant the launch needs is compiled"""
    _switch(monkeypatch, True)
    prob, x0 = _cartpole(N=12), t.problems.cartpole_x0(B_RAGGED, seed=41)
    run = _closed_loop(prob, B_RAGGED, TOL, x0, 3, "lean<4,1,12>")
    _against_oracle(oracle_built, prob, TOL, run, np.r_[0:32, 20480:20480 + 33], "N=12 specialised")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. workspace parity, host-stepped closed loop
# ---------------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _loop_run(monkeypatch, ct, sb, on):
    """three warm-started solves of the protocol, cached per configuration; the switch-on run is fed the switch-off run's
    x0 sequence"""
    key = (ct, sb, on)
    if key not in _RUNS:
        prob = _cartpole(sb)
        kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=ct)
        x0 = t.problems.cartpole_x0(B_RAGGED, seed=41)
        _switch(monkeypatch, on)
        xs = None if not on else [r[3] for r in _loop_run(monkeypatch, ct, sb, False)]
        _switch(monkeypatch, on)
        _RUNS[key] = _closed_loop(prob, B_RAGGED, kw, x0, 3, LEAN if on else QUAD, xs=xs)
    return _RUNS[key]


@pytest.mark.parametrize("state_bound", [False, True], ids=["free", "state_bound"])
@pytest.mark.parametrize("ct", [1, 10])
@pytest.mark.parametrize("on", [False, True], ids=["switch_off", "switch_on"])
def test_kept_workspace_closed_loop(hip_lib, oracle_built, monkeypatch, on, ct, state_bound):
    """ragged batch 20 480 + 33, cartpole u_bound 0.5, cartpole_x0(seed=41), tolerance 1e-3, max_iter 100, three solves with
    the host applying the model in between.  switch_off is the quad kernel (the yardstick: it has to hold the same oracle
    comparison and the same 3 % cap of replayed instances on the same inputs), switch_on the lean kernel.
    Measured on an MI355X: share of the batch whose counts agree with the quad kernel's in every step so far — check
    every iteration 1.0 / 0.99976 / 0.99951 (free), 1.0 / 0.99990 / 0.99990 (state bound); check every 10: 1.0 in all
    steps; replayed share of the 289-instance oracle sample: 0 in every step, on both kernels; converged share per step by
    the oracle 0.48 / 0.54 / 0.57 (free), 0.29 / 0.32 / 0.34 (state bound)."""
    prob = _cartpole(state_bound)
    kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=ct)
    run = _loop_run(monkeypatch, ct, state_bound, on)
    tag = f"{'lean' if on else 'quad'} ct={ct} sb={state_bound}"
    _against_oracle(oracle_built, prob, kw, run, SAMPLE, tag, want_exits=0.10)
    if not on:
        return
    ref = _loop_run(monkeypatch, ct, state_bound, False)
    agree = np.ones(B_RAGGED, dtype=bool)
    for k in range(3):
        (sa, ta, wa, xa), (sb_, tb, wb, xb) = run[k], ref[k]
        assert np.array_equal(xa, xb)
        agree &= (ta["iter"] == tb["iter"]) & (ta["solved"] == tb["solved"])
        print(f"{tag}: step {k}: counts agree so far on {agree.mean():.5f} of the batch")
        assert agree.mean() >= 0.995 ** (k + 1), (k, agree.mean())
        ex, eu = nrel_batch(sa["states"], sb_["states"])[agree].max(), nrel_batch(sa["controls"], sb_["controls"])[agree].max()
        assert ex <= FP32_TOL and eu <= FP32_TOL, (k, ex, eu)
        for key in WS_KEYS:
            scale = max(np.abs(wb[key]).max(), 1e-2)
            err = np.abs(wa[key] - wb[key])[:, :, agree].max()
            assert err <= _lim(key) * scale, (k, key, err / scale)


@pytest.mark.parametrize("state_bound", [False, True], ids=["free", "state_bound"])
def test_exit_at_iteration_one_hands_back_the_loaded_workspace(hip_lib, oracle_built, monkeypatch, state_bound):
    """the same x0 solved warm twice (and a third and fourth time): an instance that converges at iteration 1 returns before
    v = vnew, z = znew and the backward pass (admm.cpp:181-193), so its v, z, d are the ones it loaded — bit for bit without
    a state bound (fp32 -> register -> fp32 is exact), within the workspace limits with one (v is re-formed as q~ + g in
    fp32) — and match the oracle's.  The first two solves are held to the whole oracle comparison on the sample (every
    instance, all five arrays); the third and fourth, where an instance that never converges has integrated 300 / 400
    iterations of fp32 rounding into its duals, to the solution and to v, z, d of the instances that leave at iteration 1.
    Measured on an MI355X (worst workspace error of the sample against the oracle, of max(|ref|, 1e-2), solves 1-4, state
    bound on): y 9.7e-6, 8.5e-6, 1.6e-5, 6.3e-5 and g 6.0e-6, 9.9e-6, 1.1e-5, 1.7e-5 — the same figures to three digits
    on the quad kernel (switch off) and on the lean kernel; v 6.5e-7 (quad) / 2.5e-6 (lean: q~ + g in fp32).  Without a
    state bound the worst array stays below 0.28 of its limit over the four solves."""
    _switch(monkeypatch, True)
    prob = _cartpole(state_bound)
    kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1)
    x0 = t.problems.cartpole_x0(B_RAGGED, seed=41)
    run = _closed_loop(prob, B_RAGGED, kw, x0, 4, LEAN, xs=[x0] * 4)
    _against_oracle(oracle_built, prob, kw, run[:2], SAMPLE, f"same x0 sb={state_bound}")
    own = np.zeros((4, len(SAMPLE), 2), dtype=int)
    worst = np.zeros(4)
    for j, b in enumerate(SAMPLE):
        o = _oracle(oracle_built, prob, kw)
        for k in range(4):
            sol, st, ws, _ = run[k]
            r, sv, own[k, j], _ = _oracle_step(o, x0[:, b], st["iter"][b], st["solved"][b])
            assert nrel(sol["states"][:, :, b], r["x"]) <= FP32_TOL and nrel(sol["controls"][:, :, b], r["u"]) <= FP32_TOL, (b, k)
            worst[k] = max(worst[k], max(np.abs(ws[key][:, :, b] - sv[key]).max() / (_lim(key) * max(np.abs(sv[key]).max(), 1e-2)) for key in WS_KEYS))
            if k >= 1 and st["iter"][b] == 1 and st["solved"][b] == 1:
                for key in ("v", "z", "d"):
                    scale = max(np.abs(sv[key]).max(), 1e-2)
                    assert np.abs(ws[key][:, :, b] - sv[key]).max() <= _lim(key) * scale, (b, k, key)
        o.close()
    print(f"same x0 sb={state_bound}: worst workspace error of the sample per solve, in units of its limit: {worst}")
    for k in range(1, 4):
        first_o = (own[k, :, 0] == 1) & (own[k, :, 1] == 1)
        print(f"solve {k + 1}: the oracle leaves at iteration 1 on {first_o.mean():.3f} of the sample")
        assert first_o.mean() >= 0.10
        st, ws, prev = run[k][1], run[k][2], run[k - 1][2]
        first = (st["iter"] == 1) & (st["solved"] == 1)
        assert first.mean() >= 0.10 and first[20480:].any()
        for key in ("v", "z", "d"):
            if not state_bound or key != "v":
                assert np.array_equal(ws[key][:, :, first], prev[key][:, :, first]), (k, key)
            else:
                scale = max(np.abs(prev[key]).max(), 1e-2)
                assert np.abs(ws[key] - prev[key])[:, :, first].max() <= _lim(key) * scale, (k, key)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. fixed-iteration kept workspace
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter,dense,state_bound", [(100, False, False), (1, False, False), (100, True, False), (1, True, False),
                                                        (100, False, True), (1, False, True)])
def test_fixed_iteration_kept_workspace(hip_lib, oracle_built, monkeypatch, max_iter, dense, state_bound):
    """tolerances 0: every instance leaves at max_iter with the last iteration's slack and the d of the backward pass behind
    it.  max_iter 1 makes the first iteration the residual iteration: knot 0 of the dual residual against the loaded v_0;
    dense sweeps (TINYMPC_HIP_LEAN_DENSE=1) reach the Hessenberg form, whose loaded v goes through x^ = T' v"""
    _switch(monkeypatch, True)
    if dense:
        monkeypatch.setenv("TINYMPC_HIP_LEAN_DENSE", "1")
    prob = _cartpole(state_bound)
    kw = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=max_iter, check_termination=1)
    x0 = t.problems.cartpole_x0(B_RAGGED, seed=41)
    bs = _solver(prob, B_RAGGED, kw)
    x, run = x0.copy(), []
    for k in range(3):
        bs.set_x0(x)
        bs.solve()
        assert bs.last_launch_name == LEAN
        assert _form(bs) == ((LF_PLAIN if state_bound else LF_HB) if dense else LF_SPARSE)
        sol, st, ws = bs.get_solution(), bs.get_status(), bs.get_workspace()
        assert np.all(st["iter"] == max_iter) and not st["solved"].any()
        run.append((sol, st, ws, x.copy()))
        x = np.asfortranarray(prob.A @ x + prob.B @ sol["controls"][:, 0, :])
    bs.close()
    own, share = _against_oracle(oracle_built, prob, kw, run, SAMPLE, f"fixed {max_iter} dense={dense} sb={state_bound}", cap=0.0)
    # residuals as the reference reports them, from a loaded workspace (the last check's values): on the sample
    o = _oracle(oracle_built, prob, kw)
    for k in range(3):
        o.set_x0(run[k][3][:, 7])
        o.solve()
        r = o.get_solution()
        dres = np.abs(run[k][1]["residuals"][7] - r["res"]) / np.maximum(1.0, np.abs(r["res"]))
        assert dres.max() <= FP32_TOL, (k, dres)
    o.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5b. the other calling patterns the lean kernel takes: per-knot input bounds, shared references, a workspace whose state dual
#     is not zero while no state bound is active
# ---------------------------------------------------------------------------------------------------------------------------
FIXED30 = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=30, check_termination=1)
SMALL = np.r_[0:48, 20480:20480 + 33]


@pytest.mark.parametrize("case,kw", [("knot_bounds", TOL), ("knot_bounds", FIXED30), ("shared_refs", TOL), ("shared_refs", FIXED30),
                                     ("state_bound+shared_refs", TOL), ("knot_bounds+state_bound+shared_refs", FIXED30),
                                     ("knot_bounds+state_bound+shared_refs", TOL)],
                         ids=lambda v: v if isinstance(v, str) else ("tol" if v["abs_pri_tol"] > 0 else "fixed"))
def test_other_calling_patterns_kept_workspace(hip_lib, oracle_built, monkeypatch, case, kw):
    """three warm solves of a host-stepped loop against persistent oracles, workspace included: input bounds that differ from
    knot to knot (read from LDS knot by knot), a shared state reference (reference terms from LDS), both with a state bound —
    the fixed-iteration case of all three is the one the launcher sends to the tolerance-terminated kernel of the same flags"""
    _switch(monkeypatch, True)
    prob = _cartpole("state_bound" in case)
    if "knot_bounds" in case:
        rng = np.random.default_rng(5)
        prob.u_max = np.asfortranarray(0.2 + 0.5 * rng.random((1, 19)))
        prob.u_min = np.asfortranarray(-(0.2 + 0.5 * rng.random((1, 19))))
    xref = None
    if "shared_refs" in case:
        xref = np.zeros((4, 20), order="F")
        xref[0] = 0.05
    x0 = t.problems.cartpole_x0(B_RAGGED, seed=41)
    run = _closed_loop(prob, B_RAGGED, kw, x0, 3, LEAN, xref=xref)
    _against_oracle(oracle_built, prob, kw, run, SMALL, f"{case} {'tol' if kw['abs_pri_tol'] > 0 else 'fixed'}", xref=xref)
    if kw["abs_pri_tol"] == 0:
        assert all(np.all(r[1]["iter"] == kw["max_iter"]) and not r[1]["solved"].any() for r in run)


def test_state_dual_left_by_a_lifted_state_bound(hip_lib, oracle_built, monkeypatch):
    """two solves with a state bound, then the bound is lifted and the loop goes on warm: the workspace's g is not zero, so
    the launch takes the state-bounded form (whose clamps then clamp nothing) instead of dropping it"""
    _switch(monkeypatch, True)
    bound, free = _cartpole(True), _cartpole(False)
    x0 = t.problems.cartpole_x0(B_RAGGED, seed=41)
    bs = _solver(bound, B_RAGGED, TOL)
    oracles = [_oracle(oracle_built, bound, TOL) for _ in SMALL]
    x, replayed = x0.copy(), 0
    for k in range(4):
        if k == 2:
            bs.set_bound_constraints(free.x_min, free.x_max, free.u_min, free.u_max)
            for o in oracles:
                o.set_bound_constraints(free.x_min, free.x_max, free.u_min, free.u_max)
        bs.set_x0(x)
        bs.solve()
        assert bs.last_launch_name == LEAN
        sol, st, ws = bs.get_solution(), bs.get_status(), bs.get_workspace()
        if k == 1:
            assert np.abs(ws["g"]).max() > 1e-4                 # (what the next solve loads: its first iteration forms vnew = x + g)
        for o, b in zip(oracles, SMALL):
            r, sv, _, rep = _oracle_step(o, x[:, b], st["iter"][b], st["solved"][b])
            replayed += rep
            assert nrel(sol["states"][:, :, b], r["x"]) <= FP32_TOL and nrel(sol["controls"][:, :, b], r["u"]) <= FP32_TOL, (k, b)
            for key in WS_KEYS:
                scale = max(np.abs(sv[key]).max(), 1e-2)
                assert np.abs(ws[key][:, :, b] - sv[key]).max() <= _lim(key) * scale, (k, b, key)
        x = np.asfortranarray(free.A @ x + free.B @ sol["controls"][:, 0, :])
    assert replayed <= 0.03 * 4 * len(SMALL)
    for o in oracles:
        o.close()
    bs.close()


def test_horizon_beyond_the_lds_budget_stays_on_quad(hip_lib, monkeypatch, jit_on):
    """N = 30, tolerance-terminated: the parked slack would need 202 KB of LDS.  No unit is compiled for it; the solves and
    the closed loop stay on the quad kernel"""
    import glob
    _switch(monkeypatch, True)
    prob, x0 = _cartpole(N=30), t.problems.cartpole_x0(B_G1, seed=54)
    bs = _solver(prob, B_G1, dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=10, check_termination=1))
    bs.set_x0(x0)
    for _ in range(2):
        bs.solve()
        assert bs.last_launch_name == "quad<4,1,30,g1>", bs.last_launch_name
    bs.mpc_rollout(3)
    assert bs.last_launch_name == "quad<4,1,30,g1>"
    ws_units = [f for f in glob.glob(os.path.join(jit_on, "*", "lean_4_1_30_v*")) if int(os.path.basename(f).split("_v")[1].split("_")[0].split(".")[0]) & 128]
    assert not ws_units, ws_units
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the golden loops inside a full batch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["G5_cartpole_mpc_warm", "G5b_cartpole_mpc_warm_bounded"])
def test_golden_loop_inside_a_batch(hip_lib, monkeypatch, name):
    """instance 0 and one instance of the ragged wavefront follow the fixture's x0 sequence, the rest random ones: iter,
    solved, solution at FP32_TOL (test_golden_mpc_warm_start's bar) and state_after at FP32_TOL of max(|ref|, 1e-2)
    (test_golden_mpc_workspace_state's bar), for both fixtures.  The worst error per array is printed before it is
    asserted."""
    _switch(monkeypatch, True)
    g = load_golden(name)
    prob = problem_of(g)
    nx, nu, N = prob.nx, prob.nu, prob.N
    who = [0, 20480 + 17]
    worst = {key: 0.0 for key in WS_KEYS}
    bs = _solver(prob, B_RAGGED, g["settings"])
    for k, step in enumerate(g["steps"]):
        x = t.problems.cartpole_x0(B_RAGGED, seed=100 + k)
        for b in who:
            x[:, b] = np.array(step["x0"])
        bs.set_x0(x)
        bs.solve()
        assert bs.last_launch_name == LEAN
        sol, st, ws = bs.get_solution(), bs.get_status(), bs.get_workspace()
        for b in who:
            assert int(st["iter"][b]) == step["iter"] and int(st["solved"][b]) == step["solved"], (k, b)
            assert nrel(sol["states"][:, :, b], cm(step["x"], nx, N)) <= FP32_TOL, (k, b)
            assert nrel(sol["controls"][:, :, b], cm(step["u"], nu, N - 1)) <= FP32_TOL, (k, b)
            for key, r, c in (("d", nu, N - 1), ("y", nu, N - 1), ("z", nu, N - 1), ("g", nx, N), ("v", nx, N)):
                ref = cm(step["state_after"][key], r, c)
                scale = max(np.abs(ref).max(), 1e-2)
                worst[key] = max(worst[key], np.abs(ws[key][:, :, b] - ref).max() / scale)
    bs.close()
    print(f"{name}: worst state_after error per array over all steps, of max(|ref|, 1e-2): " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for key, v in worst.items():
        assert v <= FP32_TOL, f"{name} {key}: {v:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# 7. mpc_rollout
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle_rollout(oracle_built, prob, kw, x0, steps, b, forced=None):
    o = _oracle(oracle_built, prob, kw)
    x = x0[:, b].copy()
    u, xs, it, so = np.zeros((prob.nu, steps)), np.zeros((prob.nx, steps)), np.zeros(steps, dtype=int), np.zeros(steps, dtype=int)
    for k in range(steps):
        if forced is not None:
            o.set_forced_exit(int(forced[k][0]) if forced[k][1] else -1)
        o.set_x0(x)
        o.solve()
        r = o.get_solution()
        x = prob.A @ x + prob.B @ r["u"][:, 0]
        u[:, k], xs[:, k], it[k], so[k] = r["u"][:, 0], x, r["iter"], r["solved"]
    fin = (o.get_solution(), o.get_state())
    o.close()
    return u, xs, it, so, fin


def _rollout_vs_oracle(oracle_built, prob, kw, x0, steps, bs, log, pick, tag):
    sol, ws = bs.get_solution(), bs.get_workspace()
    n_same, first_exit = 0, 0
    for b in pick:
        u, xs, it, so, fin = _oracle_rollout(oracle_built, prob, kw, x0, steps, b)
        first_exit += int(np.any((it == 1) & (so == 1)))
        same = np.array_equal(it, log["iter"][:, b]) and np.array_equal(so, log["solved"][:, b])
        n_same += same
        if not same:
            assert np.abs(log["iter"][:, b] - it).max() <= kw["max_iter"]
            u, xs, it, so, fin = _oracle_rollout(oracle_built, prob, kw, x0, steps, b,
                                                 [(log["iter"][k, b], log["solved"][k, b]) for k in range(steps)])
            assert np.array_equal(it, log["iter"][:, b]) and np.array_equal(so, log["solved"][:, b])
        eu = np.abs(log["u"][:, :, b] - u).max() / np.abs(u).max()
        ex = np.abs(log["x"][:, :, b] - xs).max() / np.abs(xs).max()
        assert eu <= FP32_TOL and ex <= FP32_TOL, (tag, b, eu, ex)
        r, sv = fin
        assert nrel(sol["states"][:, :, b], r["x"]) <= FP32_TOL and nrel(sol["controls"][:, :, b], r["u"]) <= FP32_TOL, (tag, b)
        for key in WS_KEYS:
            scale = max(np.abs(sv[key]).max(), 1e-2)
            assert np.abs(ws[key][:, :, b] - sv[key]).max() <= _lim(key) * scale, (tag, b, key)
    print(f"{tag}: {n_same} of {len(pick)} sampled closed loops took the oracle's own iteration counts; {first_exit} contain an exit at iteration 1")
    assert n_same >= 0.9 * len(pick)
    return first_exit


def test_mpc_rollout_chain(hip_lib, oracle_built, monkeypatch):
    """test_fused_mpc_rollout_batch_vs_oracle's cartpole case at batch 24 576: a stream-ordered chain of workspace-carrying
    lean launches and plant updates (plant state in fp64) — against the oracle loop on a sample, and against the quad
    kernel's fused in-kernel loop on every instance whose iteration counts agree in all steps"""
    prob = _cartpole(u_bound=0.8)
    kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=10, check_termination=1)
    steps, x0 = 15, t.problems.cartpole_x0(B_G1, seed=31)
    _switch(monkeypatch, True)
    bs = _solver(prob, B_G1, kw)
    bs.set_x0(x0)
    log = bs.mpc_rollout(steps)
    assert bs.kernel_name == QUAD and bs.last_launch_name == LEAN
    _rollout_vs_oracle(oracle_built, prob, kw, x0, steps, bs, log, np.r_[0:24, 12000:12012, B_G1 - 12:B_G1], "15 steps")
    _switch(monkeypatch, False)
    bq = _solver(prob, B_G1, kw)
    bq.set_x0(x0)
    logq = bq.mpc_rollout(steps)
    assert bq.last_launch_name == QUAD
    agree = np.all((logq["iter"] == log["iter"]) & (logq["solved"] == log["solved"]), axis=0)
    print(f"chain vs fused loop: iteration counts agree in all steps on {agree.mean():.4f} of the batch")
    assert agree.mean() >= 0.9
    den_u, den_x = np.abs(logq["u"]).max(axis=(0, 1)), np.abs(logq["x"]).max(axis=(0, 1))
    eu = (np.abs(log["u"] - logq["u"]).max(axis=(0, 1)) / den_u)[agree].max()
    ex = (np.abs(log["x"] - logq["x"]).max(axis=(0, 1)) / den_x)[agree].max()
    assert eu <= FP32_TOL and ex <= FP32_TOL, (eu, ex)
    bs.close(); bq.close()


def test_mpc_rollout_chain_sixty_steps(hip_lib, oracle_built, monkeypatch):
    """the loop itself reaches the exit at iteration 1 only late (the plant has settled): 60 steps, oracle sample only"""
    prob = _cartpole(u_bound=0.8)
    kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=10, check_termination=1)
    steps, x0 = 60, t.problems.cartpole_x0(B_G1, seed=41)
    _switch(monkeypatch, True)
    bs = _solver(prob, B_G1, kw)
    bs.set_x0(x0)
    log = bs.mpc_rollout(steps)
    assert bs.last_launch_name == LEAN
    first_exit = _rollout_vs_oracle(oracle_built, prob, kw, x0, steps, bs, log, np.arange(256), "60 steps")
    assert first_exit >= 1, "the sample holds no closed loop with an exit at iteration 1"
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. a solver goes back and forth
# ---------------------------------------------------------------------------------------------------------------------------
def test_back_and_forth(hip_lib, monkeypatch):
    _switch(monkeypatch, True)
    prob, x0 = _cartpole(), t.problems.cartpole_x0(B_G1, seed=15)
    bs = _solver(prob, B_G1, FIXED, warm=False)
    bs.set_x0(x0)
    bs.solve()
    assert bs.last_launch_name == LEAN
    base = bs.get_solution()
    bs.set_warm_start(True)
    bs.reset()
    bs.solve()                                                  # a zero workspace: the cold result
    assert bs.last_launch_name == LEAN
    warm = bs.get_solution()
    assert nrel_batch(warm["controls"], base["controls"]).max() <= 4e-6 and nrel_batch(warm["states"], base["states"]).max() <= 4e-6
    for _ in range(2):
        bs.solve()
        assert bs.last_launch_name == LEAN
    later = bs.get_solution()
    assert not np.array_equal(later["controls"], base["controls"])   # (twenty more iterations on the kept workspace)
    bs.set_warm_start(False)
    bs.solve()
    assert bs.last_launch_name == LEAN
    again = bs.get_solution()
    assert np.array_equal(again["controls"], base["controls"]) and np.array_equal(again["states"], base["states"])
    bs.close()
