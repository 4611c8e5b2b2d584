"""Cone coefficients PER INSTANCE (tinympc_set_instance_cones): the `ic` form of the stream kernel on the benchmark shapes, of the
generic kernel elsewhere, through tinympc.py.

Batch 70: four lanes per instance make that two stream workgroups, the second ragged with 6 live instances.  The base case is
tests/test_instance_bounds_gpu.py's `rocket_cones`: the rocket at N = 12 (no on-chip entry, so the shared-cones arm of a
comparison runs on the stream kernel too) with the affine term, references and one cone a side, `([0], [3], mu_u, [0], [3], mu_x)`,
max_iter 40, tolerances 1e-3, a check every iteration.

 1 equal coefficients, equal bits   (a) with per-instance rows against the `il` form with those rows and the shared cones, (b) without
                                    rows against the plain stream kernel with the shared cones: x, u, status, residuals, workspace
 2 oracle, every instance           one orc64 CpuSolver per instance with that instance's coefficients; alone, beside per-instance
                                    bounds, beside per-instance rows, on per-instance families
 3 absent cones                     mu = +inf on the device is a cone left out of that instance's oracle cone list
 4 compaction                       the coefficients are indexed by the instance, not by the launch's dense slot
 5 generic fallback                 a shape outside the stream grid, precision 1 and precision 2
 6 routing and refusals             7 closed loop (both chains)       8 sharded       9 process-global entry

The coefficient recipe of 2 (fp32 values: the oracle and the device hold the same numbers): rng = default_rng(4), mu_u =
round(uniform(0.05, 0.3, B) 64) / 64, then mu_x = round(uniform(0.1, 0.5, B) 64) / 64.  That they bite is asserted on the ORACLE's
results alone, before the device is compared: at least half the instances differ by more than 1e-3 (nrel) from their solution
under the shared (0.25, 0.5) and from their solution under their neighbour's coefficients.
Every test fails without the feature (BatchSolver.set_instance_cones does not exist there)."""
import ctypes

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.test_instance_bounds_gpu import (B, ROCKET_CONES, TOL_KW, _bounds, _case, _f32, _identical, _knots, _model, _oracle_solves,
                                            _results, _solver)
from tests.test_instance_rows_gpu import _plain_rows, _rows
from tests.util import FP32_TOL, nrel_batch, parity_every_instance, precision1_limit

pytestmark = pytest.mark.gpu

TIGHT = 1e-6        # tests/test_precision2_gpu.py: generic<f64> against the oracle fed the same fp32 inputs
LAYOUT = ([0], [3], [0], [3])      # Acu, qcu, Acx, qcx of the base case
INF = float("inf")
c_ip = ctypes.POINTER(ctypes.c_int)


# ---------------------------------------------------------------------------------------------------------------------------
# cases, coefficients, oracles
# ---------------------------------------------------------------------------------------------------------------------------
def _cone_case(batch=B, N=12, families=False):
    """`rocket_cones` without its shared cones: the affine term and the references stay the case's extension"""
    case = _case("rocket_cones", batch)
    prob = case["prob"] = t.problems.rocket(N)
    xr, ur = t.problems.rocket_refs(N)

    def ext(o):
        o.set_fdyn(prob.fdyn)
        o.set_x_ref(xr)
        o.set_u_ref(ur)
    case["ext"] = ext
    if families:
        rng = np.random.default_rng(3)
        A = np.repeat(prob.A[:, :, None], batch, axis=2) * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, (6, 6, batch)))
        Bm = np.repeat(prob.B[:, :, None], batch, axis=2) * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, (6, 3, batch)))
        Q = np.repeat(prob.Q[:, :, None], batch, axis=2)
        R = np.repeat(prob.R[:, :, None], batch, axis=2)
        case["fam"] = tuple(np.asfortranarray(m) for m in (A, Bm, Q, R)) + (np.full(batch, prob.rho),)
    return case


def _mu(batch=B):
    rng = np.random.default_rng(4)
    mu_u = np.round(rng.uniform(0.05, 0.3, batch) * 64.0) / 64.0
    mu_x = np.round(rng.uniform(0.1, 0.5, batch) * 64.0) / 64.0
    return mu_u[None, :], mu_x[None, :]


def _make_oracle(oracle, case, layout, cu, cx, kw=None, shift=0, kind="orc64", bounds=None, rows=None):
    """make_oracle(b) of parity_every_instance: a cold solver with the cones instance (b + shift) % B has (mu = +inf: left out),
    its own bounds and non-absent rows where given"""
    prob = case["prob"]
    Acu, qcu, Acx, qcx = layout
    cu, cx = np.asarray(cu, dtype=np.float64), np.asarray(cx, dtype=np.float64)

    def make(b):
        o = oracle.CpuSolver(kind, *_model(case, b), prob.N)
        o.update_settings(**(kw or case["kw"]))
        if bounds is None:
            o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        else:
            o.set_bound_constraints(*[_knots(a, prob.N - (i >= 2))[:, :, b] for i, a in enumerate(bounds)])
        if "ext" in case:
            case["ext"](o)
        j = (b + shift) % (cu.shape[1] if cu.size else cx.shape[1])
        ku = [i for i in range(len(Acu)) if np.isfinite(cu[i, j])]
        kx = [i for i in range(len(Acx)) if np.isfinite(cx[i, j])]
        o.set_cone_constraints([Acu[i] for i in ku], [qcu[i] for i in ku], [cu[i, j] for i in ku],
                               [Acx[i] for i in kx], [qcx[i] for i in kx], [cx[i, j] for i in kx])
        if rows is not None:
            Ax, bx, Au, bu = rows
            rx, ru = np.abs(Ax[:, :, b]).sum(axis=1) > 0, np.abs(Au[:, :, b]).sum(axis=1) > 0
            o.set_linear_constraints(Ax[rx, :, b].reshape(-1, prob.nx), bx[rx, b], Au[ru, :, b].reshape(-1, prob.nu), bu[ru, b])
        return o
    return make


def _differ(a, c):
    return np.maximum(nrel_batch(a["x"], c["x"]), nrel_batch(a["u"], c["u"])) > 1e-3


def _coefficients_bite(oracle, case, cu, cx, ref, tag, **extra):
    """on the oracle alone: at least half the instances differ from the shared (0.25, 0.5) and from their neighbour's coefficients"""
    Bn = case["x0"].shape[1]
    shared = _oracle_solves(_make_oracle(oracle, case, LAYOUT, np.full((1, Bn), 0.25), np.full((1, Bn), 0.5), **extra), [case["x0"]])
    nb = _oracle_solves(_make_oracle(oracle, case, LAYOUT, cu, cx, shift=1, **extra), [case["x0"]])
    d_sh, d_nb = _differ(ref, shared), _differ(ref, nb)
    print(f"{tag}: {int(d_sh.sum())} of {Bn} differ from the shared coefficients, {int(d_nb.sum())} from the neighbour's; "
          f"{int(ref['solved'].sum())} converged, iterations {ref['iter'].min()}..{ref['iter'].max()}")
    assert d_sh.sum() >= Bn / 2, f"{tag}: only {int(d_sh.sum())} of {Bn} instances differ from their solution under the shared (0.25, 0.5)"
    assert d_nb.sum() >= Bn / 2, f"{tag}: only {int(d_nb.sum())} of {Bn} instances differ from the solution under their neighbour's coefficients"


def _ic_solver(case, cu, cx, layout=LAYOUT, precision=0):
    bs = _solver(case, precision=precision)
    bs.set_instance_cones(layout[0], layout[1], cu, layout[2], layout[3], cx)
    return bs


# ---------------------------------------------------------------------------------------------------------------------------
# 1. equal coefficients, equal bits
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [True, False], ids=["30_iterations", "tolerance"])
@pytest.mark.parametrize("rows", [True, False], ids=["with_rows", "without_rows"])
def test_equal_coefficients_equal_bits(hip_lib, monkeypatch, rows, fixed):
    # (the shared-cones arm without rows is the stream kernel's: a one-shot solve of this case would otherwise go to the LDS-resident
    # matrix-core kernel, a kept-workspace one to a transposed-sets unit specialised at setup — another algorithm's schedule)
    monkeypatch.setenv("TINYMPC_HIP_NO_MFMAC", "1")
    monkeypatch.setenv("TINYMPC_HIP_NO_JIT", "1")
    case = _cone_case()
    x0 = case["x0"]
    case["kw"] = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=30, check_termination=1) if fixed else dict(TOL_KW, max_iter=30)
    lin = _plain_rows(case) if rows else None
    cu, cx = np.full((1, B), ROCKET_CONES[2][0]), np.full((1, B), ROCKET_CONES[5][0])
    x0b = _f32(0.9 * x0)
    runs = {}
    for arm in ("none", "shared", "ic"):
        bs = _solver(case)
        if lin is not None:
            bs.set_instance_linear(*lin)
        if arm == "shared":
            bs.set_cone_constraints(*ROCKET_CONES)
        elif arm == "ic":
            bs.set_instance_cones(LAYOUT[0], LAYOUT[1], cu, LAYOUT[2], LAYOUT[3], cx)
        assert bs.cone_mode() == (1 if arm == "ic" else 0) and bs.lin_mode() == (1 if rows else 0)
        want = "stream4<6,3;ic>" if arm == "ic" else ("stream4<6,3;il>" if rows else "stream4<6,3>")
        out = []
        bs.set_warm_start(False)                 # one-shot
        bs.set_x0(x0)
        bs.solve()
        assert bs.kernel_name == want and bs.last_launch_name == want, (arm, bs.kernel_name, bs.last_launch_name)
        out.append(_results(bs, workspace=False))
        if arm != "none":
            bs.set_warm_start(True)              # two consecutive kept-workspace solves
            bs.reset()
            bs.solve()
            out.append(_results(bs))
            bs.set_x0(x0b)
            bs.solve()
            assert bs.last_launch_name == want
            out.append(_results(bs))
        bs.close()
        runs[arm] = out
    assert runs["shared"][0]["st"]["iter"].max() > 1
    assert not np.array_equal(runs["none"][0]["sol"]["controls"], runs["shared"][0]["sol"]["controls"]), "the shared cones decide nothing"
    for j, what in enumerate(("one-shot", "kept workspace, first", "kept workspace, second")):
        _identical(runs["shared"][j], runs["ic"][j], f"rows {rows}, {what}")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. oracle, every instance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beside", ["alone", "bounds", "rows", "families"])
def test_oracle_every_instance(hip_lib, oracle_built, beside):
    case = _cone_case(families=beside == "families")
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    cu, cx = _mu()
    extra = {}
    if beside == "bounds":
        extra["bounds"] = _bounds(case, per_knot=False)
    if beside == "rows":
        free = _oracle_solves(_make_oracle(oracle_built, case, LAYOUT, cu, cx), [x0])
        extra["rows"] = _rows(case, free)
    make = _make_oracle(oracle_built, case, LAYOUT, cu, cx, **extra)
    ref = _oracle_solves(make, [x0])
    _coefficients_bite(oracle_built, case, cu, cx, ref, beside, **extra)
    rho = float(np.max(case["fam"][4])) if "fam" in case else prob.rho
    bs = _ic_solver(case, cu, cx)
    if beside == "bounds":
        bs.set_instance_bounds(*extra["bounds"])
    if beside == "rows":
        bs.set_instance_linear(*extra["rows"])
    assert bs.cone_mode() == 1 and bs.kernel_name == "stream4<6,3;ic>"
    assert bs.bounds_mode() == (1 if beside == "bounds" else 0) and bs.lin_mode() == (1 if beside == "rows" else 0)
    bs.set_warm_start(False)
    bs.set_x0(x0)
    bs.solve()
    assert bs.last_launch_name == "stream4<6,3;ic>"
    same = parity_every_instance(bs.get_solution(), bs.get_status(), ref, make, x0, kw, rho, tag=beside + ", cold")
    print(f"{beside}: cold, {same:.2f} of the iteration counts are the oracle's")
    if beside == "alone":
        # the second solve of a warm pair from a shifted x0; the first solve's exits are the GPU's own on both sides
        x1 = _f32(0.9 * x0)
        bs.set_warm_start(True)
        bs.reset()
        bs.solve()
        st0 = bs.get_status()
        bs.set_x0(x1)
        bs.solve()
        assert bs.last_launch_name == "stream4<6,3;ic>"
        first = (st0["iter"], st0["solved"])
        ref1 = _oracle_solves(make, [x0, x1], forced_first=first)

        def make_warm(b):
            o = make(b)
            o.set_forced_exit(int(first[0][b]) if first[1][b] else -1)
            o.set_x0(x0[:, b])
            o.solve()
            o.set_forced_exit(0)
            return o
        parity_every_instance(bs.get_solution(), bs.get_status(), ref1, make_warm, x1, kw, rho, tag="warm pair, second")
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. absent cones
# ---------------------------------------------------------------------------------------------------------------------------
def test_absent_cones(hip_lib, oracle_built):
    """one input cone and two state cones (rows 0..2 and 3..5); mu row 0 is the input cone's, rows 1 and 2 the state cones'.
    Instance b keeps both state cones (b % 3 == 0), only the first (1) or only the second (2)."""
    case = _cone_case()
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    layout = ([0], [3], [0, 3], [3, 3])
    mu = np.round(np.random.default_rng(5).uniform(0.05, 0.4, (3, B)) * 64.0) / 64.0
    cu, both = mu[:1], mu[1:]
    cx = both.copy()
    cx[1, np.arange(B) % 3 == 1] = INF
    cx[0, np.arange(B) % 3 == 2] = INF
    lacks = np.arange(B) % 3 != 0
    make = _make_oracle(oracle_built, case, layout, cu, cx)
    ref = _oracle_solves(make, [x0])
    full = _oracle_solves(_make_oracle(oracle_built, case, layout, cu, both), [x0])
    d = _differ(ref, full) & lacks
    print(f"absent cones: {int(d.sum())} of the {int(lacks.sum())} instances with an absent cone differ from their both-cones solution")
    assert d.sum() >= lacks.sum() / 2
    bs = _ic_solver(case, cu, cx, layout)
    assert bs.kernel_name == "stream4<6,3;ic>"
    bs.set_warm_start(False)
    bs.set_x0(x0)
    bs.solve()
    sol, st = bs.get_solution(), bs.get_status()
    bs.close()
    assert np.isfinite(sol["states"]).all() and np.isfinite(sol["controls"]).all() and np.isfinite(st["residuals"]).all()
    parity_every_instance(sol, st, ref, make, x0, kw, prob.rho, tag="absent cones")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. compaction: instance index against dense slot
# ---------------------------------------------------------------------------------------------------------------------------
def test_compaction_indexes_coefficients_by_instance(hip_lib):
    Bn = 200
    case = _cone_case(batch=Bn)
    spread = np.linspace(0.05, 1.5, Bn)[np.random.default_rng(4).permutation(Bn)]       # iteration counts range widely
    x0 = case["x0"] = _f32(t.problems.rocket_x0(Bn, seed=7) * spread[None, :])
    case["kw"] = dict(TOL_KW, max_iter=60)
    cu, cx = _mu(Bn)
    runs = []
    for chunk in (0, 4):
        bs = _ic_solver(case, cu, cx)
        bs.set_compaction(chunk)
        bs.set_x0(x0)
        bs.solve()
        assert bs.last_launch_name == "stream4<6,3;ic>"
        runs.append(_results(bs))
        bs.close()
    it, so = runs[0]["st"]["iter"], runs[0]["st"]["solved"]
    print(f"compaction: {int(so.sum())} of {Bn} converged, {len(np.unique(it))} different iteration counts")
    assert len(np.unique(it)) > 4 and 0 < so.sum(), "the chunks compact nothing"
    _identical(runs[0], runs[1], "single launch against chunks of 4 iterations")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. generic fallback
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [1, 2], ids=["precision1", "precision2"])
def test_generic_fallback(hip_lib, oracle_built, precision):
    case = _case("odd52")
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    prob.u_min, prob.u_max = _f32(prob.u_min), _f32(prob.u_max)      # (0.6 is no fp32 value: the oracle gets what the device holds)
    layout = ([0], [2], [0], [3])                                    # one cone a side: inputs (0, 1), states (0, 1, 2)
    rng = np.random.default_rng(4)
    cu = (np.round(rng.uniform(0.3, 1.5, B) * 64.0) / 64.0)[None, :]
    cx = (np.round(rng.uniform(0.3, 1.5, B) * 64.0) / 64.0)[None, :]
    make = _make_oracle(oracle_built, case, layout, cu, cx)
    ref = _oracle_solves(make, [x0])
    nb = _oracle_solves(_make_oracle(oracle_built, case, layout, cu, cx, shift=1), [x0])
    assert _differ(ref, nb).sum() >= B / 2, "the coefficients decide nothing"
    want = "generic<f64;ic>" if precision == 2 else "generic<ic>"
    bs = _ic_solver(case, cu, cx, layout, precision=precision)
    assert bs.kernel_name == want and bs.cone_mode() == 1
    bs.set_warm_start(False)
    bs.set_x0(x0)
    bs.solve()
    assert bs.last_launch_name == want
    sol, st = bs.get_solution(), bs.get_status()
    bs.close()
    if precision == 2:
        assert np.array_equal(st["iter"], ref["iter"]) and np.array_equal(st["solved"], ref["solved"])
        ex, eu = nrel_batch(sol["states"], ref["x"]).max(), nrel_batch(sol["controls"], ref["u"]).max()
        print(f"precision 2: worst states {ex:.3e}, controls {eu:.3e}")
        assert ex <= TIGHT and eu <= TIGHT
    else:
        # the bar of an all-fp32 kernel, from the reference model alone: orc32 against orc64 on these very problems
        r32 = _oracle_solves(_make_oracle(oracle_built, case, layout, cu, cx, kind="orc32"), [x0])
        limit, e32, share = precision1_limit(r32, ref)
        print(f"precision 1: limit {limit:.3e} (orc32 against orc64 {e32:.3e}, {share:.2f} of the instances agree on the exit)")
        parity_every_instance(sol, st, ref, make, x0, kw, prob.rho, tol=limit, tag="precision 1")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. routing and refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_routing_round_trip_and_refusals(hip_lib, monkeypatch):
    monkeypatch.delenv("TINYMPC_HIP_STREAM_MPC", raising=False)
    case = _cone_case(N=10)
    x0 = case["x0"]
    cu, cx = _mu()
    ic = (LAYOUT[0], LAYOUT[1], cu, LAYOUT[2], LAYOUT[3], cx)

    def run(bs):
        bs.set_x0(x0)
        bs.solve()
        return _results(bs, workspace=False)
    stay = _solver(case)
    stay.set_cone_constraints(*ROCKET_CONES)
    home = stay.kernel_name
    assert home == "mfmat<6,3,10>", home
    r_stay = run(stay)
    home_launch = stay.last_launch_name
    stay.close()
    bs = _solver(case)
    bs.set_cone_constraints(*ROCKET_CONES)
    assert bs.kernel_name == home and bs.cone_mode() == 0
    bs.set_instance_cones(*ic)
    assert bs.kernel_name == "stream4<6,3;ic>" and bs.cone_mode() == 1
    r_ic = run(bs)
    assert bs.last_launch_name == "stream4<6,3;ic>"
    assert not np.array_equal(r_ic["sol"]["controls"], r_stay["sol"]["controls"])
    # refused, each with a message; the solver stays as it was
    with pytest.raises(t.TinyMPCError, match="at most 8 cones"):
        bs.set_instance_cones(None, None, None, [0] * 9, [2] * 9, np.ones((9, B)))
    one = (np.zeros(1, dtype=np.int32), np.full(1, 3, dtype=np.int32))
    with pytest.raises(t.TinyMPCError, match="null layout or coefficients"):
        bs._chk(bs.lib.tinympc_set_instance_cones(bs.h, None, None, None, 0, one[0].ctypes.data_as(c_ip), one[1].ctypes.data_as(c_ip),
                                                  None, 1), "set_instance_cones")
    for bad in (0.0, -0.25, float("nan"), -INF):
        worse = cx.copy()
        worse[0, B - 1] = bad
        with pytest.raises(t.TinyMPCError, match="mu must be positive and finite"):
            bs.set_instance_cones(LAYOUT[0], LAYOUT[1], cu, LAYOUT[2], LAYOUT[3], worse)
    with pytest.raises(t.TinyMPCError, match="per-instance cones"):
        bs.set_adaptive_rho(True)
    with pytest.raises(t.TinyMPCError, match="per-instance cones have no closed loop"):
        bs.mpc_rollout(2)
    assert bs.cone_mode() == 1 and bs.kernel_name == "stream4<6,3;ic>"
    bs.reset()
    _identical(r_ic, run(bs), "after the refusals")
    # enable_cones off then on: no new upload, the same bits; off, the cones do not act
    bs.reset()
    bs.enable_cones(0, 0)
    assert bs.cone_mode() == 1
    r_off = run(bs)
    bs.enable_cones(1, 1)
    bs.reset()
    _identical(r_ic, run(bs), "enable_cones off then on")
    assert not np.array_equal(r_off["sol"]["controls"], r_ic["sol"]["controls"])
    # set_precision keeps the coefficients: the generic form at precision 2, the same stream bits back at precision 0
    bs.set_precision(2)
    assert bs.cone_mode() == 1
    r_64 = run(bs)                  # (the route is decided at the solve)
    assert bs.kernel_name == "generic<f64;ic>" and bs.last_launch_name == "generic<f64;ic>"
    assert np.isfinite(r_64["sol"]["controls"]).all() and not np.array_equal(r_64["sol"]["controls"], r_off["sol"]["controls"])
    bs.set_precision(0)
    assert bs.cone_mode() == 1
    bs.reset()
    _identical(r_ic, run(bs), "precision 2 and back")
    assert bs.kernel_name == "stream4<6,3;ic>" and bs.last_launch_name == "stream4<6,3;ic>"
    # the shared entry point drops them: back home, and to the bits of a solver that never left
    bs.set_cone_constraints(*ROCKET_CONES)
    assert bs.kernel_name == home and bs.cone_mode() == 0
    bs.reset()
    r_back = run(bs)
    assert bs.last_launch_name == home_launch
    _identical(r_stay, r_back, "after the round trip")
    bs.close()
    # ... and in the other order: per-instance cones on a solver that already adapts rho
    ad = _solver(case)
    ad.set_adaptive_rho(True)
    with pytest.raises(t.TinyMPCError, match="adaptive rho"):
        ad.set_instance_cones(*ic)
    assert ad.cone_mode() == 0
    ad.close()
    # per-instance families: precision 2 and adaptive rho are refused as without the cones
    fam = _cone_case(N=10, families=True)
    hs = _ic_solver(fam, cu, cx)
    assert hs.kernel_name == "stream4<6,3;ic>" and hs.cone_mode() == 1
    with pytest.raises(t.TinyMPCError, match="per-instance-family"):
        hs.set_adaptive_rho(True)
    with pytest.raises(t.TinyMPCError, match="per-instance-family"):
        hs.set_precision(2)
    hs.close()
    # ... and on a shape without the stream form's ic kernels they are refused, the solver stays as it was
    rng = np.random.default_rng(8)
    A3 = np.repeat((np.eye(3) + np.diag([0.1, 0.1], 1))[:, :, None], B, axis=2) * (1.0 + 0.02 * rng.uniform(-1, 1, (3, 3, B)))
    B3 = np.repeat(np.array([[0.005], [0.05], [0.1]])[:, :, None], B, axis=2)
    f3 = tuple(np.asfortranarray(m) for m in (A3, B3, np.repeat(np.eye(3)[:, :, None], B, axis=2), np.ones((1, 1, B)))) + (np.ones(B),)
    h3 = t.BatchSolver.from_families(*f3, 8)
    name31 = h3.kernel_name
    with pytest.raises(t.TinyMPCError, match="per-instance cones need the stream kernel's ic form"):
        h3.set_instance_cones(None, None, None, [0], [3], np.full((1, B), 0.5))
    assert h3.cone_mode() == 0 and h3.kernel_name == name31
    h3.close()
    # the process-global entry: mixed widths are refused; re-batching drops the coefficients
    prob = case["prob"]
    s = t.TinyMPCSolver()
    t.setup(s, prob.A, prob.B, prob.fdyn, prob.Q, prob.R, prob.rho, 6, 3, prob.N, batch=B)
    try:
        with pytest.raises(t.TinyMPCError, match="mixed widths"):
            t.set_cone_constraints(s, LAYOUT[0], LAYOUT[1], cu, LAYOUT[2], LAYOUT[3], [0.5])
        assert t.cone_mode() == 0
        t.set_cone_constraints(s, LAYOUT[0], LAYOUT[1], cu, LAYOUT[2], LAYOUT[3], cx)
        assert t.cone_mode() == 1 and t.kernel_name() == "stream4<6,3;ic>"
        t.set_batch_size(s, B + 2)
        assert t.cone_mode() == 0 and not t.kernel_name().endswith(";ic>"), t.kernel_name()
    finally:
        t.cleanup()


def test_set_gpus_drops_the_coefficients(hip_lib, monkeypatch):
    """re-batching through set_gpus: the fresh shards get the master's family state WITHOUT its per-instance coefficients — no
    cones at all, not shared cones with a stale mu — and solve like the shards of a solver that never had cones; per-instance
    coefficients given to the sharded global solver reach the shards, equal the single handle, and do not survive the next
    re-batch either"""
    monkeypatch.setenv("TINYMPC_HIP_SHARD_DEVICES", "0,0")
    case = _cone_case()
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    cu, cx = _mu()

    def setup():
        s = t.TinyMPCSolver()
        t.setup(s, prob.A, prob.B, prob.fdyn, prob.Q, prob.R, prob.rho, 6, 3, prob.N, batch=B, max_iter=kw["max_iter"],
                abs_pri_tol=kw["abs_pri_tol"], abs_dua_tol=kw["abs_dua_tol"], check_termination=kw["check_termination"])
        t.set_bound_constraints(s, prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        return s

    def run(s):
        t.set_x0(s, x0)
        status = t.solve(s)
        return dict(sol=t.get_solution(s), st=t.get_status(s), status=status)
    bs = _solver(dict(case, ext=lambda o: o.set_fdyn(prob.fdyn)))
    bs.set_instance_cones(LAYOUT[0], LAYOUT[1], cu, LAYOUT[2], LAYOUT[3], cx)
    bs.set_x0(x0)
    bs.solve()
    single = _results(bs, workspace=False)
    bs.close()
    try:
        s = setup()
        t.set_gpus(s, 2)
        plain = run(s)                                     # two shards, never any cone
        plain_name = t.kernel_name()
        t.cleanup()
        s = setup()
        t.set_cone_constraints(s, *ROCKET_CONES)           # (a shared set first: its mu must not come back either)
        t.set_cone_constraints(s, LAYOUT[0], LAYOUT[1], cu, LAYOUT[2], LAYOUT[3], cx)
        assert t.cone_mode() == 1
        with_cones = run(s)
        assert not np.array_equal(with_cones["sol"]["controls"], plain["sol"]["controls"])
        t.set_gpus(s, 2)
        assert t.cone_mode() == 0
        dropped = run(s)
        assert t.cone_mode() == 0 and t.kernel_name() == plain_name, t.kernel_name()
        _identical(plain, dropped, "set_gpus on a solver with per-instance cones against shards that never had cones")
        # per-instance coefficients on the sharded global solver: scattered to the shards, the single handle's results
        t.set_cone_constraints(s, LAYOUT[0], LAYOUT[1], cu, LAYOUT[2], LAYOUT[3], cx)
        assert t.cone_mode() == 1 and t.kernel_name() == "stream4<6,3;ic>"
        t.reset_workspace(s)                               # (the shards keep the workspace of the solve above)
        _identical(single, run(s), "the sharded global solver against one handle")
        t.set_batch_size(s, B)                             # the master replays no cones
        assert t.cone_mode() == 0
        _identical(plain, run(s), "re-batched sharded solver against shards that never had cones")
    finally:
        t.cleanup()


def test_no_ic_loop_kernel(hip_lib, monkeypatch):
    """under both stream switches the loop is still the chain: there is no `ic` loop kernel to pick"""
    monkeypatch.setenv("TINYMPC_HIP_STREAM_MPC", "1")
    monkeypatch.setenv("TINYMPC_HIP_STREAM_LOOP", "1")
    case = _cone_case()
    case["kw"] = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=10, check_termination=1)
    bs = _ic_solver(case, *_mu())
    bs.set_warm_start(True)
    bs.set_x0(case["x0"])
    bs.mpc_rollout(3)
    from tests.test_stream_loop_gpu import _launches
    assert bs.last_launch_name == "stream4<6,3;ic>" and _launches(bs) == 3      # (one launch a step: the chain)
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. closed loop: both chains
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["stream_mpc", "own_plant"])
def test_closed_loop_chains(hip_lib, monkeypatch, chain):
    from tests.test_plant_loop_gpu import _rule_row
    if chain == "stream_mpc":
        monkeypatch.setenv("TINYMPC_HIP_STREAM_MPC", "1")
    else:
        monkeypatch.delenv("TINYMPC_HIP_STREAM_MPC", raising=False)
    steps = 5
    case = _cone_case()
    prob, x0 = case["prob"], case["x0"]
    case["kw"] = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=15, check_termination=1)
    cu, cx = _mu()
    rng = np.random.default_rng(12)
    Ap = prob.A * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, prob.A.shape)) if chain == "own_plant" else prob.A
    Bp = prob.B * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, prob.B.shape)) if chain == "own_plant" else prob.B
    f = np.asarray(prob.fdyn, dtype=np.float64).ravel()

    def solver():
        bs = _ic_solver(case, cu, cx)
        bs.set_warm_start(True)
        if chain == "own_plant":
            bs.set_plant(Ap, Bp, f)
        return bs
    bs = solver()
    bs.set_x0(x0)
    log = bs.mpc_rollout(steps)
    assert bs.kernel_name == "stream4<6,3;ic>" and bs.last_launch_name == "stream4<6,3;ic>"
    bs.close()
    # the same loop stepped from the host on an identical solver, bit for bit
    hs = _ic_solver(case, cu, cx)
    hs.set_warm_start(True)
    x = np.array(x0, dtype=np.float64)
    for k in range(steps):
        hs.set_x0(_f32(x))
        hs.solve()
        u0, st = hs.get_solution()["controls"][:, 0, :], hs.get_status()
        x = np.array([[_rule_row(Ap, Bp, f, x[:, b], u0[:, b], r) for b in range(B)] for r in range(prob.nx)])
        assert np.array_equal(log["u"][:, k, :], u0), f"{chain}: step {k}, u log"
        assert np.array_equal(log["x"][:, k, :], _f32(x)), f"{chain}: step {k}, x log"
        assert np.array_equal(log["iter"][k], st["iter"]) and np.array_equal(log["solved"][k], st["solved"]), f"{chain}: step {k}"
    assert hs.last_launch_name == "stream4<6,3;ic>"
    hs.close()
    assert len(np.unique(log["u"][:, 0, :], axis=1).T) > B / 2          # (the instances are not copies of each other)
    # 3 + 2 steps are 5 steps
    two = solver()
    two.set_x0(x0)
    la, lb = two.mpc_rollout(3), two.mpc_rollout(2)
    two.close()
    for key in ("x", "u"):
        assert np.array_equal(np.concatenate([la[key], lb[key]], axis=1), log[key]), f"{chain}: 3 + 2 steps, {key}"
    if chain == "own_plant":       # without a plant of its own and without the switch there is no loop
        plain = _ic_solver(case, cu, cx)
        plain.set_warm_start(True)
        plain.set_x0(x0)
        with pytest.raises(t.TinyMPCError, match="per-instance cones have no closed loop"):
            plain.mpc_rollout(2)
        plain.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. sharded     9. process-global entry
# ---------------------------------------------------------------------------------------------------------------------------
def test_sharded_equals_single_handle(hip_lib):
    Bn = 37
    case = _cone_case(batch=Bn)
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    xr, ur = t.problems.rocket_refs(prob.N)
    cu, cx = _mu(Bn)
    bs = _ic_solver(case, cu, cx)
    bs.set_x0(x0)
    bs.solve()
    one = _results(bs)
    bs.close()
    sh = t.ShardedBatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=Bn, n_gpus=2, devices=[0, 0])
    assert sh.fold_backend == "host"
    sh.update_settings(**kw)
    sh.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    f = np.ascontiguousarray(np.asarray(prob.fdyn, dtype=np.float64).reshape(-1))
    for i in range(sh.n_shards):       # (the sharded handle has no entry for the affine term: every shard's own)
        assert sh.lib.tinympc_set_fdyn(sh.shard(i)[3], f.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    sh.set_x_ref(xr)
    sh.set_u_ref(ur)
    sh.set_instance_cones(LAYOUT[0], LAYOUT[1], cu, LAYOUT[2], LAYOUT[3], cx)
    assert sh.kernel_names() == ["stream4<6,3;ic>"] * 2
    sh.set_x0(x0)
    status = sh.solve()
    two = dict(sol=sh.get_solution(), st=sh.get_status(), status=status, ws=sh.get_workspace())
    sh.close()
    _identical(one, two, "two shards against one handle")
    assert len(np.unique(one["st"]["iter"])) > 2


def test_global_entry_takes_two_dimensional_coefficients(hip_lib):
    case = _cone_case()
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    xr, ur = t.problems.rocket_refs(prob.N)
    cu, cx = _mu()
    bs = _ic_solver(case, cu, cx)
    bs.set_x0(x0)
    bs.solve()
    want = _results(bs, workspace=False)
    bs.close()
    s = t.TinyMPCSolver()
    try:
        t.setup(s, prob.A, prob.B, prob.fdyn, prob.Q, prob.R, prob.rho, 6, 3, prob.N, batch=B, max_iter=kw["max_iter"],
                abs_pri_tol=kw["abs_pri_tol"], abs_dua_tol=kw["abs_dua_tol"], check_termination=kw["check_termination"])
        t.set_bound_constraints(s, prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        t.set_x_ref(s, xr)
        t.set_u_ref(s, ur)
        t.set_cone_constraints(s, LAYOUT[0], LAYOUT[1], cu, LAYOUT[2], LAYOUT[3], cx)
        assert t.kernel_name() == "stream4<6,3;ic>"
        t.set_x0(s, x0)
        status = t.solve(s)
        got = dict(sol=t.get_solution(s), st=t.get_status(s), status=status)
        assert t.kernel_name() == "stream4<6,3;ic>"
    finally:
        t.cleanup()
    _identical(want, got, "global entry against BatchSolver.set_instance_cones")
