"""Box bounds PER INSTANCE (tinympc_set_instance_bounds): the `ib` form of the stream kernel on the three benchmark shapes, of
the generic kernel elsewhere, through tinympc.py.

Batch 70: four lanes per instance make that two stream workgroups, the second ragged with 6 live instances.  The horizons
have no built-in on-chip entry (cartpole N = 17, quadrotor N = 7, rocket N = 12: the shapes of tests/test_stream_loop_gpu.py),
so the shared-bounds arm of a comparison runs on the stream kernel too.

 1 equal bounds, equal bits   per-instance bounds that replicate a shared set reproduce the shared-bounds stream kernel bit for
                              bit, both layouts (constant over the horizon, per knot), one-shot and kept-workspace solves
 2 oracle, every instance     one CpuSolver per instance with that instance's bounds (tests/util.parity_every_instance): input
                              limits drawn in [0.2, 1] x the example's, a finite state bound on one row for every other
                              instance, the per-knot layout tightening over the horizon by an instance-dependent slope
 3 compaction                 the bound arrays are indexed by the instance, not by the launch's dense slot
 4 generic fallback           a shape outside the stream grid, precision 1, precision 2
 5 routing and refusals       6 settings toggle       7 closed loop (chain)       8 sharded       9 process-global entry

The inputs of 2 and 3 are checked on the ORACLE's results alone, so that the tests cannot pass vacuously: at least half the
instances have a control knot at their own limit (within 1e-6) and at least half differ by more than 1e-3 (nrel) from the
oracle's solution under the batch's widest limits.  Every limit is an fp32 value, so the oracle (fp64) and the device arrays
(fp32) hold the same numbers.  The closed loop (7) takes its switch as tests/test_stream_loop_gpu.py does: the environment
is read when a solver is created, so a solver created under monkeypatch sees it — no child process is needed.
Every test fails without the feature (BatchSolver.set_instance_bounds does not exist there)."""
import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.util import FP32_TOL, load_golden, nrel_batch, parity_every_instance, precision1_limit

pytestmark = pytest.mark.gpu

B = 70
TIGHT = 1e-6        # tests/test_precision2_gpu.py: generic<f64> against the oracle fed the same fp32 inputs
BIG = 1e17
ROCKET_CONES = ([0], [3], [0.25], [0], [3], [0.5])
TOL_KW = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, check_termination=1)


def _f32(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float32).astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------------------
# cases: the family, the x0 batch, the row that gets a state bound, extensions; bounds: per-instance limits of a case
# ---------------------------------------------------------------------------------------------------------------------------
def _case(name, batch=B):
    if name == "cartpole":
        return dict(prob=t.problems.cartpole(17, u_bound=0.5), x0=_f32(2.0 * t.problems.cartpole_x0(batch, seed=7)), row=1,
                    kw=dict(TOL_KW, max_iter=40), name="stream4<4,1>")
    if name == "quadrotor":
        return dict(prob=t.problems.quadrotor(7), x0=_f32(t.problems.quadrotor_x0(batch, seed=5)), row=8,
                    kw=dict(TOL_KW, max_iter=25), name="stream4<12,4>")
    if name == "rocket":
        return dict(prob=t.problems.rocket(12), x0=_f32(t.problems.rocket_x0(batch, seed=5)), row=5, kw=dict(TOL_KW, max_iter=40),
                    name="stream4<6,3>")
    if name == "rocket_cones":
        prob = t.problems.rocket(12)
        xr, ur = t.problems.rocket_refs(12)

        def ext(o):
            o.set_fdyn(prob.fdyn)
            o.set_cone_constraints(*ROCKET_CONES)
            o.set_x_ref(xr)
            o.set_u_ref(ur)
        return dict(prob=prob, x0=_f32(t.problems.rocket_x0(batch, seed=6)), row=5, kw=dict(TOL_KW, max_iter=40), ext=ext,
                    name="stream4<6,3>")
    if name == "cartpole_rows":
        g = load_golden("X3_cartpole_linear_rows")
        lin = (np.array(g["lin"]["Ax"]), np.array(g["lin"]["bx"]), np.array(g["lin"]["Au"]), np.array(g["lin"]["bu"]))
        return dict(prob=t.problems.cartpole(17, u_bound=0.5), x0=_f32(2.0 * t.problems.cartpole_x0(batch, seed=9)), row=1,
                    kw=dict(TOL_KW, max_iter=40), ext=lambda o: o.set_linear_constraints(*lin), name="stream4<4,1>")
    if name == "cartpole_families":
        base = t.problems.cartpole(17, u_bound=0.5)
        rng = np.random.default_rng(3)
        A = np.repeat(base.A[:, :, None], batch, axis=2) * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, (4, 4, batch)))
        Bm = np.repeat(base.B[:, :, None], batch, axis=2) * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, (4, 1, batch)))
        Q = np.repeat(base.Q[:, :, None], batch, axis=2)
        R = np.repeat(base.R[:, :, None], batch, axis=2)
        fam = tuple(np.asfortranarray(m) for m in (A, Bm, Q, R)) + (np.full(batch, base.rho),)
        return dict(prob=base, x0=_f32(2.0 * t.problems.cartpole_x0(batch, seed=11)), row=1, kw=dict(TOL_KW, max_iter=40), fam=fam,
                    name="stream4<4,1>")
    if name == "odd52":      # a shape outside the stream kernel's ib grid: (5, 2), N = 6
        rng = np.random.default_rng(52)
        nx, nu, N = 5, 2, 6
        A = np.eye(nx) + 0.1 * rng.standard_normal((nx, nx))
        Bm = 0.3 * rng.standard_normal((nx, nu))
        prob = t.problems.Problem("odd52", A, Bm, np.diag(rng.uniform(1.0, 5.0, nx)), np.diag(rng.uniform(0.5, 2.0, nu)), 1.0, N)
        prob.x_min, prob.x_max = np.full((nx, N), -BIG), np.full((nx, N), BIG)
        prob.u_min, prob.u_max = np.full((nu, N - 1), -0.6), np.full((nu, N - 1), 0.6)
        return dict(prob=prob, x0=_f32(rng.uniform(-1.0, 1.0, (nx, batch))), row=2, kw=dict(TOL_KW, max_iter=40), name="generic")
    raise KeyError(name)


def _bounds(case, per_knot, seed=1):
    """(x_min, x_max, u_min, u_max) per instance, fp32 values.  Constant layout: (nx, B) / (nu, B); per knot: (nx, N, B) /
    (nu, N-1, B), the constant set tightened over the horizon by a slope drawn per instance (up to 30 % at the last knot)."""
    prob, x0 = case["prob"], case["x0"]
    nx, nu, N, Bn = prob.nx, prob.nu, prob.N, x0.shape[1]
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.2, 1.0, Bn)
    u_min, u_max = prob.u_min[:, :1] * s[None, :], prob.u_max[:, :1] * s[None, :]
    x_min, x_max = np.full((nx, Bn), -BIG), np.full((nx, Bn), BIG)
    r = case["row"]
    lim = 1.05 * np.abs(x0[r]) + 0.02 * np.abs(x0[r]).max()        # just outside the instance's own x0: met at knot 0, active later
    x_min[r, ::2], x_max[r, ::2] = -lim[::2], lim[::2]               # every other instance; none for the rest
    if not per_knot:
        return tuple(_f32(a) for a in (x_min, x_max, u_min, u_max))
    slope = rng.uniform(0.0, 0.3, Bn)
    fx = 1.0 - slope[None, None, :] * (np.arange(N) / (N - 1))[None, :, None]
    fu = fx[:, :N - 1, :]
    finite = lambda a, f: np.where(np.abs(a[:, None, :]) >= BIG, a[:, None, :], a[:, None, :] * f)
    return tuple(_f32(a) for a in (finite(x_min, fx), finite(x_max, fx), finite(u_min, fu), finite(u_max, fu)))


def _knots(a, knots):
    """an instance-bounds array as (rows, knots, B)"""
    return a if a.ndim == 3 else np.repeat(a[:, None, :], knots, axis=1)


def _model(case, b):
    if "fam" in case:
        A, Bm, Q, R, rho = case["fam"]
        return A[:, :, b], Bm[:, :, b], Q[:, :, b], R[:, :, b], float(rho[b])
    p = case["prob"]
    return p.A, p.B, p.Q, p.R, p.rho


def _make_oracle(oracle, case, bounds, kw=None):
    """make_oracle(b) of parity_every_instance: a cold orc64 solver with instance b's own bounds"""
    N = case["prob"].N
    xlo, xhi, ulo, uhi = _knots(bounds[0], N), _knots(bounds[1], N), _knots(bounds[2], N - 1), _knots(bounds[3], N - 1)

    def make(b):
        o = oracle.CpuSolver("orc64", *_model(case, b), N)
        o.update_settings(**(kw or case["kw"]))
        o.set_bound_constraints(xlo[:, :, b], xhi[:, :, b], ulo[:, :, b], uhi[:, :, b])
        if "ext" in case:
            case["ext"](o)
        return o
    return make


def _oracle_solves(make, x0s, forced_first=None):
    """every instance on its own persistent oracle through the solves x0s[0], x0s[1], ...; the result of the last one.
    forced_first: (iter, solved) of the first solve, imposed on it (the GPU's decisions), the later solves free."""
    Bn = x0s[0].shape[1]
    out = None
    for b in range(Bn):
        o = make(b)
        for j, x0 in enumerate(x0s):
            o.set_forced_exit(0)
            if j == 0 and forced_first is not None and len(x0s) > 1:
                o.set_forced_exit(int(forced_first[0][b]) if forced_first[1][b] else -1)
            o.set_x0(x0[:, b])
            o.solve()
        r = o.get_solution()
        if out is None:
            out = dict(x=np.zeros(r["x"].shape + (Bn,)), u=np.zeros(r["u"].shape + (Bn,)), iter=np.zeros(Bn, dtype=int),
                       solved=np.zeros(Bn, dtype=int), res=np.zeros((Bn, 4)))
        out["x"][:, :, b], out["u"][:, :, b] = r["x"], r["u"]
        out["iter"][b], out["solved"][b], out["res"][b] = r["iter"], r["solved"], r["res"]
        o.close()
    return out


def _inputs_bite(oracle, case, bounds, ref, tag):
    """the condition on the inputs, on the oracle's results alone"""
    N, Bn = case["prob"].N, case["x0"].shape[1]
    ulo, uhi = _knots(bounds[2], N - 1), _knots(bounds[3], N - 1)
    at_limit = ((np.abs(ref["u"] - ulo) <= 1e-6) | (np.abs(ref["u"] - uhi) <= 1e-6)).any(axis=(0, 1))
    assert at_limit.sum() >= Bn / 2, f"{tag}: only {int(at_limit.sum())} of {Bn} instances reach their own input limit"
    xlo, xhi = _knots(bounds[0], N), _knots(bounds[1], N)
    widest = (np.repeat(xlo.min(axis=2, keepdims=True), Bn, axis=2), np.repeat(xhi.max(axis=2, keepdims=True), Bn, axis=2),
              np.repeat(ulo.min(axis=2, keepdims=True), Bn, axis=2), np.repeat(uhi.max(axis=2, keepdims=True), Bn, axis=2))
    wide = _oracle_solves(_make_oracle(oracle, case, widest), [case["x0"]])
    differs = np.maximum(nrel_batch(ref["x"], wide["x"]), nrel_batch(ref["u"], wide["u"])) > 1e-3
    assert differs.sum() >= Bn / 2, f"{tag}: only {int(differs.sum())} of {Bn} instances differ from the widest-limit solution"


def _solver(case, precision=0, batch=None):
    prob = case["prob"]
    if "fam" in case:
        bs = t.BatchSolver.from_families(*case["fam"], prob.N)
    else:
        bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=batch or case["x0"].shape[1])
    bs.update_settings(**case["kw"])
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if "ext" in case:
        case["ext"](bs)
    if precision:
        bs.set_precision(precision)
        if precision == 1:
            bs.set_strict_precision(True)
    return bs


def _results(bs, workspace=True):
    out = dict(sol=bs.get_solution(), st=bs.get_status(), status=bs.solve_status())
    if workspace:
        out["ws"] = bs.get_workspace()
    return out


def _identical(a, c, tag):
    assert a["status"] == c["status"], tag
    for key in ("states", "controls"):
        assert np.array_equal(a["sol"][key], c["sol"][key]), f"{tag}: {key}"
    for key in ("iter", "solved", "residuals"):
        assert np.array_equal(a["st"][key], c["st"][key]), f"{tag}: {key}"
    if "ws" in a and "ws" in c:
        for key in ("d", "y", "g", "v", "z"):
            assert np.array_equal(a["ws"][key], c["ws"][key]), f"{tag}: workspace {key}"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. equal bounds, equal bits
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [True, False], ids=["30_iterations", "tolerance"])
@pytest.mark.parametrize("name", ["cartpole", "quadrotor", "rocket"])
def test_equal_bounds_equal_bits(hip_lib, name, fixed):
    case = _case(name)
    prob, x0 = case["prob"], case["x0"]
    nx, nu, N = prob.nx, prob.nu, prob.N
    kw = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=30, check_termination=1) if fixed else dict(TOL_KW, max_iter=30)
    r = case["row"]
    xb = _f32(0.9 * np.abs(x0[r]).max())        # a finite state bound that is active for part of the batch
    x_min, x_max = prob.x_min.copy(), prob.x_max.copy()
    x_min[r, :], x_max[r, :] = -xb, xb
    shared = tuple(_f32(a) for a in (x_min, x_max, prob.u_min, prob.u_max))
    x0b = _f32(0.9 * x0)
    runs = {}
    for arm in ("shared", "constant", "per_knot"):
        bs = _solver(case)
        bs.update_settings(**kw)
        if arm == "shared":
            bs.set_bound_constraints(*shared)
        elif arm == "constant":
            bs.set_instance_bounds(*[np.repeat(a[:, :1], B, axis=1) for a in shared])
        else:
            bs.set_instance_bounds(*[np.repeat(a[:, :, None], B, axis=2) for a in shared])
        assert bs.bounds_mode() == ("shared", "constant", "per_knot").index(arm)
        want = case["name"] if arm == "shared" else case["name"][:-1] + ";ib>"
        out = []
        bs.set_warm_start(False)                 # one-shot
        bs.set_x0(x0)
        bs.solve()
        assert bs.kernel_name == want and bs.last_launch_name == want, (bs.kernel_name, bs.last_launch_name)
        out.append(_results(bs, workspace=False))
        bs.set_warm_start(True)                  # two consecutive kept-workspace solves
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
    if not fixed and name == "cartpole":
        assert len(np.unique(runs["shared"][1]["st"]["iter"])) > 2, "the tolerance decides nothing in this batch"
    for arm in ("constant", "per_knot"):
        for j, what in enumerate(("one-shot", "kept workspace, first", "kept workspace, second")):
            _identical(runs["shared"][j], runs[arm][j], f"{name}, {arm}, {what}")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. oracle, every instance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_knot", [False, True], ids=["constant", "per_knot"])
@pytest.mark.parametrize("name", ["cartpole", "quadrotor", "rocket", "rocket_cones", "cartpole_rows", "cartpole_families"])
def test_oracle_every_instance(hip_lib, oracle_built, name, per_knot):
    case = _case(name)
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    bounds = _bounds(case, per_knot)
    make = _make_oracle(oracle_built, case, bounds)
    ref = _oracle_solves(make, [x0])
    tag = f"{name}, {'per knot' if per_knot else 'constant'}"
    _inputs_bite(oracle_built, case, bounds, ref, tag)
    rho = float(np.max(case["fam"][4])) if "fam" in case else prob.rho
    want = case["name"][:-1] + ";ib>"
    bs = _solver(case)
    bs.set_instance_bounds(*bounds)
    assert bs.bounds_mode() == (2 if per_knot else 1) and bs.kernel_name == want
    bs.set_x0(x0)
    # cold start
    bs.set_warm_start(False)
    bs.solve()
    assert bs.last_launch_name == want
    same = parity_every_instance(bs.get_solution(), bs.get_status(), ref, make, x0, kw, rho, tag=tag + ", cold")
    print(f"{tag}: cold, {same:.2f} of the iteration counts are the oracle's; iterations {ref['iter'].min()}..{ref['iter'].max()}")
    # the second solve of a warm pair from a shifted x0; the first solve's exits are the GPU's own on both sides
    x1 = _f32(0.9 * x0)
    bs.set_warm_start(True)
    bs.reset()
    bs.solve()
    st0 = bs.get_status()
    parity_every_instance(bs.get_solution(), st0, ref, make, x0, kw, rho, tag=tag + ", warm pair, first")
    bs.set_x0(x1)
    bs.solve()
    assert bs.last_launch_name == want
    first = (st0["iter"], st0["solved"])
    ref1 = _oracle_solves(make, [x0, x1], forced_first=first)

    def make_warm(b):
        o = make(b)
        o.set_forced_exit(int(first[0][b]) if first[1][b] else -1)
        o.set_x0(x0[:, b])
        o.solve()
        o.set_forced_exit(0)
        return o
    parity_every_instance(bs.get_solution(), bs.get_status(), ref1, make_warm, x1, kw, rho, tag=tag + ", warm pair, second")
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. compaction: instance index against dense slot
# ---------------------------------------------------------------------------------------------------------------------------
def test_compaction_indexes_bounds_by_instance(hip_lib, oracle_built):
    Bn = 200
    case = _case("cartpole", batch=Bn)
    spread = np.linspace(0.05, 3.0, Bn)[np.random.default_rng(4).permutation(Bn)]       # iteration counts range widely
    case["x0"] = x0 = _f32(t.problems.cartpole_x0(Bn, seed=7) * spread[None, :])
    case["kw"] = kw = dict(TOL_KW, max_iter=60)
    bounds = _bounds(case, per_knot=True)
    make = _make_oracle(oracle_built, case, bounds)
    ref = _oracle_solves(make, [x0])
    _inputs_bite(oracle_built, case, bounds, ref, "compaction")
    assert ref["iter"].max() >= 4 * max(1, ref["iter"].min()) and 0 < ref["solved"].sum()
    runs = []
    for chunk in (0, 4):
        bs = _solver(case)
        bs.set_instance_bounds(*bounds)
        bs.set_compaction(chunk)
        bs.set_x0(x0)
        bs.solve()
        assert bs.last_launch_name == "stream4<4,1;ib>"
        runs.append(_results(bs))
        bs.close()
    _identical(runs[0], runs[1], "single launch against chunks of 4 iterations")
    parity_every_instance(runs[1]["sol"], runs[1]["st"], ref, make, x0, kw, case["prob"].rho, tag="compaction")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. generic fallback
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["odd_shape", "precision1", "precision2"])
def test_generic_fallback(hip_lib, oracle_built, which):
    case = _case("odd52" if which == "odd_shape" else "cartpole")
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    precision = dict(odd_shape=0, precision1=1, precision2=2)[which]
    bounds = _bounds(case, per_knot=True)
    make = _make_oracle(oracle_built, case, bounds)
    ref = _oracle_solves(make, [x0])
    want = "generic<f64;ib>" if precision == 2 else "generic<ib>"
    bs = _solver(case, precision=precision)
    bs.set_instance_bounds(*bounds)
    assert bs.kernel_name == want and bs.bounds_mode() == 2
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
    elif precision == 1:
        # the bar of an all-fp32 kernel, from the reference model alone: orc32 against orc64 on these very problems
        r32 = dict(x=np.zeros_like(ref["x"]), u=np.zeros_like(ref["u"]), iter=np.zeros(B, dtype=int), solved=np.zeros(B, dtype=int))
        N = prob.N
        b4 = [_knots(a, N if i < 2 else N - 1) for i, a in enumerate(bounds)]
        for b in range(B):
            o = oracle_built.CpuSolver("orc32", prob.A, prob.B, prob.Q, prob.R, prob.rho, N)
            o.update_settings(**kw)
            o.set_bound_constraints(*[a[:, :, b] for a in b4])
            o.set_x0(x0[:, b])
            o.solve()
            r = o.get_solution()
            r32["x"][:, :, b], r32["u"][:, :, b], r32["iter"][b], r32["solved"][b] = r["x"], r["u"], r["iter"], r["solved"]
            o.close()
        limit, e32, share = precision1_limit(r32, ref)
        print(f"precision 1: limit {limit:.3e} (orc32 against orc64 {e32:.3e}, {share:.2f} of the instances agree on the exit)")
        parity_every_instance(sol, st, ref, make, x0, kw, prob.rho, tol=limit, tag="precision 1")
    else:
        parity_every_instance(sol, st, ref, make, x0, kw, prob.rho, tag="(5, 2)")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. routing and refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_routing_round_trip_and_refusals(hip_lib, monkeypatch):
    monkeypatch.delenv("TINYMPC_HIP_STREAM_MPC", raising=False)
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), _f32(t.problems.cartpole_x0(B, seed=3))
    case = dict(prob=prob, x0=x0, row=1, kw=dict(TOL_KW, max_iter=40))
    shared = (prob.x_min, prob.x_max, prob.u_min, prob.u_max)

    def run(bs):
        bs.set_x0(x0)
        bs.solve()
        return _results(bs)
    stay = _solver(case)
    home = stay.kernel_name
    assert home.startswith(("quad<4,1,20", "lean<4,1,20")), home
    r_stay = run(stay)
    home_launch = stay.last_launch_name
    stay.close()
    bs = _solver(case)
    assert bs.kernel_name == home and bs.bounds_mode() == 0
    bs.set_instance_bounds(*_bounds(case, per_knot=False))
    assert bs.kernel_name == "stream4<4,1;ib>" and bs.bounds_mode() == 1
    run(bs)
    assert bs.last_launch_name == "stream4<4,1;ib>"
    bs.set_instance_bounds(*_bounds(case, per_knot=True))
    assert bs.kernel_name == "stream4<4,1;ib>" and bs.bounds_mode() == 2
    # refused beside per-instance bounds, each with a message: adaptive rho, the closed loop without its switch
    with pytest.raises(t.TinyMPCError, match="per-instance bounds"):
        bs.set_adaptive_rho(True)
    with pytest.raises(t.TinyMPCError, match="per-instance bounds"):
        bs.mpc_rollout(2)
    with pytest.raises(t.TinyMPCError):          # a layout that is neither
        bs.set_instance_bounds(np.zeros((4, B)), np.zeros((4, B)), np.zeros((1, 16, B)), np.zeros((1, 16, B)))
    bs.set_bound_constraints(*shared)
    assert bs.kernel_name == home and bs.bounds_mode() == 0
    bs.reset()
    r_back = run(bs)
    assert bs.last_launch_name == home_launch
    _identical(r_stay, r_back, "after the round trip")
    bs.close()
    # ... and in the other order: per-instance bounds on a solver that already adapts rho
    ad = _solver(case)
    ad.set_adaptive_rho(True)
    with pytest.raises(t.TinyMPCError, match="adaptive rho"):
        ad.set_instance_bounds(*_bounds(case, per_knot=False))
    assert ad.bounds_mode() == 0
    ad.close()
    # mixed column counts on the process-global entry
    s = t.TinyMPCSolver()
    t.setup(s, prob.A, prob.B, np.zeros(4), prob.Q, prob.R, prob.rho, 4, 1, 20, batch=B)
    try:
        b3 = _bounds(case, per_knot=True)
        with pytest.raises(t.TinyMPCError, match="mixed widths"):
            t.set_bound_constraints(s, b3[0], b3[1], prob.u_min, prob.u_max)
    finally:
        t.cleanup()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. settings toggle
# ---------------------------------------------------------------------------------------------------------------------------
def test_settings_toggle(hip_lib):
    case = _case("cartpole")
    kw, x0 = case["kw"], case["x0"]
    bounds = _bounds(case, per_knot=True)
    no_u = (bounds[0], bounds[1], np.full_like(bounds[2], -BIG), np.full_like(bounds[3], BIG))

    def run(bs):
        bs.set_warm_start(False)
        bs.set_x0(x0)
        bs.solve()
        assert bs.last_launch_name == "stream4<4,1;ib>"
        return _results(bs, workspace=False)
    free = _solver(case)
    free.set_instance_bounds(*no_u)
    r_free = run(free)
    free.close()
    bs = _solver(case)
    bs.set_instance_bounds(*bounds)
    r_on = run(bs)
    bs.update_settings(**kw, en_state_bound=1, en_input_bound=0)
    r_off = run(bs)
    bs.update_settings(**kw, en_state_bound=1, en_input_bound=1)
    r_again = run(bs)
    bs.close()
    _identical(r_free, r_off, "en_input_bound = 0 against the solve without input bounds")
    _identical(r_on, r_again, "en_input_bound back to 1")
    assert not np.array_equal(r_on["sol"]["controls"], r_off["sol"]["controls"])


# ---------------------------------------------------------------------------------------------------------------------------
# 7. closed loop: the chain of launches under TINYMPC_HIP_STREAM_MPC
# ---------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_chain(hip_lib, oracle_built, monkeypatch):
    monkeypatch.setenv("TINYMPC_HIP_STREAM_MPC", "1")
    monkeypatch.setenv("TINYMPC_HIP_STREAM_LOOP", "1")      # (no ib loop form: the chain takes it all the same)
    steps = 3
    case = _case("cartpole")
    prob, x0 = case["prob"], case["x0"]
    kw = case["kw"] = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=15, check_termination=1)
    bounds = _bounds(case, per_knot=False)
    bs = _solver(case)
    bs.set_instance_bounds(*bounds)
    bs.set_warm_start(True)
    bs.set_x0(x0)
    log = bs.mpc_rollout(steps)
    assert bs.kernel_name == "stream4<4,1;ib>" and bs.last_launch_name == "stream4<4,1;ib>"
    sol = bs.get_solution()
    bs.close()
    assert np.all(log["iter"] == kw["max_iter"]) and not log["solved"].any()
    make = _make_oracle(oracle_built, case, bounds)
    xs, us = np.zeros((prob.nx, steps, B)), np.zeros((prob.nu, steps, B))
    last_x, last_u = np.zeros_like(sol["states"]), np.zeros_like(sol["controls"])
    for b in range(B):       # orc64 stepped by the same rule: fp64 plant, fp32 applied control, each solve from the fp32 rounding
        o = make(b)
        x = np.array(x0[:, b])
        for k in range(steps):
            o.set_x0(_f32(x))
            o.solve()
            r = o.get_solution()
            u0 = _f32(r["u"][:, 0])
            x = prob.A @ x + prob.B @ u0
            xs[:, k, b], us[:, k, b] = x, u0
        last_x[:, :, b], last_u[:, :, b] = r["x"], r["u"]
        o.close()
    ulo, uhi = bounds[2], bounds[3]
    assert ((np.abs(us - ulo[:, None, :]) <= 1e-6) | (np.abs(us - uhi[:, None, :]) <= 1e-6)).any(axis=(0, 1)).sum() >= B / 2
    ex, eu = nrel_batch(log["x"], xs).max(), nrel_batch(log["u"], us).max()
    wx, wu = nrel_batch(sol["states"], last_x).max(), nrel_batch(sol["controls"], last_u).max()
    print(f"closed loop: plant states {ex:.3e}, applied controls {eu:.3e}, last solve {wx:.3e} / {wu:.3e}")
    assert max(ex, eu, wx, wu) <= FP32_TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 8. sharded     9. process-global entry
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_knot", [False, True], ids=["constant", "per_knot"])
def test_sharded_equals_single_handle(hip_lib, per_knot):
    Bn = 37
    case = _case("cartpole", batch=Bn)
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    bounds = _bounds(case, per_knot)
    bs = _solver(case)
    bs.set_instance_bounds(*bounds)
    bs.set_x0(x0)
    bs.solve()
    one = _results(bs)
    bs.close()
    sh = t.ShardedBatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=Bn, n_gpus=2, devices=[0, 0])
    assert sh.fold_backend == "host"
    sh.update_settings(**kw)
    sh.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    sh.set_instance_bounds(*bounds)
    assert sh.kernel_names() == ["stream4<4,1;ib>"] * 2
    sh.set_x0(x0)
    status = sh.solve()
    two = dict(sol=sh.get_solution(), st=sh.get_status(), status=status, ws=sh.get_workspace())
    sh.close()
    _identical(one, two, "two shards against one handle")
    assert len(np.unique(one["st"]["iter"])) > 2


def test_global_entry_takes_three_dimensional_bounds(hip_lib):
    case = _case("cartpole")
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    bounds = _bounds(case, per_knot=True)
    bs = _solver(case)
    bs.set_instance_bounds(*bounds)
    bs.set_x0(x0)
    bs.solve()
    want = _results(bs, workspace=False)
    bs.close()
    s = t.TinyMPCSolver()
    try:
        t.setup(s, prob.A, prob.B, np.zeros(4), prob.Q, prob.R, prob.rho, 4, 1, prob.N, batch=B, max_iter=kw["max_iter"],
                abs_pri_tol=kw["abs_pri_tol"], abs_dua_tol=kw["abs_dua_tol"], check_termination=kw["check_termination"])
        t.set_bound_constraints(s, *bounds)
        assert t.kernel_name() == "stream4<4,1;ib>"
        t.set_x0(s, x0)
        status = t.solve(s)
        got = dict(sol=t.get_solution(s), st=t.get_status(s), status=status)
        assert t.kernel_name() == "stream4<4,1;ib>"
    finally:
        t.cleanup()
    _identical(want, got, "global entry against BatchSolver.set_instance_bounds")
