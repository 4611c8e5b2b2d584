"""Linear rows PER INSTANCE (tinympc_set_instance_linear): the `il` form of the stream kernel on the three benchmark shapes, of the
generic kernel elsewhere, through tinympc.py.

Batch 70: four lanes per instance make that two stream workgroups, the second ragged with 6 live instances.  The horizons have
no built-in on-chip entry (cartpole N = 17, quadrotor N = 7, rocket N = 12), so the shared-rows arm of a comparison runs on the
stream kernel too.  The cases (family, x0 batch, settings, extensions) are tests/test_instance_bounds_gpu.py's.

 1 equal rows, equal bits     per-instance rows that replicate a shared set reproduce the plain stream kernel's EXT = 2 form bit
                              for bit, one-shot and over two kept-workspace solves, with and without replicated per-instance bounds
 2 oracle, every instance     one orc64 CpuSolver per instance with that instance's non-absent rows (tests/util.parity_every_instance)
 3 compaction                 the row arrays are indexed by the instance, not by the launch's dense slot
 4 generic fallback           a shape outside the stream grid, precision 1 and precision 2
 5 routing and refusals       6 closed loop (both chains)       7 sharded       8 process-global entry

The row recipe of 2 (every value an fp32 value, so the oracle and the device hold the same numbers): every instance is solved
without rows on the oracle; state row 0 is a unit direction (to the 2^-10 grid the coefficients lie on, so that |a|^2 is an fp32
value as well) at a per-instance angle in coordinates (0, 1); state row 1 is the
coordinate that moves most over the horizon, scaled by a factor in [0.5, 2]; both point where the free trajectory moves away from
x0, and b lies between a.x0 (plus a margin: x0 is feasible) and 0.7 of the way to the free maximum of a.x; two input rows are
single-coordinate rows scaled in [0.5, 2] with b at 0.8 of the free maximum; every third instance gets the same rows placed at 3.0,
where they never act.  That the inputs bite is asserted on the ORACLE's results alone, before the device is compared: at least half
the instances differ by more than 1e-3 (nrel) from their no-rows solution and from the solution under their neighbour's rows.
Every test fails without the feature (BatchSolver.set_instance_linear does not exist there)."""
import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.test_instance_bounds_gpu import B, TOL_KW, _case, _f32, _identical, _model, _oracle_solves, _results, _solver
from tests.util import FP32_TOL, load_golden, nrel_batch, parity_every_instance, precision1_limit

pytestmark = pytest.mark.gpu

TIGHT = 1e-6        # tests/test_precision2_gpu.py: generic<f64> against the oracle fed the same fp32 inputs
FAR = 3.0           # a right-hand side no trajectory of these cases reaches


# ---------------------------------------------------------------------------------------------------------------------------
# oracles and the row recipe
# ---------------------------------------------------------------------------------------------------------------------------
def _make_oracle(oracle, case, rows=None, kw=None, shift=0, kind="orc64"):
    """make_oracle(b) of parity_every_instance: a cold solver with the non-absent rows of instance (b + shift) % B (rows None: none)"""
    prob = case["prob"]

    def make(b):
        o = oracle.CpuSolver(kind, *_model(case, b), prob.N)
        o.update_settings(**(kw or case["kw"]))
        o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        if "ext" in case:
            case["ext"](o)
        if rows is not None:
            Ax, bx, Au, bu = rows
            j = (b + shift) % bx.shape[1]
            kx, ku = np.abs(Ax[:, :, j]).sum(axis=1) > 0, np.abs(Au[:, :, j]).sum(axis=1) > 0
            o.set_linear_constraints(Ax[kx, :, j].reshape(-1, prob.nx), bx[kx, j], Au[ku, :, j].reshape(-1, prob.nu), bu[ku, j])
        return o
    return make


def _grid(a):
    """coefficients on a grid of 2^-10: fp32 values whose squares, and the sum of two of them, are fp32 values too — the library
    keeps |a|^2 in fp32 (as the shared pack does), so the oracle's fp64 |a|^2 is then the same number"""
    return np.round(np.asarray(a) * 1024.0) / 1024.0


def _rows(case, free, seed=4, state_rows=2):
    """(Alin_x (mx, nx, B), blin_x (mx, B), Alin_u (2, nu, B), blin_u (2, B)) by the recipe of the module docstring, from the
    no-rows oracle solutions `free`.  state_rows = 3 adds the second most moving coordinate as a third row and keeps 1 + b % 3 of
    them for instance b (the others absent: zeros)."""
    prob, x0 = case["prob"], case["x0"]
    nx, nu, Bn = prob.nx, prob.nu, x0.shape[1]
    rng = np.random.default_rng(seed)
    X, U = free["x"], free["u"]
    moves = (X.max(axis=1) - X.min(axis=1)).mean(axis=1)
    order = np.argsort(-moves)
    Ax, bx = np.zeros((state_rows, nx, Bn)), np.zeros((state_rows, Bn))
    th = rng.uniform(0.0, 2.0 * np.pi, Bn)
    Ax[0, 0, :], Ax[0, 1, :] = _grid(np.cos(th)), _grid(np.sin(th))
    for k in range(1, state_rows):
        Ax[k, order[k - 1], :] = _grid(rng.uniform(0.5, 2.0, Bn))
    frac = rng.uniform(0.3, 0.7, (state_rows, Bn))
    for k in range(state_rows):
        for b in range(Bn):
            p = Ax[k, :, b] @ X[:, :, b]
            if p.max() - p[0] < p[0] - p.min():          # towards where the free trajectory moves away from x0
                Ax[k, :, b], p = -Ax[k, :, b], -p
            margin = 1e-3 * (1.0 + abs(p[0]))
            bx[k, b] = p[0] + max(margin, frac[k, b] * (p.max() - p[0]))
    Au, bu = np.zeros((2, nu, Bn)), np.zeros((2, Bn))
    s = _grid(rng.uniform(0.5, 2.0, (2, Bn)))
    for k in range(2):
        c = k if nu > 1 else 0
        sign = 1.0 if (k == 0 or nu > 1) else -1.0     # one input: the second row is the opposite side
        Au[k, c, :] = sign * s[k]
        bu[k, :] = 0.8 * (Au[k, c, :][None, :] * U[c]).max(axis=0)
    never = np.arange(Bn) % 3 == 2
    bx[:, never], bu[:, never] = FAR, FAR
    if state_rows == 3:
        for b in range(Bn):
            Ax[1 + b % 3:, :, b], bx[1 + b % 3:, b] = 0.0, 0.0
    return tuple(np.array(_f32(a)) for a in (Ax, bx, Au, bu))


def _inputs_bite(oracle, case, rows, ref, free, tag, kw=None):
    Bn = case["x0"].shape[1]
    differs = np.maximum(nrel_batch(ref["x"], free["x"]), nrel_batch(ref["u"], free["u"])) > 1e-3
    assert differs.sum() >= Bn / 2, f"{tag}: only {int(differs.sum())} of {Bn} instances differ from their no-rows solution"
    nb = _oracle_solves(_make_oracle(oracle, case, rows, kw=kw, shift=1), [case["x0"]])
    other = np.maximum(nrel_batch(ref["x"], nb["x"]), nrel_batch(ref["u"], nb["u"])) > 1e-3
    assert other.sum() >= Bn / 2, f"{tag}: only {int(other.sum())} of {Bn} instances differ from the solution under their neighbour's rows"
    print(f"{tag}: {int(differs.sum())} of {Bn} differ from no rows, {int(other.sum())} from the neighbour's rows; "
          f"{int(ref['solved'].sum())} converged, iterations {ref['iter'].min()}..{ref['iter'].max()}")


def _prepared(oracle, case, state_rows=2, kw=None, tag=""):
    free = _oracle_solves(_make_oracle(oracle, case, kw=kw), [case["x0"]])
    rows = _rows(case, free, state_rows=state_rows)
    make = _make_oracle(oracle, case, rows, kw=kw)
    ref = _oracle_solves(make, [case["x0"]])
    _inputs_bite(oracle, case, rows, ref, free, tag, kw=kw)
    return rows, make, ref


def _il_name(case):
    return case["name"][:-1] + ";il>" if case["name"].startswith("stream") else "generic<il>"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. equal rows, equal bits
# ---------------------------------------------------------------------------------------------------------------------------
def _shared_rows(name, case):
    if name == "cartpole":
        g = load_golden("X3_cartpole_linear_rows")["lin"]
        return np.array(g["Ax"]), np.array(g["bx"]), np.array(g["Au"]), np.array(g["bu"])
    prob, x0 = case["prob"], case["x0"]
    nx, nu = prob.nx, prob.nu
    Ax = np.zeros((2, nx))
    Ax[0, 0], Ax[0, 1] = 0.6, 0.8
    Ax[1, case["row"]] = 1.3
    bx = np.array([0.5 * np.abs(Ax[0] @ x0).max(), 0.5 * np.abs(Ax[1] @ x0).max()])      # met by part of the batch at knot 0
    Au = np.zeros((2, nu))
    Au[0, 0], Au[1, nu - 1] = 0.7, -1.1
    bu = 0.3 * np.array([0.7, 1.1]) * np.abs(prob.u_max).max()
    return Ax, bx, Au, bu


@pytest.mark.parametrize("fixed", [True, False], ids=["30_iterations", "tolerance"])
@pytest.mark.parametrize("name", ["cartpole", "quadrotor", "rocket"])
def test_equal_rows_equal_bits(hip_lib, name, fixed):
    case = _case(name)
    prob, x0 = case["prob"], case["x0"]
    kw = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=30, check_termination=1) if fixed else dict(TOL_KW, max_iter=30)
    lin = _shared_rows(name, case)
    rep = (np.repeat(lin[0][:, :, None], B, axis=2), np.repeat(lin[1][:, None], B, axis=1),
           np.repeat(lin[2][:, :, None], B, axis=2), np.repeat(lin[3][:, None], B, axis=1))
    x0b = _f32(0.9 * x0)
    runs = {}
    for arm in ("none", "shared", "il", "il_ib"):
        bs = _solver(case)
        bs.update_settings(**kw)
        bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)     # (update_settings switches both sides off)
        if arm == "shared":
            bs.set_linear_constraints(*lin)
        elif arm != "none":
            bs.set_instance_linear(*rep)
        if arm == "il_ib":
            bs.set_instance_bounds(*[np.repeat(a[:, :, None], B, axis=2) for a in (prob.x_min, prob.x_max, prob.u_min, prob.u_max)])
        assert bs.lin_mode() == (1 if arm.startswith("il") else 0) and bs.bounds_mode() == (2 if arm == "il_ib" else 0)
        want = case["name"] if not arm.startswith("il") else _il_name(case)
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
    assert not np.array_equal(runs["none"][0]["sol"]["controls"], runs["shared"][0]["sol"]["controls"]), "the shared rows decide nothing"
    for arm in ("il", "il_ib"):
        for j, what in enumerate(("one-shot", "kept workspace, first", "kept workspace, second")):
            _identical(runs["shared"][j], runs[arm][j], f"{name}, {arm}, {what}")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. oracle, every instance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole", "quadrotor", "rocket", "rocket_cones", "cartpole_families", "cartpole_123_rows"])
def test_oracle_every_instance(hip_lib, oracle_built, name):
    case = _case("cartpole" if name == "cartpole_123_rows" else name)
    if name == "quadrotor":
        case["kw"] = dict(TOL_KW, max_iter=60)
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    rows, make, ref = _prepared(oracle_built, case, state_rows=3 if name == "cartpole_123_rows" else 2, tag=name)
    if name == "quadrotor":     # both exits of the termination test are taken
        assert ref["solved"].sum() >= 10 and (ref["iter"] == kw["max_iter"]).sum() >= 10, (int(ref["solved"].sum()), ref["iter"])
    if name == "cartpole_123_rows":
        present = (np.abs(rows[0]).sum(axis=1) > 0).sum(axis=0)
        assert sorted(np.unique(present)) == [1, 2, 3]
    rho = float(np.max(case["fam"][4])) if "fam" in case else prob.rho
    want = _il_name(case)
    bs = _solver(case)
    bs.set_instance_linear(*rows)
    assert bs.lin_mode() == 1 and bs.kernel_name == want
    bs.set_warm_start(False)
    bs.set_x0(x0)
    bs.solve()
    assert bs.last_launch_name == want
    same = parity_every_instance(bs.get_solution(), bs.get_status(), ref, make, x0, kw, rho, tag=name + ", cold")
    print(f"{name}: cold, {same:.2f} of the iteration counts are the oracle's")
    # the second solve of a warm pair from a shifted x0; the first solve's exits are the GPU's own on both sides
    x1 = _f32(0.9 * x0)
    bs.set_warm_start(True)
    bs.reset()
    bs.solve()
    st0 = bs.get_status()
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
    parity_every_instance(bs.get_solution(), bs.get_status(), ref1, make_warm, x1, kw, rho, tag=name + ", warm pair, second")
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. compaction: instance index against dense slot
# ---------------------------------------------------------------------------------------------------------------------------
def test_compaction_indexes_rows_by_instance(hip_lib, oracle_built):
    Bn = 200
    case = _case("cartpole", batch=Bn)
    spread = np.linspace(0.05, 3.0, Bn)[np.random.default_rng(4).permutation(Bn)]       # iteration counts range widely
    case["x0"] = x0 = _f32(t.problems.cartpole_x0(Bn, seed=7) * spread[None, :])
    case["kw"] = kw = dict(TOL_KW, max_iter=60)
    rows, make, ref = _prepared(oracle_built, case, tag="compaction")
    assert len(np.unique(ref["iter"])) > 4 and 0 < ref["solved"].sum() < Bn
    runs = []
    for chunk in (0, 4):
        bs = _solver(case)
        bs.set_instance_linear(*rows)
        bs.set_compaction(chunk)
        bs.set_x0(x0)
        bs.solve()
        assert bs.last_launch_name == "stream4<4,1;il>"
        runs.append(_results(bs))
        bs.close()
    _identical(runs[0], runs[1], "single launch against chunks of 4 iterations")
    parity_every_instance(runs[1]["sol"], runs[1]["st"], ref, make, x0, kw, case["prob"].rho, tag="compaction")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. generic fallback
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [1, 2], ids=["precision1", "precision2"])
def test_generic_fallback(hip_lib, oracle_built, precision):
    case = _case("odd52")
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    prob.u_min, prob.u_max = _f32(prob.u_min), _f32(prob.u_max)      # (0.6 is no fp32 value: the oracle gets what the device holds)
    rows, make, ref = _prepared(oracle_built, case, tag=f"(5, 2) precision {precision}")
    want = "generic<f64;il>" if precision == 2 else "generic<il>"
    bs = _solver(case, precision=precision)
    bs.set_instance_linear(*rows)
    assert bs.kernel_name == want and bs.lin_mode() == 1
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
        r32 = _oracle_solves(_make_oracle(oracle_built, case, rows, kind="orc32"), [x0])
        limit, e32, share = precision1_limit(r32, ref)
        print(f"precision 1: limit {limit:.3e} (orc32 against orc64 {e32:.3e}, {share:.2f} of the instances agree on the exit)")
        parity_every_instance(sol, st, ref, make, x0, kw, prob.rho, tol=limit, tag="precision 1")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. routing and refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _plain_rows(case, seed=5):
    """rows that differ between instances without an oracle: the recipe's directions against x0's own scale"""
    prob, x0 = case["prob"], case["x0"]
    nx, nu, Bn = prob.nx, prob.nu, x0.shape[1]
    rng = np.random.default_rng(seed)
    Ax, Au = np.zeros((2, nx, Bn)), np.zeros((2, nu, Bn))
    th = rng.uniform(0.0, 2.0 * np.pi, Bn)
    Ax[0, 0, :], Ax[0, 1, :] = np.cos(th), np.sin(th)
    Ax[1, case["row"], :] = rng.uniform(0.5, 2.0, Bn)
    Ax = np.array(_f32(Ax))
    bx = np.stack([np.einsum("jb,jb->b", Ax[k], x0) + rng.uniform(0.01, 0.05, Bn) for k in range(2)])
    Au[0, 0, :], Au[1, nu - 1, :] = rng.uniform(0.5, 2.0, Bn), -rng.uniform(0.5, 2.0, Bn)
    bu = np.abs(np.stack([Au[0, 0, :], Au[1, nu - 1, :]])) * rng.uniform(0.2, 0.6, (2, Bn)) * np.abs(prob.u_max).max()
    return tuple(np.array(_f32(a)) for a in (Ax, bx, Au, bu))


def test_routing_round_trip_and_refusals(hip_lib, monkeypatch):
    monkeypatch.delenv("TINYMPC_HIP_STREAM_MPC", raising=False)
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), _f32(t.problems.cartpole_x0(B, seed=3))
    case = dict(prob=prob, x0=x0, row=1, kw=dict(TOL_KW, max_iter=40))
    rows = _plain_rows(case)
    none = (np.zeros((0, 4)), [], np.zeros((0, 1)), [])

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
    assert bs.kernel_name == home and bs.lin_mode() == 0
    bs.set_instance_linear(*rows)
    assert bs.kernel_name == "stream4<4,1;il>" and bs.lin_mode() == 1
    r_il = run(bs)
    assert bs.last_launch_name == "stream4<4,1;il>"
    assert not np.array_equal(r_il["sol"]["controls"], r_stay["sol"]["controls"])
    # per-instance bounds beside the rows: the same kernel under the same name; shared bounds leave the rows where they are
    shared_b = (prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_instance_bounds(*[np.repeat(a[:, :1], B, axis=1) for a in shared_b])
    assert bs.kernel_name == "stream4<4,1;il>" and bs.bounds_mode() == 1 and bs.lin_mode() == 1
    bs.reset()
    _identical(r_il, run(bs), "replicated per-instance bounds beside the rows")
    bs.set_bound_constraints(*shared_b)
    assert bs.kernel_name == "stream4<4,1;il>" and bs.bounds_mode() == 0 and bs.lin_mode() == 1
    # refused, each with a message
    nine = np.zeros((9, 4, B))
    nine[:, 0, :] = 1.0
    with pytest.raises(t.TinyMPCError, match="at most 8 rows"):
        bs.set_instance_linear(nine, np.ones((9, B)), None, None)
    with pytest.raises(t.TinyMPCError, match="null matrix or right-hand side"):
        bs._chk(bs.lib.tinympc_set_instance_linear(bs.h, None, 2, None, None, 0, None), "set_instance_linear")
    with pytest.raises(t.TinyMPCError, match="per-instance linear rows"):
        bs.set_adaptive_rho(True)
    with pytest.raises(t.TinyMPCError, match="per-instance linear rows"):
        bs.mpc_rollout(2)
    assert bs.lin_mode() == 1 and bs.kernel_name == "stream4<4,1;il>"
    # enable_linear off then on: no new upload, the same bits; off, the rows do not act
    bs.reset()
    bs.enable_linear(0, 0)
    r_off = run(bs)
    bs.enable_linear(1, 1)
    bs.reset()
    _identical(r_il, run(bs), "enable_linear off then on")
    assert not np.array_equal(r_off["sol"]["controls"], r_il["sol"]["controls"])
    # the shared entry point drops them: with no rows, back home, and to the bits of a solver that never left
    bs.set_linear_constraints(*none)
    assert bs.kernel_name == home and bs.lin_mode() == 0
    bs.reset()
    r_back = run(bs)
    assert bs.last_launch_name == home_launch
    _identical(r_stay, r_back, "after the round trip")
    bs.close()
    # ... and in the other order: per-instance rows on a solver that already adapts rho
    ad = _solver(case)
    ad.set_adaptive_rho(True)
    with pytest.raises(t.TinyMPCError, match="adaptive rho"):
        ad.set_instance_linear(*rows)
    assert ad.lin_mode() == 0
    ad.close()
    # per-instance families on a shape without the stream form's il kernels: refused, the solver stays as it was
    rng = np.random.default_rng(8)
    A2 = np.repeat(np.array([[1.0, 0.1], [0.0, 1.0]])[:, :, None], B, axis=2) * (1.0 + 0.02 * rng.uniform(-1, 1, (2, 2, B)))
    B2 = np.repeat(np.array([[0.005], [0.1]])[:, :, None], B, axis=2)
    fam = tuple(np.asfortranarray(m) for m in (A2, B2, np.repeat(np.eye(2)[:, :, None], B, axis=2), np.ones((1, 1, B)))) + (np.ones(B),)
    hs = t.BatchSolver.from_families(*fam, 8)
    name21 = hs.kernel_name
    a21 = np.zeros((1, 2, B))
    a21[0, 0, :] = 1.0
    with pytest.raises(t.TinyMPCError, match="per-instance linear rows need the stream kernel's il form"):
        hs.set_instance_linear(a21, np.ones((1, B)), None, None)
    assert hs.lin_mode() == 0 and hs.kernel_name == name21
    hs.close()
    # mixed widths on the process-global entry
    s = t.TinyMPCSolver()
    t.setup(s, prob.A, prob.B, np.zeros(4), prob.Q, prob.R, prob.rho, 4, 1, 20, batch=B)
    try:
        with pytest.raises(t.TinyMPCError, match="mixed widths"):
            t.set_linear_constraints(s, rows[0], rows[1], rows[2][:, :, 0], rows[3][:, 0])
    finally:
        t.cleanup()


def test_no_il_loop_kernel(hip_lib, monkeypatch):
    """under both stream switches the loop is still the chain: there is no `il` loop kernel to pick"""
    monkeypatch.setenv("TINYMPC_HIP_STREAM_MPC", "1")
    monkeypatch.setenv("TINYMPC_HIP_STREAM_LOOP", "1")
    case = _case("cartpole")
    case["kw"] = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=10, check_termination=1)
    bs = _solver(case)
    bs.set_instance_linear(*_plain_rows(case))
    bs.set_warm_start(True)
    bs.set_x0(case["x0"])
    bs.mpc_rollout(3)
    from tests.test_stream_loop_gpu import _launches
    assert bs.last_launch_name == "stream4<4,1;il>" and _launches(bs) == 3      # (one launch a step: the chain)
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. closed loop: both chains
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["stream_mpc", "own_plant"])
def test_closed_loop_chains(hip_lib, oracle_built, monkeypatch, chain):
    from tests.test_plant_loop_gpu import _rule_row
    if chain == "stream_mpc":
        monkeypatch.setenv("TINYMPC_HIP_STREAM_MPC", "1")
    else:
        monkeypatch.delenv("TINYMPC_HIP_STREAM_MPC", raising=False)
    steps = 5
    case = _case("cartpole")
    prob, x0 = case["prob"], case["x0"]
    kw = case["kw"] = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=15, check_termination=1)
    rows, make, ref = _prepared(oracle_built, case, tag=f"closed loop, {chain}")
    rng = np.random.default_rng(12)
    Ap = prob.A * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, prob.A.shape)) if chain == "own_plant" else prob.A
    Bp = prob.B * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, prob.B.shape)) if chain == "own_plant" else prob.B

    def solver():
        bs = _solver(case)
        bs.set_instance_linear(*rows)
        bs.set_warm_start(True)
        return bs
    bs = solver()
    if chain == "own_plant":
        bs.set_plant(Ap, Bp)
    bs.set_x0(x0)
    log = bs.mpc_rollout(steps)
    assert bs.kernel_name == "stream4<4,1;il>" and bs.last_launch_name == "stream4<4,1;il>"
    bs.close()
    # the first step against the oracle
    eu = nrel_batch(log["u"][:, :1, :], ref["u"][:, :1, :]).max()
    print(f"{chain}: first applied control against the oracle {eu:.3e}")
    assert eu <= FP32_TOL
    # the same loop stepped from the host on an identical solver, bit for bit
    hs = solver()
    x, f = np.array(x0, dtype=np.float64), np.zeros(prob.nx)
    for k in range(steps):
        hs.set_x0(_f32(x))
        hs.solve()
        u0, st = hs.get_solution()["controls"][:, 0, :], hs.get_status()
        x = np.array([[_rule_row(Ap, Bp, f, x[:, b], u0[:, b], r) for b in range(B)] for r in range(prob.nx)])
        assert np.array_equal(log["u"][:, k, :], u0), f"{chain}: step {k}, u log"
        assert np.array_equal(log["x"][:, k, :], _f32(x)), f"{chain}: step {k}, x log"
        assert np.array_equal(log["iter"][k], st["iter"]) and np.array_equal(log["solved"][k], st["solved"]), f"{chain}: step {k}"
    assert hs.last_launch_name == "stream4<4,1;il>"
    hs.close()
    # 3 + 2 steps are 5 steps
    two = solver()
    if chain == "own_plant":
        two.set_plant(Ap, Bp)
    two.set_x0(x0)
    la, lb = two.mpc_rollout(3), two.mpc_rollout(2)
    two.close()
    for key in ("x", "u"):
        assert np.array_equal(np.concatenate([la[key], lb[key]], axis=1), log[key]), f"{chain}: 3 + 2 steps, {key}"


# ---------------------------------------------------------------------------------------------------------------------------
# 7. sharded     8. process-global entry
# ---------------------------------------------------------------------------------------------------------------------------
def test_sharded_equals_single_handle(hip_lib):
    Bn = 37
    case = _case("cartpole", batch=Bn)
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    rows = _plain_rows(case)
    bs = _solver(case)
    bs.set_instance_linear(*rows)
    bs.set_x0(x0)
    bs.solve()
    one = _results(bs)
    bs.close()
    sh = t.ShardedBatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=Bn, n_gpus=2, devices=[0, 0])
    assert sh.fold_backend == "host"
    sh.update_settings(**kw)
    sh.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    sh.set_instance_linear(*rows)
    assert sh.kernel_names() == ["stream4<4,1;il>"] * 2
    sh.set_x0(x0)
    status = sh.solve()
    two = dict(sol=sh.get_solution(), st=sh.get_status(), status=status, ws=sh.get_workspace())
    sh.close()
    _identical(one, two, "two shards against one handle")
    assert len(np.unique(one["st"]["iter"])) > 2


def test_global_entry_takes_three_dimensional_rows(hip_lib):
    case = _case("cartpole")
    prob, x0, kw = case["prob"], case["x0"], case["kw"]
    rows = _plain_rows(case)
    bs = _solver(case)
    bs.set_instance_linear(*rows)
    bs.set_x0(x0)
    bs.solve()
    want = _results(bs, workspace=False)
    bs.close()
    s = t.TinyMPCSolver()
    try:
        t.setup(s, prob.A, prob.B, np.zeros(4), prob.Q, prob.R, prob.rho, 4, 1, prob.N, batch=B, max_iter=kw["max_iter"],
                abs_pri_tol=kw["abs_pri_tol"], abs_dua_tol=kw["abs_dua_tol"], check_termination=kw["check_termination"])
        t.set_bound_constraints(s, prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        t.set_linear_constraints(s, *rows)
        assert t.kernel_name() == "stream4<4,1;il>"
        t.set_x0(s, x0)
        status = t.solve(s)
        got = dict(sol=t.get_solution(s), st=t.get_status(s), status=status)
        assert t.kernel_name() == "stream4<4,1;il>"
    finally:
        t.cleanup()
    _identical(want, got, "global entry against BatchSolver.set_instance_linear")
