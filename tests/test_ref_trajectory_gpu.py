"""Reference trajectories windowed on the device (BatchSolver.set_ref_trajectory): with the cursor c the references of a solve
are x_ref[k] = x_traj[min(c + k, Lx - 1)], u_ref[k] = u_traj[min(c + k, Lu - 1)] (tinympc.ref_window), cut out of the
device-resident trajectory by ref_window_kernel (csrc/solver.hip) before a plain solve and before every step of mpc_rollout,
which such a solver runs as the own-plant chain (rollout_chain) and which leaves the cursor `steps` further on.

The reference is orc64, one persistent oracle per instance, stepped in numpy fp64 by the chain's rule: set_x0(f32(x)),
set_x_ref(ref_window(x_traj, c + t, N)), set_u_ref(ref_window(u_traj, c + t, N - 1)), solve, x+ = f_p + A_p x + B_p f32(u0) (+ w).
The comparison is tests/test_stream_loop_gpu.py's: every instance at FP32_TOL, an instance whose (iteration count, solved flag)
differs at a step is replayed with the GPU's decision imposed and may differ by one iteration; tolerance-terminated cases take
max_iter from the oracle's own counts so that both exits occur at some step, asserted from those counts.  Trajectories are
given as fp32-representable values, so the oracle and the GPU read the same references.

The oracle's states are asserted finite and bounded first, row by row: the references move the set point of a stable regulation
loop, so its state stays within the regulation transient (the same loop with zero references, and x0) plus the range of the
reference itself; the bound is twice their sum (the factor of tests/test_plant_loop_gpu.py).

 (1) cartpole N = 20, input bound, per-instance x_traj (a cart-position sinusoid, amplitude and phase per instance),
     L = steps + N - 1: the kernel a kept-workspace per-instance-reference solve takes, `steps` launches
 (2) quadrotor N = 10, fixed 10 iterations, per-instance x_traj and u_traj (quadrotor_tracking_refs shifted and scaled per
     instance), Lx = N + 2 and Lu = N: the clamp is live from step 3 and step 2; counts exact
 (3) rocket N = 12 on stream4<6,3>: cones, affine term, a SHARED trajectory (rocket_refs extended by its own shift; u_traj of
     one row), a per-instance plant and a per-instance disturbance
 (4) cartpole N = 17 on the generic kernel, and a per-instance-family solver, per-instance trajectories
 (5) precision 2 on generic<f64> at 1e-6 with exact counts; precision 1 against the host-stepped loop of the same solver
 (6) identities, bit for bit: the trajectory is `steps` x [set_x_ref(window), set_u_ref(window), mpc_rollout(1)], is
     `steps` x [set_ref_cursor(t), mpc_rollout(1)], and shared is set_ref_sequence of its windows
 (7) the cursor: 3 + 2 steps are 5, ref_cursor reads 5, set_ref_cursor(0) repeats the run, a plain solve reads the window at
     the cursor and leaves it
 (8) dropping returns the solver to its fused loop with the window at the cursor as ordinary references
 (9) under the closed-loop switches a trajectory solver keeps the chain and its results
 (10) the later setter wins
 (11) refusals, by a word of their message, each followed by a plain solve

Batch 70 (one full stream workgroup and a ragged wavefront), 5 steps.  Every test fails without the feature:
set_ref_trajectory does not exist there."""
import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.test_ref_sequence import quadrotor_tracking_refs
from tests.test_stream_loop_gpu import ROCKET_CONES, _collect, _configure, _f32, _identical, _launches, _rel, _tol
from tests.util import FP32_TOL, nrel

pytestmark = pytest.mark.gpu

B, STEPS = 70, 5
TIGHT = 1e-6
SWITCHES = ("TINYMPC_HIP_STREAM_MPC", "TINYMPC_HIP_STREAM_LOOP", "TINYMPC_HIP_NO_STREAM", "TINYMPC_HIP_STREAM_F64", "TINYMPC_HIP_NO_MFMAT",
            "TINYMPC_HIP_LEAN_WS", "TINYMPC_HIP_LEAN_LOOP")
ref_window = t.ref_window


# ---------------------------------------------------------------------------------------------------------------------------
# the trajectories and the cases
# ---------------------------------------------------------------------------------------------------------------------------
def _cart_sinusoid(L, seed):
    """(4, L, B): the cart position on a sinusoid, amplitude 0.05 .. 0.3 and phase per instance; the other states at zero"""
    rng = np.random.default_rng(seed)
    amp, phase = rng.uniform(0.05, 0.3, B), rng.uniform(0.0, 2.0 * np.pi, B)
    xt = np.zeros((4, L, B))
    xt[0] = amp[None, :] * np.sin(0.15 * np.arange(L)[:, None] + phase[None, :])
    return _f32(xt)


def _quad_trajectories(N, Lx, Lu, seed):
    """quadrotor_tracking_refs as ONE trajectory (its ramp in the knot index), shifted by 0 .. 4 rows and scaled by 0.5 .. 2 per
    instance: (12, Lx, B); inputs (4, Lu, B) a small per-instance wave (the tracking references' own are zero)"""
    rng = np.random.default_rng(seed)
    shift, scale = rng.integers(0, 5, B), rng.uniform(0.5, 2.0, B)
    xs, _ = quadrotor_tracking_refs(N, Lx + 5)
    base = np.concatenate([xs[:, :, 0], xs[:, -1, 1:]], axis=1)          # (12, N + Lx + 4)
    xt = np.stack([scale[b] * base[:, shift[b]:shift[b] + Lx] for b in range(B)], axis=2)
    j, a = np.arange(Lu)[None, :, None], np.arange(4)[:, None, None]
    ut = 0.02 * scale[None, None, :] * np.cos(0.3 * j + a + shift[None, None, :])
    return _f32(xt), _f32(ut)


def _cartpole20():
    prob = t.problems.cartpole(20, u_bound=0.5)
    return dict(prob=prob, x0=t.problems.cartpole_x0(B, seed=7), kw=_tol(8), xt=_cart_sinusoid(STEPS + 20 - 1, 41))


def _quadrotor10():
    prob = t.problems.quadrotor(10)
    kw = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=10, check_termination=1)
    xt, ut = _quad_trajectories(10, 12, 10, 42)
    return dict(prob=prob, x0=t.problems.quadrotor_x0(B, seed=5), kw=kw, xt=xt, ut=ut)


def _quadrotor10_shared():
    """the tracking references themselves as one shared trajectory: its windows are quadrotor_tracking_refs(10, STEPS)"""
    c = _quadrotor10()
    xs, us = quadrotor_tracking_refs(10, STEPS)
    return dict(c, xt=np.concatenate([xs[:, :, 0], xs[:, -1, 1:]], axis=1), ut=np.concatenate([us[:, :, 0], us[:, -1, 1:]], axis=1), seq=(xs, us))


def _rocket12():
    from tests.test_plant_loop_gpu import _disturbance, _perturbed
    prob = t.problems.rocket(12)
    rng = np.random.default_rng(43)
    x0 = t.problems.rocket_x0(B, seed=5)

    def ext(o):
        o.set_fdyn(prob.fdyn)
        o.set_cone_constraints(*ROCKET_CONES)
    A, Bm = _perturbed(prob, rng, True)
    fp = np.asfortranarray(np.repeat(prob.fdyn[:, None], B, axis=1) * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (6, B))))
    xt = _f32(t.problems.rocket_refs(12 + STEPS - 1)[0])      # (the interpolation goes on: window c is the reference shifted by c knots)
    ut = _f32(t.problems.rocket_refs(12)[1][:, :1])           # (one row, held: Lu = 1)
    return dict(prob=prob, x0=x0, kw=_tol(40), ext=ext, f=prob.fdyn, plant=(A, Bm, fp), w=_disturbance(x0, rng, STEPS, True), xt=xt, ut=ut,
                name="stream4<6,3>", env={"TINYMPC_HIP_NO_MFMAT": "1"})


def _cartpole17(generic):
    prob = t.problems.cartpole(17, u_bound=0.5)
    c = dict(prob=prob, x0=t.problems.cartpole_x0(B, seed=7), kw=_tol(12), xt=_cart_sinusoid(STEPS + 17 - 1, 44), name="stream4<4,1>", key="cartpole17")
    return dict(c, name="generic", env={"TINYMPC_HIP_NO_STREAM": "1"}) if generic else c


def _cartpole_families():
    base = t.problems.cartpole(17, u_bound=0.5)
    rng = np.random.default_rng(3)
    A = np.repeat(base.A[:, :, None], B, axis=2) * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, (4, 4, B)))
    Bm = np.repeat(base.B[:, :, None], B, axis=2) * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, (4, 1, B)))
    Q, R = np.repeat(base.Q[:, :, None], B, axis=2), np.repeat(base.R[:, :, None], B, axis=2)
    fam = tuple(np.asfortranarray(m) for m in (A, Bm, Q, R)) + (np.full(B, base.rho),)
    return dict(prob=base, x0=t.problems.cartpole_x0(B, seed=11), kw=_tol(12), fam=fam, xt=_cart_sinusoid(STEPS + 17 - 1, 45), name="stream4<4,1>")


def _quadrotor10_p2():
    prob = t.problems.quadrotor(10)
    prob.x_min, prob.x_max = np.full((12, 10), -0.5), np.full((12, 10), 0.5)
    xt, ut = _quad_trajectories(10, 12, 10, 46)
    return dict(prob=prob, x0=_f32(t.problems.quadrotor_x0(B, seed=8)), kw=_tol(40), precision=2, name="generic<f64>", xt=xt, ut=ut)


CASES = dict(cartpole20=_cartpole20, quadrotor10=_quadrotor10, quadrotor10_shared=_quadrotor10_shared, rocket12=_rocket12,
             cartpole17_generic=lambda: _cartpole17(True), cartpole17=lambda: _cartpole17(False), cartpole_families=_cartpole_families,
             quadrotor10_p2=_quadrotor10_p2)
_CASE_CACHE = {}


def _case(name):
    if name not in _CASE_CACHE:
        _CASE_CACHE[name] = dict(CASES[name](), id=name)
    return _CASE_CACHE[name]


def _model(case, b):
    if "fam" in case:
        A, Bm, Q, R, rho = case["fam"]
        return A[:, :, b], Bm[:, :, b], Q[:, :, b], R[:, :, b], float(rho[b])
    p = case["prob"]
    return p.A, p.B, p.Q, p.R, p.rho


def _plant_of(case, b):
    """instance b's (A_p, B_p, f_p): the installed plant, else the model with its affine term"""
    if "plant" not in case:
        A, Bm = _model(case, b)[:2]
        return A, Bm, np.asarray(case.get("f", np.zeros(case["prob"].nx)), dtype=np.float64)
    A, Bm, f = case["plant"]
    return A[:, :, b], Bm[:, :, b], f[:, b]


def _windows(case, cursor, b=None):
    """(x_ref, u_ref) of the solve at `cursor`: the whole batch's (what set_x_ref / set_u_ref take), or instance b's"""
    prob, xt, ut = case["prob"], case.get("xt"), case.get("ut")
    if xt is None:
        return None, None
    if b is not None and xt.ndim == 3:
        xt, ut = xt[:, :, b], None if ut is None else ut[:, :, b]
    xw = ref_window(xt, cursor, prob.N)
    uw = np.zeros((prob.nu, prob.N - 1) + xw.shape[2:]) if ut is None else ref_window(ut, cursor, prob.N - 1)
    return xw, uw


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's loops: computed once per case, shared, never written to
# ---------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_loop(oracle, case, b, steps, forced=None):
    prob = case["prob"]
    o = _configure(oracle.CpuSolver("orc64", *_model(case, b), prob.N), case)
    Ap, Bp, fp = _plant_of(case, b)
    x = np.array(case["x0"][:, b], dtype=np.float64)
    u_log, x_log = np.zeros((prob.nu, steps)), np.zeros((prob.nx, steps))
    it, so = np.zeros(steps, dtype=int), np.zeros(steps, dtype=int)
    r = None
    for k in range(steps):
        if forced is not None:
            o.set_forced_exit(int(forced[k][0]) if forced[k][1] else -1)
        o.set_x0(_f32(x))
        xw, uw = _windows(case, k, b)
        if xw is not None:
            o.set_x_ref(xw)
            o.set_u_ref(uw)
        o.solve()
        r = o.get_solution()
        u0 = _f32(r["u"][:, 0])
        x = Ap @ x + Bp @ u0 + fp + (case["w"][:, k, b] if "w" in case else 0.0)
        u_log[:, k], x_log[:, k], it[k], so[k] = u0, x, r["iter"], r["solved"]
    ws = o.get_state()
    o.close()
    return dict(u=u_log, x=x_log, iter=it, solved=so, last_x=np.array(r["x"]), last_u=np.array(r["u"]), ws=ws)


def _oracle_loops(oracle, case, steps=STEPS):
    key = (case.get("key", case["id"]), steps)
    if key not in _ORACLE:
        loops = [_oracle_loop(oracle, case, b, steps) for b in range(B)]
        so, x = np.stack([r["solved"] for r in loops], axis=-1), np.stack([r["x"] for r in loops], axis=-1)
        if case["kw"]["abs_pri_tol"] > 0.0:      # both exits in the batch at some step, by the oracle's own counts
            assert any(0 < so[k].sum() < B for k in range(steps)), (key, so.sum(axis=1))
        # finite, and bounded row by row (module docstring): regulation transient + the reference's range, twice
        nominal = {k: v for k, v in case.items() if k not in ("xt", "ut", "plant", "w")}
        xn = np.stack([_oracle_loop(oracle, nominal, b, steps)["x"] for b in range(B)], axis=-1)
        span = np.abs(case["xt"]).reshape(case["xt"].shape[0], -1).max(axis=1)
        bound = 2.0 * (np.maximum(np.abs(xn).max(axis=(1, 2)), np.abs(case["x0"]).max(axis=1)) + span)
        assert np.isfinite(x).all() and (np.abs(x).max(axis=(1, 2)) <= bound).all(), (key, np.abs(x).max(axis=(1, 2)) / bound)
        _ORACLE[key] = loops
    return _ORACLE[key]


def _stack(loops, key):
    return np.stack([r[key] for r in loops], axis=-1)


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU's runs
# ---------------------------------------------------------------------------------------------------------------------------
def _env(monkeypatch, case, extra=()):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in case.get("env", {}).items():
        monkeypatch.setenv(name, v)
    for name in extra:
        monkeypatch.setenv(name, "1")


def _solver(case, precision=None, traj=True, zero_w=False):
    prob = case["prob"]
    if "fam" in case:
        bs = t.BatchSolver.from_families(*case["fam"], prob.N)
    else:
        bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    _configure(bs, case)
    bs.set_warm_start(True)
    precision = case.get("precision", 0) if precision is None else precision
    if precision:
        bs.set_precision(precision)
        if precision == 1:
            bs.set_strict_precision(True)
    if "plant" in case:
        bs.set_plant(*case["plant"])
    if "w" in case or zero_w:
        bs.set_disturbance(case["w"] if "w" in case else np.zeros((prob.nx, STEPS)))
    if traj:
        bs.set_ref_trajectory(case["xt"], case.get("ut"))
        assert bs.ref_trajectory_mode() == (2 if case["xt"].ndim == 3 else 1) and bs.ref_cursor() == 0
    return bs


def _set_windows(bs, case, cursor):
    xw, uw = _windows(case, cursor)
    bs.set_x_ref(xw)
    bs.set_u_ref(uw)


def _plain_launch_name(case):
    """the kernel a kept-workspace solve takes with window 0 set as ordinary references, per instance or shared as the trajectory is"""
    bs = _solver(case, traj=False)
    _set_windows(bs, case, 0)
    bs.set_x0(case["x0"])
    bs.solve()
    name = bs.last_launch_name
    bs.close()
    return name


def _join(logs):
    return dict(status=logs[-1]["status"], x=np.concatenate([l["x"] for l in logs], axis=1), u=np.concatenate([l["u"] for l in logs], axis=1),
                iter=np.concatenate([l["iter"] for l in logs], axis=0), solved=np.concatenate([l["solved"] for l in logs], axis=0))


_RUNS = {}


def _run(monkeypatch, case, extra=(), zero_w=False):
    """mpc_rollout(STEPS) of the case's trajectory solver: the kernel, `steps` launches and the cursor asserted"""
    key = (case["id"], tuple(extra), zero_w)
    if key in _RUNS:
        return _RUNS[key]
    _env(monkeypatch, case, extra)
    want = _plain_launch_name(case)
    if "name" in case:
        assert want == case["name"], want
    bs = _solver(case, zero_w=zero_w)
    bs.set_x0(case["x0"])
    log = bs.mpc_rollout(STEPS)
    assert bs.last_launch_name == want, (bs.last_launch_name, want)
    assert _launches(bs) == STEPS, (_launches(bs), STEPS)
    assert bs.ref_cursor() == STEPS
    out = _collect(bs, log)
    bs.close()
    _RUNS[key] = out
    return out


def _check_vs_oracle(oracle, case, run, tol, exact):
    tag, log = case["id"], run["log"]
    loops = list(_oracle_loops(oracle, case))
    it, so = _stack(loops, "iter"), _stack(loops, "solved")
    same = np.all((log["iter"] == it) & (log["solved"] == so), axis=0)
    print(f"{tag}: {int(same.sum())} of {B} closed loops took the oracle's own iteration counts; iterations {it.min()}..{it.max()}, "
          f"converged per step {so.sum(axis=1)}")
    if exact:
        assert same.all(), f"{tag}: instances {np.nonzero(~same)[0]}"
    for b in np.nonzero(~same)[0]:
        assert np.abs(log["iter"][:, b] - it[:, b]).max() <= 1, f"{tag}: instance {b}: {log['iter'][:, b]} vs {it[:, b]}"
        loops[b] = _oracle_loop(oracle, case, b, STEPS, forced=[(log["iter"][k, b], log["solved"][k, b]) for k in range(STEPS)])
        assert np.array_equal(loops[b]["iter"], log["iter"][:, b]) and np.array_equal(loops[b]["solved"], log["solved"][:, b])
    eu, ex = _rel(log["u"], _stack(loops, "u")), _rel(log["x"], _stack(loops, "x"))
    print(f"{tag}: worst applied control {eu.max():.3e}, worst plant state {ex.max():.3e}")
    assert eu.max() <= tol, f"{tag}: applied controls, worst {eu.max():.3e} (instance {eu.argmax()})"
    assert ex.max() <= tol, f"{tag}: plant states, worst {ex.max():.3e} (instance {ex.argmax()})"
    wx = max(nrel(run["sol"]["states"][:, :, b], loops[b]["last_x"]) for b in range(B))
    wu = max(nrel(run["sol"]["controls"][:, :, b], loops[b]["last_u"]) for b in range(B))
    print(f"{tag}: last solve, worst states {wx:.3e}, worst controls {wu:.3e}")
    assert wx <= tol and wu <= tol, f"{tag}: last solve, states {wx:.3e} controls {wu:.3e}"
    assert np.array_equal(run["st"]["iter"], log["iter"][-1]) and np.array_equal(run["st"]["solved"], log["solved"][-1])
    assert np.array_equal(run["x0"], log["x"][:, -1, :].T.astype(np.float32)), f"{tag}: x0 is not the last plant state"
    return loops


def _references_act(oracle, case):
    """the trajectory moves the loop: the oracle's applied controls differ from the zero-reference loop's by far more than the bar"""
    nominal = {k: v for k, v in case.items() if k not in ("xt", "ut")}
    u = _stack(_oracle_loops(oracle, case), "u")
    un = np.stack([_oracle_loop(oracle, nominal, b, STEPS)["u"] for b in range(0, B, 10)], axis=-1)
    assert np.abs(u[:, :, ::10] - un).max() > 1e3 * FP32_TOL * np.abs(u).max()


# ---------------------------------------------------------------------------------------------------------------------------
# (1) - (4) against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole20", "quadrotor10", "rocket12", "cartpole17_generic", "cartpole_families"])
def test_trajectory_chain_vs_oracle(hip_lib, oracle_built, monkeypatch, name):
    case = _case(name)
    run = _run(monkeypatch, case)
    fixed = case["kw"]["abs_pri_tol"] == 0.0
    _check_vs_oracle(oracle_built, case, run, FP32_TOL, exact=fixed)
    if fixed:
        assert np.all(run["log"]["iter"] == case["kw"]["max_iter"]) and not run["log"]["solved"].any()
    _references_act(oracle_built, case)
    if name == "quadrotor10":       # (the clamp is live: Lx = N + 2, Lu = N — from step 3 / step 2 on the windows hold the last row)
        N = case["prob"].N
        assert case["xt"].shape[1] == N + 2 and case["ut"].shape[1] == N
        assert np.array_equal(ref_window(case["xt"], 3, N)[:, -1], case["xt"][:, -1]) and np.array_equal(ref_window(case["xt"], 3, N)[:, -2], case["xt"][:, -1])
        assert np.array_equal(ref_window(case["ut"], 2, N - 1)[:, -2], case["ut"][:, -1])
        assert np.any(case["xt"][:, -1] != case["xt"][:, -2]) and np.any(case["ut"][:, -1] != case["ut"][:, -2])


# ---------------------------------------------------------------------------------------------------------------------------
# (5) precision 2 and precision 1
# ---------------------------------------------------------------------------------------------------------------------------
def test_precision2(hip_lib, oracle_built, monkeypatch):
    case = _case("quadrotor10_p2")
    run = _run(monkeypatch, case)
    loops = _check_vs_oracle(oracle_built, case, run, TIGHT, exact=True)
    for key in ("d", "y", "g", "v", "z"):
        e = max(np.abs(run["ws"][key][:, :, b] - loops[b]["ws"][key]).max() / max(np.abs(loops[b]["ws"][key]).max(), 1e-2) for b in range(B))
        assert e <= TIGHT, f"workspace {key} {e:.3e}"


def test_precision1_vs_host_stepped(hip_lib, monkeypatch):
    """precision 1: the chain against the loop a caller steps on the same solver with set_x_ref / set_u_ref of every window"""
    case = _case("cartpole17")
    prob = case["prob"]
    _env(monkeypatch, case)
    bs = _solver(case, precision=1)
    bs.set_x0(case["x0"])
    log = bs.mpc_rollout(STEPS)
    assert bs.last_launch_name == "stream4<4,1>" and bs.effective_precision == 1 and _launches(bs) == STEPS
    sol = bs.get_solution()
    bs.close()
    hs = _solver(case, precision=1, traj=False)
    x = np.array(case["x0"], dtype=np.float64)
    u, xl = np.zeros((1, STEPS, B)), np.zeros((4, STEPS, B))
    it, so = np.zeros((STEPS, B), dtype=int), np.zeros((STEPS, B), dtype=int)
    for k in range(STEPS):
        hs.set_x0(_f32(x))
        _set_windows(hs, case, k)
        hs.solve()
        assert hs.last_launch_name == "stream4<4,1>"
        s, st = hs.get_solution(), hs.get_status()
        u[:, k, :] = s["controls"][:, 0, :]
        x = prob.A @ x + prob.B @ u[:, k, :]
        xl[:, k, :], it[k], so[k] = x, st["iter"], st["solved"]
    assert np.array_equal(it, log["iter"]) and np.array_equal(so, log["solved"])
    assert 0 < so.sum() < so.size, "one kind of exit only"
    eu, ex = _rel(log["u"], u), _rel(log["x"], xl)
    print(f"precision 1: chain vs host-stepped loop, controls {eu.max():.3e} states {ex.max():.3e}")
    assert eu.max() <= FP32_TOL and ex.max() <= FP32_TOL
    assert max(nrel(sol["controls"][:, :, b], s["controls"][:, :, b]) for b in range(B)) <= FP32_TOL
    assert max(nrel(sol["states"][:, :, b], s["states"][:, :, b]) for b in range(B)) <= FP32_TOL
    hs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (6) identities
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole20", "quadrotor10"])
def test_trajectory_is_the_windows_set_step_by_step(hip_lib, monkeypatch, name):
    """a solver under an all-zero disturbance runs the same chain without a trajectory: set_x_ref / set_u_ref of every step's
    window and mpc_rollout(1), `steps` times, is the trajectory's mpc_rollout(steps); so is set_ref_cursor(t) and mpc_rollout(1)"""
    case = _case(name)
    whole = _run(monkeypatch, case, zero_w=True)
    assert np.abs(whole["log"]["u"]).max() > 0.0 and len(np.unique(whole["log"]["x"][:, -1, :])) > B
    _env(monkeypatch, case)
    bs = _solver(case, traj=False, zero_w=True)
    bs.set_x0(case["x0"])
    logs = []
    for k in range(STEPS):
        _set_windows(bs, case, k)
        logs.append(bs.mpc_rollout(1))
        assert _launches(bs) == 1 and bs.ref_trajectory_mode() == 0
    _identical(_collect(bs, _join(logs)), whole, f"{name}: windows set step by step")
    bs.close()
    bs = _solver(case, zero_w=True)
    bs.set_x0(case["x0"])
    logs = []
    for k in (0, 1, 2, 3, 4):
        bs.set_ref_cursor(k)
        logs.append(bs.mpc_rollout(1))
        assert bs.ref_cursor() == k + 1
    _identical(_collect(bs, _join(logs)), whole, f"{name}: the cursor set step by step")
    bs.close()


def test_shared_trajectory_is_the_sequence_of_its_windows(hip_lib, monkeypatch):
    case = _case("quadrotor10_shared")
    mine = _run(monkeypatch, case, zero_w=True)
    _env(monkeypatch, case)
    bs = _solver(case, traj=False, zero_w=True)
    xs = np.stack([ref_window(case["xt"], c, 10) for c in range(STEPS)], axis=2)
    us = np.stack([ref_window(case["ut"], c, 9) for c in range(STEPS)], axis=2)
    assert np.array_equal(xs, case["seq"][0]) and np.array_equal(us, case["seq"][1])
    bs.set_ref_sequence(xs, us)
    bs.set_x0(case["x0"])
    log = bs.mpc_rollout(STEPS)
    assert _launches(bs) == STEPS
    _identical(_collect(bs, log), mine, "shared trajectory vs sequence")
    bs.close()
    assert len(np.unique(mine["log"]["x"][:, -1, :])) > B


# ---------------------------------------------------------------------------------------------------------------------------
# (7) the cursor
# ---------------------------------------------------------------------------------------------------------------------------
def test_cursor(hip_lib, monkeypatch):
    case = _case("cartpole20")
    whole = _run(monkeypatch, case)
    _env(monkeypatch, case)
    bs = _solver(case)
    bs.set_x0(case["x0"])
    logs = [bs.mpc_rollout(3)]
    assert bs.ref_cursor() == 3
    logs.append(bs.mpc_rollout(2))
    assert bs.ref_cursor() == 5
    _identical(_collect(bs, _join(logs)), whole, "3 + 2 vs 5")
    bs.set_ref_cursor(0)
    bs.reset()
    bs.set_x0(case["x0"])
    again = _collect(bs, bs.mpc_rollout(STEPS))
    assert bs.ref_cursor() == 5
    _identical(again, whole, "the repeat from cursor 0")
    # a plain solve reads the window at the cursor and leaves the cursor
    bs.set_ref_cursor(2)
    bs.reset()
    bs.set_x0(case["x0"])
    assert bs.solve() in (0, 1) and bs.ref_cursor() == 2 and _launches(bs) == STEPS
    got = (bs.get_solution(), bs.get_status(), bs.get_workspace(), bs.last_launch_name)
    assert bs.solve() in (0, 1) and bs.ref_cursor() == 2      # (a second solve: the window is there already)
    bs.close()
    other = _solver(case, traj=False)
    _set_windows(other, case, 2)
    other.set_x0(case["x0"])
    other.solve()
    want = (other.get_solution(), other.get_status(), other.get_workspace(), other.last_launch_name)
    other.close()
    assert got[3] == want[3]
    for a, c in zip(got[:3], want[:3]):
        for key in c:
            assert np.array_equal(a[key], c[key]), key
    assert np.abs(want[0]["controls"]).max() > 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# (8) dropping
# ---------------------------------------------------------------------------------------------------------------------------
def test_dropping_leaves_the_window_at_the_cursor(hip_lib, monkeypatch):
    case = _case("cartpole20")
    _env(monkeypatch, case)
    fresh = _solver(case, traj=False)
    _set_windows(fresh, case, STEPS)
    fresh.set_x0(case["x0"])
    want = _collect(fresh, fresh.mpc_rollout(STEPS))
    assert _launches(fresh) == 1                      # (the fused loop, its per-instance references frozen)
    name = fresh.last_launch_name
    fresh.close()
    bs = _solver(case)
    bs.set_x0(case["x0"])
    bs.mpc_rollout(STEPS)
    assert _launches(bs) == STEPS and bs.ref_cursor() == STEPS
    bs.set_ref_trajectory(None)
    assert bs.ref_trajectory_mode() == 0
    bs.reset()
    bs.set_x0(case["x0"])
    got = _collect(bs, bs.mpc_rollout(STEPS))
    assert _launches(bs) == 1 and bs.last_launch_name == name
    _identical(got, want, "after dropping")
    bs.close()
    whole = _run(monkeypatch, case)
    assert not np.array_equal(whole["log"]["u"], want["log"]["u"])      # (frozen references are another loop)


# ---------------------------------------------------------------------------------------------------------------------------
# (9) the closed-loop switches
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [("TINYMPC_HIP_LEAN_WS",), ("TINYMPC_HIP_LEAN_LOOP",), ("TINYMPC_HIP_STREAM_MPC",), ("TINYMPC_HIP_STREAM_LOOP",),
                                   ("TINYMPC_HIP_LEAN_WS", "TINYMPC_HIP_LEAN_LOOP"), ("TINYMPC_HIP_STREAM_MPC", "TINYMPC_HIP_STREAM_LOOP")],
                         ids=lambda e: "+".join(n[len("TINYMPC_HIP_"):] for n in e))
def test_switches_keep_the_chain(hip_lib, monkeypatch, extra):
    case = _case("cartpole20")
    chain = _run(monkeypatch, case)
    switched = _run(monkeypatch, case, extra=extra)      # (`steps` launches: asserted in _run)
    _identical(switched, chain, "+".join(extra))


# ---------------------------------------------------------------------------------------------------------------------------
# (10) the later setter wins
# ---------------------------------------------------------------------------------------------------------------------------
def test_setter_interplay(hip_lib, monkeypatch):
    case = _case("quadrotor10")
    seq = quadrotor_tracking_refs(10, STEPS)
    _env(monkeypatch, case)
    bs = _solver(case)
    bs.set_ref_sequence(*seq)
    assert bs.ref_trajectory_mode() == 0
    bs.set_ref_trajectory(case["xt"], case["ut"])
    assert bs.ref_trajectory_mode() == 2
    bs.set_precision(1)                       # (a change of precision keeps the trajectory)
    assert bs.ref_trajectory_mode() == 2
    bs.set_precision(0)
    bs.set_x_ref(_windows(case, 0)[0])
    assert bs.ref_trajectory_mode() == 0
    bs.set_ref_trajectory(case["xt"][:, :, 0], case["ut"][:, :, 0])
    assert bs.ref_trajectory_mode() == 1
    bs.set_u_ref(_windows(case, 0)[1])
    assert bs.ref_trajectory_mode() == 0
    bs.set_ref_trajectory(case["xt"], case["ut"])
    bs.set_ref_mode(1)
    assert bs.ref_trajectory_mode() == 0
    # a sequence beside per-instance references is refused; the per-instance trajectory after it runs, as case (2) ran
    bs.set_ref_sequence(*seq)
    bs.set_x_ref(_windows(case, 0)[0])
    bs.set_x0(case["x0"])
    with pytest.raises(t.TinyMPCError, match="shared by the batch"):
        bs.mpc_rollout(STEPS)
    assert _launches(bs) == -1
    bs.set_ref_trajectory(case["xt"], case["ut"])
    got = _collect(bs, bs.mpc_rollout(STEPS))
    assert _launches(bs) == STEPS and bs.ref_cursor() == STEPS
    bs.close()
    _identical(got, _run(monkeypatch, case), "a trajectory after a sequence")


# ---------------------------------------------------------------------------------------------------------------------------
# (11) refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["adaptive", "cold", "instance_bounds", "short_disturbance"])
def test_rollout_refusals(hip_lib, monkeypatch, what):
    case = _case("cartpole17")
    prob = case["prob"]
    _env(monkeypatch, case)
    bs = _solver(case)
    bs.set_x0(case["x0"])
    if what == "adaptive":
        bs.set_adaptive_rho(True)
        want = "a reference trajectory is not available with adaptive rho"
    elif what == "cold":
        bs.set_warm_start(False)
        want = "needs the persistent workspace"
    elif what == "instance_bounds":
        bs.set_instance_bounds(np.full((4, B), -1e17), np.full((4, B), 1e17), np.full((1, B), -0.5), np.full((1, B), 0.5))
        want = "per-instance bounds have no closed loop by default"
    else:
        bs.set_disturbance(np.zeros((prob.nx, 3)))
        want = "the disturbance holds 3 steps"
    with pytest.raises(t.TinyMPCError, match=want):
        bs.mpc_rollout(STEPS)
    assert _launches(bs) == -1 and bs.ref_cursor() == 0 and bs.ref_trajectory_mode() == 2
    if what == "adaptive":
        bs.set_adaptive_rho(False)
    assert bs.solve() in (0, 1) and np.isfinite(bs.get_solution()["controls"]).all()
    bs.close()


def test_setter_refusals(hip_lib, monkeypatch):
    case = _case("cartpole17")
    _env(monkeypatch, case)
    bs = _solver(case, traj=False)
    bs.set_x0(case["x0"])
    xt = case["xt"]
    ut = np.zeros((1, 6, B))
    for args, word in (((xt[:3],), "expected"),                                   # wrong row count
                       ((xt, np.zeros((2, 6, B))), "expected"),
                       ((xt[:, :0],), "Lx, Lu >= 1"),                            # Lx < 1
                       ((xt, ut[:, :0]), "Lx, Lu >= 1"),                         # Lu < 1 with a u_traj
                       ((xt[:, :, :B - 1],), "expected"),                        # a per-instance width that is not L * batch
                       ((xt, ut[:, :, :B - 1]), "expected"),
                       ((xt[:, :, 0], ut), "both shared or both per instance"),  # a per-instance u_traj beside a shared x_traj
                       ((xt, ut[:, :, 0]), "both shared or both per instance"),  # ... and the reverse
                       ((xt[0],), "expected")):
        with pytest.raises(t.TinyMPCError, match=word):
            bs.set_ref_trajectory(*args)
        assert bs.ref_trajectory_mode() == 0
    # the library's own checks, through the handle
    flat = np.ascontiguousarray(xt.reshape(-1, order="F"))
    ptr = flat.ctypes.data_as(t.tinympc.c_dp)
    for args, word in (((ptr, 0, None, 0, 1), "Lx >= 1"), ((ptr, 5, ptr, 0, 1), "Lu >= 1"), ((ptr, 5, None, 0, 2), "per_instance")):
        assert bs.lib.tinympc_set_ref_trajectory(bs.h, *args) == -1
        assert word in bs.lib.tinympc_last_error().decode()
    with pytest.raises(t.TinyMPCError, match="0 or more"):
        bs.set_ref_cursor(-1)
    assert bs.ref_trajectory_mode() == 0 and bs.ref_cursor() == 0
    assert bs.solve() in (0, 1)
    bs.close()


def test_global_forms(hip_lib, monkeypatch):
    """the process-global solver: set_ref_trajectory / set_ref_cursor / ref_cursor, the library's own shape checks, and the refusal
    under set_gpus (one device, listed twice)"""
    case = _case("cartpole20")
    _env(monkeypatch, case)
    monkeypatch.delenv("TINYMPC_HIP_SHARD_DEVICES", raising=False)
    prob, xt = case["prob"], case["xt"]
    s = t.TinyMPCSolver()
    try:
        t.setup(s, prob.A, prob.B, None, prob.Q, prob.R, prob.rho, 4, 1, prob.N, batch=B, **case["kw"])
        t.set_bound_constraints(s, prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        for args in ((xt[:3],), (xt[:, :, :B - 1],), (xt, np.zeros((2, 6, B))), (xt, np.zeros((1, 6, B - 1)))):
            with pytest.raises(t.TinyMPCError, match="expected"):
                t.set_ref_trajectory(s, *args)
        t.set_ref_trajectory(s, xt)
        assert t.ref_cursor(s) == 0
        with pytest.raises(t.TinyMPCError, match="0 or more"):
            t.set_ref_cursor(s, -2)
        t.set_x0(s, case["x0"])
        log = t.mpc_rollout(s, STEPS)
        assert t.ref_cursor(s) == STEPS
        ref = _run(monkeypatch, case)["log"]
        for key in ("x", "u", "iter", "solved"):
            assert np.array_equal(log[key], ref[key]), key
        t.set_ref_cursor(s, 1)
        assert t.ref_cursor(s) == 1
        # re-batching drops the trajectory like every per-instance input: the loop is the zero-reference solver's, the cursor stays
        t.set_batch_size(s, B)
        t.set_x0(s, case["x0"])
        log = t.mpc_rollout(s, STEPS)
        bs = _solver(case, traj=False)
        bs.set_x0(case["x0"])
        ref = bs.mpc_rollout(STEPS)
        assert _launches(bs) == 1
        bs.close()
        for key in ("x", "u", "iter", "solved"):
            assert np.array_equal(log[key], ref[key]), key
        assert t.ref_cursor(s) == 1
        t.set_ref_trajectory(s, None)
        monkeypatch.setenv("TINYMPC_HIP_SHARD_DEVICES", "0,0")
        t.set_gpus(s, 2)
        for call, word in ((lambda: t.set_ref_trajectory(s, xt), "set_ref_trajectory"), (lambda: t.set_ref_cursor(s, 0), "set_ref_cursor"),
                           (lambda: t.ref_cursor(s), "ref_cursor")):
            with pytest.raises(t.TinyMPCError, match=word + ": not available on a sharded solver"):
                call()
        t.set_x0(s, case["x0"])
        assert t.solve(s) in (0, 1)
    finally:
        t.cleanup()
