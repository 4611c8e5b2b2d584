"""mpc_rollout under output feedback: measured outputs y = C x + v and a fixed-gain state estimator stepped on the device
(BatchSolver.set_estimator; csrc/estimator.h, csrc/estimator.hip: estimator_step_kernel).

The rule, with the noise cursor c and loop step s, t = c + s: y_t = C x_t + v_t (x_t the true fp64 plant state, v_t the first ny rows
of G_v xi_v[b][t]); xhat_t = xhat-_t + L (y_t - C xhat-_t); the solve of step s starts from float32(xhat_t); the plant step is
unchanged; xhat-_{t+1} = f + A xhat_t + B u_t with the MODEL.  The reference is orc64 stepped by that rule in numpy fp64 and fed the
DEVICE's own draws (get_noise), compared as tests/test_noise_loop_gpu.py compares: every instance at FP32_TOL on applied control,
true state, xhat log and y log, an instance whose (iteration count, solved flag) differs at a step replayed with the GPU's decision
imposed.  The rule itself is held to a numpy restatement by tests/test_estimator.py.

Initial estimate: xhat-_0 = x0 + sign * U(0.05, 0.10) * scale_r per instance and row (scale_r the largest |x0| of row r over the
batch), installed with set_estimator_state; gains from kalman_gain with the case's noise factors (a case without measurement or
process noise: 0.003 scale, the noise tests' size).  Not vacuous, on the oracle alone: on at least 90 % of the instances the applied
controls differ from the full-state loop's (same draws, the solve from float32(x + v)) by more than 1e-3 relative, and the xhat log
differs from the true state in every entry.  The cartpole cases start from a tenth of the other files' x0 (disturbance and noise
factors scaled alike): at the full size the input sits on its bound for all five steps on 41 of 70 instances whatever the solve
starts from, and that check missed on the oracle (29 of 70); the threshold stayed, the cases moved.

 (a) against orc64: cartpole N = 20 (ny = 2, per-instance plant, disturbance, both noises, per-instance C and L), quadrotor N = 10
     (ny = 6, reference sequence, fixed iterations: counts exact), rocket N = 12 on stream4<6,3> (ny = 3: f in the predict), cartpole
     N = 17 on the generic kernel (ny = 1), per-instance families on stream4<4,1> (the predict with A_b, B_b), a per-instance
     reference trajectory (both cursors at 5), ny = nx with C = I, precision 2 on generic<f64> at 1e-6 with exact counts, precision 1
     against a host-stepped loop that runs host_estimator_step
 (b) bit for bit: the fused schedule is TINYMPC_HIP_ESTIMATOR_SPLIT; 3 + 2 = 5; steps x mpc_rollout(1); two identical runs; the y log
     without measurement noise; dropping the estimator; metrics; the closed-loop switches
 (c) state: set_x0 moves the plant only, set_estimator_state(None) re-arms, x0 after a rollout
 (d) refusals, by a word of their message, each followed by a plain solve; the global forms

Batch 70, 5 steps: nx = 4 — one full 64-instance workgroup of the estimator's kernel and a ragged one; nx = 12 — 21 instances per
workgroup, 4 idle lanes, a ragged fourth; nx = 6 on stream4<6,3>.  Every test fails without the feature: the setters do not exist
there."""
import ctypes

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.test_noise_loop_gpu import SEED_V, SEED_W, _diag, _draws, _install_noise, _ncase, _without
from tests.test_noise_loop_gpu import _oracle_loop as _full_state_loop
from tests.test_plant_loop_gpu import B, STEPS, TIGHT, _case, _env, _model, _plant_of, _solver, _stack, _w_of
from tests.test_rollout_metrics import check_slots, restated
from tests.test_stream_loop_gpu import _collect, _configure, _f32, _identical, _launches, _rel
from tests.util import FP32_TOL, nrel

pytestmark = pytest.mark.gpu

SPLIT = "TINYMPC_HIP_ESTIMATOR_SPLIT"


# ---------------------------------------------------------------------------------------------------------------------------
# the cases: one of the noise / plant tests' cases plus the measured rows, the gains and the initial estimate
# ---------------------------------------------------------------------------------------------------------------------------
def _selector(nx, rows):
    return np.eye(nx)[list(rows)]


def _factors(case, shared):
    """the factors the gain is designed for: the case's own; the noise tests' nominal size where the case has none or — for a gain
    shared by the batch — one per instance (a design choice: any stabilising gain is an estimator)"""
    def pick(key):
        G = case.get(key)
        return _diag(case["x0"]) if G is None or (shared and G.ndim == 3) else G
    return pick("gw"), pick("gv")


def _with_estimator(base, rows, per_instance=False, seed=0, tag=None):
    """C picks `rows` (per instance: times a sensor gain in [0.9, 1.1]); L the steady-state Kalman gain of each instance's model, C and
    factors; xhat-_0 offset from x0 by 5 - 10 % of each row's scale"""
    prob, x0 = base["prob"], base["x0"]
    nx = prob.nx
    rng = np.random.default_rng(7000 + seed)
    several = per_instance or "fam" in base
    gw, gv = _factors(base, not several)
    sel = _selector(nx, rows)
    if several:
        gain = rng.uniform(0.9, 1.1, B) if per_instance else np.ones(B)
        C = np.asfortranarray(sel[:, :, None] * gain[None, None, :])
        L = np.zeros((nx, len(rows), B), order="F")
        for b in range(B):
            L[:, :, b] = t.kalman_gain(_model(base, b)[0], C[:, :, b], gw[:, :, b] if gw.ndim == 3 else gw, gv[:, :, b] if gv.ndim == 3 else gv)
    else:
        C = sel
        L = t.kalman_gain(prob.A, C, gw, gv)
    scale = np.abs(x0).max(axis=1)
    xhat0 = np.asfortranarray(_f32(x0) + rng.choice([-1.0, 1.0], (nx, B)) * rng.uniform(0.05, 0.10, (nx, B)) * scale[:, None])
    return dict(base, C=C, L=L, xhat0=xhat0, id="est_" + (tag or base["id"]))


CARTPOLE_SHRINK = 0.1


def _small(case):
    """the cartpole cases start so far out that the input sits on its bound for all five steps on most instances, whatever the solve
    starts from: x0, the disturbance and the noise factors (all proportional to x0's scale) a tenth of the other files', so that the
    applied control can show what the estimator does"""
    out = dict(case, x0=np.asfortranarray(CARTPOLE_SHRINK * case["x0"]))
    for key in ("w", "gw", "gv"):
        if key in case:
            out[key] = np.asfortranarray(CARTPOLE_SHRINK * case[key])
    return out


def _families_case():
    c = dict(_case("cartpole_families"))
    return dict(c, gw=_diag(c["x0"]), gv=_diag(c["x0"]))


BUILD = dict(
    cartpole20=lambda: _with_estimator(_small(_ncase("cartpole20")), (0, 2), per_instance=True, seed=1, tag="cartpole20"),
    quadrotor10_sequence=lambda: _with_estimator(_ncase("quadrotor10_sequence"), range(6), seed=2, tag="quadrotor10_sequence"),
    rocket12=lambda: _with_estimator(_ncase("rocket12"), (0, 1, 2), seed=3, tag="rocket12"),
    cartpole17_generic=lambda: _with_estimator(_small(_ncase("cartpole17_generic")), (0,), seed=4, tag="cartpole17_generic"),
    cartpole_families=lambda: _with_estimator(_small(_families_case()), (0, 2), seed=5, tag="cartpole_families"),
    cartpole20_trajectory=lambda: _with_estimator(_small(_ncase("cartpole20_trajectory")), (0, 2), seed=6, tag="cartpole20_trajectory"),
    cartpole17_identity=lambda: _with_estimator(_small(_ncase("cartpole17_plant")), range(4), seed=7, tag="cartpole17_identity"),
    quadrotor10_p2=lambda: _with_estimator(_ncase("quadrotor10_p2"), range(6), seed=8, tag="quadrotor10_p2"),
    cartpole17_plant=lambda: _with_estimator(_small(_ncase("cartpole17_plant")), (0, 2), per_instance=True, seed=9, tag="cartpole17_plant"),
    # process noise alone: the y log is float32(C x)
    cartpole20_quiet=lambda: _with_estimator(_small(_without(_ncase("cartpole20"), "gv")), (0, 2), seed=10, tag="cartpole20_quiet"),
    # the model as the plant and no disturbance: without the estimator and the noise the cartpole's fused loop
    cartpole20_model=lambda: _with_estimator(_small(_without(_ncase("cartpole20"), "plant", "w")), (0, 2), seed=11, tag="cartpole20_model"),
)
_CASES = {}


def _ecase(name):
    if name not in _CASES:
        _CASES[name] = BUILD[name]()
    return _CASES[name]


def _of(M, b):
    return M[:, :, b] if M.ndim == 3 else M


def _install(bs, case, state=True):
    _install_noise(bs, case)
    bs.set_estimator(case["C"], case["L"])
    if state:
        bs.set_estimator_state(case["xhat0"])


_RUNS = {}


def _run(monkeypatch, case, steps=STEPS, extra=(), split=None, keep=True, metrics=False):
    key = (case["id"], steps, tuple(extra), split, metrics)
    if keep and key in _RUNS:
        return _RUNS[key]
    _env(monkeypatch, case)
    monkeypatch.delenv(SPLIT, raising=False)
    for name in extra:
        monkeypatch.setenv(name, "1")
    bs = _solver(case)
    _install(bs, case)
    ny = case["C"].shape[0]
    assert bs.estimator_mode() == (2 if case["C"].ndim == 3 else 1) and int(bs.lib.tinympc_estimator_outputs(bs.h)) == ny
    assert np.array_equal(bs.get_estimator_state(), case["xhat0"])
    if metrics:
        bs.set_rollout_metrics(True)
    bs.set_x0(case["x0"])
    logs, done = [], 0
    for n in (split or (steps,)):
        if done and "w" in case:      # (the uploaded disturbance is read from row 0 whatever the cursor: its rows of this part)
            bs.set_disturbance(np.asfortranarray(case["w"][:, done:done + n]))
        logs.append(bs.mpc_rollout(n))
        done += n
        assert _launches(bs) == n, (_launches(bs), n)
        assert "y" not in logs[-1] and logs[-1]["xhat"].shape == (case["prob"].nx, n, B) and logs[-1]["yout"].shape == (ny, n, B)
    log = {k: np.concatenate([l[k] for l in logs], axis=0 if k in ("iter", "solved") else 1) for k in logs[0] if k != "status"}
    log["status"] = logs[-1]["status"]
    out = _collect(bs, log)
    out["cursor"], out["launched"], out["est"] = bs.noise_cursor(), bs.last_launch_name, bs.get_estimator_state()
    out["nw"], out["nv"] = _draws(bs, case, 0, steps)
    if metrics:
        out["metrics"] = bs.get_rollout_metrics()
    if "xt" in case:
        out["ref_cursor"] = bs.ref_cursor()
    for name in extra:
        monkeypatch.delenv(name, raising=False)
    bs.close()
    if keep:
        _RUNS[key] = out
    return out


def _same(a, c, tag):
    _identical(a, c, tag)
    for key in ("xhat", "yout"):
        assert np.array_equal(a["log"][key], c["log"][key]), f"{tag}: log {key}"
    assert np.array_equal(a["est"], c["est"]), f"{tag}: the estimate left behind"


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's loops, stepped by the rule with the device's draws
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle_loop(oracle, case, b, steps, nw, nv, forced=None):
    prob = case["prob"]
    Am, Bm = _model(case, b)[:2]
    fm = np.asarray(case.get("f", np.zeros(prob.nx)), dtype=np.float64)
    o = _configure(oracle.CpuSolver("orc64", *_model(case, b), prob.N), case)
    Ap, Bp, fp = _plant_of(case, b)
    C, L = _of(case["C"], b), _of(case["L"], b)
    ny = C.shape[0]
    x = np.array(_f32(case["x0"][:, b]), dtype=np.float64)
    xh = np.array(case["xhat0"][:, b], dtype=np.float64)
    u_log, x_log, xh_log, y_log = np.zeros((prob.nu, steps)), np.zeros((prob.nx, steps)), np.zeros((prob.nx, steps)), np.zeros((ny, steps))
    true_log = np.zeros((prob.nx, steps))      # the true state every step's measurement was taken of
    it, so = np.zeros(steps, dtype=int), np.zeros(steps, dtype=int)
    r = None
    for k in range(steps):
        if forced is not None:
            o.set_forced_exit(int(forced[k][0]) if forced[k][1] else -1)
        y = C @ x + (0.0 if nv is None else nv[:ny, k, b])
        xh = xh + L @ (y - C @ xh)
        true_log[:, k] = x
        o.set_x0(_f32(xh))
        if "seq" in case:
            o.set_x_ref(case["seq"][0][:, :, k])
            o.set_u_ref(case["seq"][1][:, :, k])
        if "xt" in case:
            o.set_x_ref(t.ref_window(_f32(case["xt"][:, :, b]), k, prob.N))
            o.set_u_ref(t.ref_window(_f32(case["ut"][:, :, b]), k, prob.N - 1))
        o.solve()
        r = o.get_solution()
        u0 = _f32(r["u"][:, 0])
        x = ((Ap @ x + Bp @ u0 + fp) + _w_of(case, b, k)) + (0.0 if nw is None else nw[:, k, b])
        u_log[:, k], x_log[:, k], xh_log[:, k], y_log[:, k], it[k], so[k] = u0, x, xh, y, r["iter"], r["solved"]
        xh = fm + Am @ xh + Bm @ u0
    ws = o.get_state()
    o.close()
    return dict(u=u_log, x=x_log, xhat=xh_log, yout=y_log, true=true_log, est=xh, iter=it, solved=so, last_x=np.array(r["x"]), last_u=np.array(r["u"]), ws=ws)


_ORACLE = {}


def _oracle_loops(oracle, case, run):
    """the case's oracle loops, once, never written to; asserted bounded and NOT VACUOUS first: the estimator changes what is applied"""
    key = case["id"]
    if key not in _ORACLE:
        loops = [_oracle_loop(oracle, case, b, STEPS, run["nw"], run["nv"]) for b in range(B)]
        x = _stack(loops, "x")
        nominal = _without(case, "plant", "w")
        xn = np.stack([_full_state_loop(oracle, nominal, b, STEPS, None, None)["x"] for b in range(B)], axis=-1)
        # (a guard against a diverging loop, not a performance bound: an estimate up to 10 % of every row's scale off — the slow and
        # the unmeasured rows' included — steers the plant away from the full-state loop's path, but within the order of magnitude)
        bound = 10.0 * np.maximum(np.abs(xn).max(axis=(1, 2)), np.abs(case["x0"]).max(axis=1))
        assert np.isfinite(x).all() and (np.abs(x).max(axis=(1, 2)) <= bound).all(), (key, np.abs(x).max(axis=(1, 2)) / bound)
        full = np.stack([_full_state_loop(oracle, case, b, STEPS, run["nw"], run["nv"])["u"] for b in range(B)], axis=-1)
        du = _rel(_stack(loops, "u"), full)
        print(f"{key}: controls against the full-state loop's differ by more than 1e-3 relative on {int((du > 1e-3).sum())} of {B} instances (median {np.median(du):.2e})")
        assert np.mean(du > 1e-3) >= 0.9, (key, np.sort(du)[:10])
        assert np.all(_f32(_stack(loops, "xhat")) != _f32(_stack(loops, "true"))), f"{key}: an estimate equals the true state"
        _ORACLE[key] = loops
    return _ORACLE[key]


def _check_vs_oracle(oracle, case, run, tol, exact):
    tag, log = case["id"], run["log"]
    loops = list(_oracle_loops(oracle, case, run))
    it, so = _stack(loops, "iter"), _stack(loops, "solved")
    same = np.all((log["iter"] == it) & (log["solved"] == so), axis=0)
    print(f"{tag}: {int(same.sum())} of {B} closed loops took the oracle's own iteration counts; iterations {it.min()}..{it.max()}, "
          f"converged per step {so.sum(axis=1)}")
    if exact:
        assert same.all(), f"{tag}: instances {np.nonzero(~same)[0]}"
    for b in np.nonzero(~same)[0]:
        assert np.abs(log["iter"][:, b] - it[:, b]).max() <= 1, f"{tag}: instance {b}: {log['iter'][:, b]} vs {it[:, b]}"
        loops[b] = _oracle_loop(oracle, case, b, STEPS, run["nw"], run["nv"], forced=[(log["iter"][k, b], log["solved"][k, b]) for k in range(STEPS)])
        assert np.array_equal(loops[b]["iter"], log["iter"][:, b]) and np.array_equal(loops[b]["solved"], log["solved"][:, b])
    errs = {k: _rel(log[k], _stack(loops, k)) for k in ("u", "x", "xhat", "yout")}
    print(f"{tag}: worst applied control {errs['u'].max():.3e}, plant state {errs['x'].max():.3e}, estimate {errs['xhat'].max():.3e}, output {errs['yout'].max():.3e}")
    for k, e in errs.items():
        assert e.max() <= tol, f"{tag}: log {k}, worst {e.max():.3e} (instance {e.argmax()})"
    ee = nrel(run["est"], _stack(loops, "est"))
    assert ee <= tol, f"{tag}: the estimate left behind {ee:.3e}"
    wx = max(nrel(run["sol"]["states"][:, :, b], loops[b]["last_x"]) for b in range(B))
    wu = max(nrel(run["sol"]["controls"][:, :, b], loops[b]["last_u"]) for b in range(B))
    print(f"{tag}: last solve, worst states {wx:.3e}, worst controls {wu:.3e}")
    assert wx <= tol and wu <= tol, f"{tag}: last solve, states {wx:.3e} controls {wu:.3e}"
    assert np.array_equal(run["st"]["iter"], log["iter"][-1]) and np.array_equal(run["st"]["solved"], log["solved"][-1])
    assert np.array_equal(run["x0"], log["x"][:, -1, :].T.astype(np.float32)), f"{tag}: x0 is not the rounding of the last TRUE plant state"
    return loops


# ---------------------------------------------------------------------------------------------------------------------------
# (a) against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole20", "quadrotor10_sequence", "rocket12", "cartpole17_generic", "cartpole_families", "cartpole20_trajectory",
                                  "cartpole17_identity"])
def test_estimator_chain_vs_oracle(hip_lib, oracle_built, monkeypatch, name):
    case = _ecase(name)
    run = _run(monkeypatch, case)
    if "name" in case:
        assert run["launched"] == case["name"], run["launched"]
    assert run["cursor"] == STEPS
    fixed = case["kw"]["abs_pri_tol"] == 0.0
    _check_vs_oracle(oracle_built, case, run, FP32_TOL, exact=fixed)
    if fixed:
        assert np.all(run["log"]["iter"] == case["kw"]["max_iter"]) and not run["log"]["solved"].any()
    if "xt" in case:        # both cursors advance
        assert run["ref_cursor"] == STEPS


def test_precision2(hip_lib, oracle_built, monkeypatch):
    case = _ecase("quadrotor10_p2")
    run = _run(monkeypatch, case)
    assert run["launched"] == "generic<f64>"
    _check_vs_oracle(oracle_built, case, run, TIGHT, exact=True)


def test_precision1_vs_host_stepped(hip_lib, monkeypatch):
    """precision 1: the chain against the loop a caller steps on the same solver — host_estimator_step around its solves, the GPU's
    fp32 controls, the draws get_noise returns"""
    case = _ecase("cartpole17_plant")
    _env(monkeypatch, case)
    monkeypatch.delenv(SPLIT, raising=False)
    bs = _solver(case, precision=1)
    _install(bs, case)
    bs.set_x0(case["x0"])
    log = bs.mpc_rollout(STEPS)
    assert bs.last_launch_name == "stream4<4,1>" and bs.effective_precision == 1 and _launches(bs) == STEPS and bs.noise_cursor() == STEPS
    sol, left = bs.get_solution(), bs.get_estimator_state()
    nw, nv = _draws(bs, case, 0, STEPS)
    bs.close()
    hs = _solver(case, precision=1, own=False)
    prob = case["prob"]
    Ap, Bp = case["plant"]
    x, xh = np.array(_f32(case["x0"]), dtype=np.float64), np.array(case["xhat0"])
    u, xl, xhl, yl = np.zeros((1, STEPS, B)), np.zeros((4, STEPS, B)), np.zeros((4, STEPS, B)), np.zeros((2, STEPS, B))
    it, so = np.zeros((STEPS, B), dtype=int), np.zeros((STEPS, B), dtype=int)
    for k in range(STEPS):
        xh, yl[:, k, :] = t.host_estimator_step(xh, C=case["C"], L=case["L"], x=x, v=nv[:2, k, :], predict=False)
        xhl[:, k, :] = xh
        hs.set_x0(_f32(xh))
        hs.solve()
        s, st = hs.get_solution(), hs.get_status()
        u[:, k, :] = s["controls"][:, 0, :]
        x = ((np.einsum("ijb,jb->ib", Ap, x) + np.einsum("ijb,jb->ib", Bp, u[:, k, :])) + case["w"][:, k, :]) + nw[:, k, :]
        xl[:, k, :], it[k], so[k] = x, st["iter"], st["solved"]
        xh, _ = t.host_estimator_step(xh, A=prob.A, B=prob.B, u=u[:, k, :], correct=False)
    assert np.array_equal(it, log["iter"]) and np.array_equal(so, log["solved"])
    errs = [_rel(log[k], w).max() for k, w in (("u", u), ("x", xl), ("xhat", xhl), ("yout", yl))]
    print("precision 1: chain vs host-stepped loop, controls %.3e states %.3e estimates %.3e outputs %.3e" % tuple(errs))
    assert max(errs) <= FP32_TOL and nrel(left, xh) <= FP32_TOL
    assert max(nrel(sol["controls"][:, :, b], s["controls"][:, :, b]) for b in range(B)) <= FP32_TOL
    hs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (b) bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole20", "quadrotor10_sequence", "rocket12"])
def test_fused_schedule_is_the_split_one(hip_lib, monkeypatch, name):
    case = _ecase(name)
    _same(_run(monkeypatch, case, extra=(SPLIT,)), _run(monkeypatch, case), f"{name}: split vs fused")


@pytest.mark.parametrize("name", ["cartpole20", "cartpole17_plant"])
def test_two_rollouts_are_one(hip_lib, monkeypatch, name):
    case = _ecase(name)
    whole = _run(monkeypatch, case)
    _same(_run(monkeypatch, case, split=(3, 2)), whole, f"{name}: 3 + 2 vs 5")
    _same(_run(monkeypatch, case, split=(1,) * STEPS), whole, f"{name}: {STEPS} x 1 vs {STEPS}")
    _same(_run(monkeypatch, case, keep=False), whole, f"{name}: a second run")


def test_outputs_without_measurement_noise(hip_lib, oracle_built, monkeypatch):
    case = _ecase("cartpole20_quiet")
    run = _run(monkeypatch, case)
    assert run["nv"] is None
    loops = _check_vs_oracle(oracle_built, case, run, FP32_TOL, exact=False)
    want = _f32(np.stack([_of(case["C"], b) @ loops[b]["true"] for b in range(B)], axis=-1))
    assert _rel(run["log"]["yout"], want).max() <= FP32_TOL
    # C picks rows 0 and 2, so y is the true state's rows to the bit: the rounding the x log holds
    x_true = np.concatenate([_f32(case["x0"])[:, None, :], run["log"]["x"][:, :-1, :]], axis=1)
    assert np.array_equal(run["log"]["yout"], x_true[[0, 2]])


def test_dropping_returns_the_solver(hip_lib, monkeypatch):
    case = _ecase("cartpole20_model")
    plain = _without(case, "gw", "gv")
    _env(monkeypatch, plain)
    monkeypatch.delenv(SPLIT, raising=False)
    fresh = _solver(plain)
    fresh.set_x0(case["x0"])
    want = _collect(fresh, fresh.mpc_rollout(STEPS))
    assert _launches(fresh) == 1 and fresh.estimator_mode() == 0
    name = fresh.last_launch_name
    fresh.close()
    noisy = _solver(case)
    _install_noise(noisy, case)
    noisy.set_x0(case["x0"])
    want_noisy = _collect(noisy, noisy.mpc_rollout(STEPS))
    noisy.close()
    bs = _solver(case)
    _install(bs, case)
    bs.set_precision(1)                            # (a change of precision keeps the estimator)
    assert bs.estimator_mode() == 1
    bs.set_precision(0)
    bs.set_x0(case["x0"])
    assert "xhat" in bs.mpc_rollout(STEPS) and _launches(bs) == STEPS
    with pytest.raises(t.TinyMPCError, match="get_mpc_estimate"):
        bs._chk(bs.lib.tinympc_get_mpc_measured(bs.h, np.zeros(4 * STEPS * B).ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "get_mpc_measured")
    bs.set_estimator(None)
    assert bs.estimator_mode() == 0 and bs.noise_mode() == 9
    # the measurement-noise chain again, with its y log
    bs.reset()
    bs.set_noise_cursor(0)
    bs.set_x0(case["x0"])
    got = _collect(bs, bs.mpc_rollout(STEPS))
    assert _launches(bs) == STEPS and "xhat" not in got["log"]
    _identical(got, want_noisy, "the noise chain after dropping the estimator")
    assert np.array_equal(got["log"]["y"], want_noisy["log"]["y"])
    # ... and without the noise the cartpole's fused loop, one launch
    bs.set_process_noise(None)
    bs.set_measurement_noise(None)
    bs.reset()
    bs.set_x0(case["x0"])
    got = _collect(bs, bs.mpc_rollout(STEPS))
    assert _launches(bs) == 1 and bs.last_launch_name == name and "xhat" not in got["log"] and "y" not in got["log"]
    _identical(got, want, "after dropping everything")
    with pytest.raises(t.TinyMPCError, match="no estimator is installed"):
        bs.get_estimator_state()
    bs.close()


def test_metrics_change_nothing_and_keep_the_true_state(hip_lib, monkeypatch):
    case = _ecase("cartpole20")
    plain, scored = _run(monkeypatch, case), _run(monkeypatch, case, metrics=True)
    _same(scored, plain, "metrics enabled")
    log = scored["log"]
    signed = np.where(log["solved"] > 0, log["iter"], -log["iter"])
    qw, rw = np.diag(case["prob"].Q), np.diag(case["prob"].R)
    want = np.stack([restated(log["x"][:, :, b].T, log["u"][:, :, b].T, signed[:, b], qw, rw) for b in range(B)])
    check_slots(scored["metrics"], want, "metrics of the estimator chain")


@pytest.mark.parametrize("extra", [("TINYMPC_HIP_LEAN_WS",), ("TINYMPC_HIP_STREAM_MPC",), ("TINYMPC_HIP_LEAN_WS", "TINYMPC_HIP_LEAN_LOOP"),
                                   ("TINYMPC_HIP_STREAM_MPC", "TINYMPC_HIP_STREAM_LOOP")],
                         ids=lambda e: "+".join(n[len("TINYMPC_HIP_"):] for n in e))
@pytest.mark.parametrize("name", ["cartpole20", "cartpole17_plant"])
def test_switches_keep_the_chain(hip_lib, monkeypatch, name, extra):
    case = _ecase(name)
    chain = _run(monkeypatch, case)
    switched = _run(monkeypatch, case, extra=extra)      # (`steps` launches: asserted in _run)
    _same(switched, chain, "+".join(extra))


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the state between rollouts
# ---------------------------------------------------------------------------------------------------------------------------
def test_estimate_and_plant_move_apart(hip_lib, monkeypatch):
    case = _ecase("cartpole20_model")
    whole = _run(monkeypatch, case)
    _env(monkeypatch, case)
    bs = _solver(case)
    _install(bs, case, state=False)
    bs.set_x0(case["x0"])
    # not yet live: the next rollout takes xhat-_0 = x0 as the device holds it
    assert np.array_equal(bs.get_estimator_state(), _f32(case["x0"]))
    first = bs.mpc_rollout(3)
    assert not np.array_equal(first["xhat"], whole["log"]["xhat"][:, :3])      # (another initial estimate, another loop)
    est = bs.get_estimator_state()
    assert np.isfinite(est).all() and not np.array_equal(est, _f32(case["x0"]))
    assert np.array_equal(_collect(bs, first)["x0"], first["x"][:, -1, :].T.astype(np.float32)), "x0 after a rollout is not the last true state's rounding"
    # set_x0 moves the plant, not the estimate
    moved = np.asfortranarray(0.5 * case["x0"])
    bs.set_x0(moved)
    assert np.array_equal(bs.get_estimator_state(), est)
    nxt = bs.mpc_rollout(1)
    y_want = _f32(_selector(4, (0, 2)) @ _f32(moved) + bs.get_noise(1, 3, 1)[:2, 0, :])
    assert np.array_equal(nxt["yout"][:, 0, :], y_want), "the measurement is not taken of the plant set_x0 installed"
    # set_estimator_state(None) re-arms: the estimate is x0 again (here the true state's rounding the rollout left)
    bs.set_estimator_state(None)
    assert np.array_equal(bs.get_estimator_state(), nxt["x"][:, -1, :])
    # installing a state and running from the start is the whole run
    bs.reset()
    bs.set_noise_cursor(0)
    bs.set_estimator_state(case["xhat0"])
    bs.set_x0(case["x0"])
    again = bs.mpc_rollout(STEPS)
    for key in ("x", "u", "xhat", "yout", "iter", "solved"):
        assert np.array_equal(again[key], whole["log"][key]), key
    assert np.array_equal(bs.get_estimator_state(), whole["est"])
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (d) refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["adaptive", "cold"])
def test_rollout_refusals(hip_lib, monkeypatch, what):
    case = _ecase("cartpole20_model")
    _env(monkeypatch, case)
    bs = _solver(case)
    _install(bs, case)
    bs.set_x0(case["x0"])
    if what == "adaptive":
        bs.set_adaptive_rho(True)
        want = "a state estimator is not available with adaptive rho"
    else:
        bs.set_warm_start(False)
        want = "needs the persistent workspace"
    with pytest.raises(t.TinyMPCError, match=want):
        bs.mpc_rollout(STEPS)
    assert _launches(bs) == -1 and bs.noise_cursor() == 0 and bs.estimator_mode() == 1
    assert np.array_equal(bs.get_estimator_state(), case["xhat0"])
    if what == "adaptive":
        bs.set_adaptive_rho(False)
    assert bs.solve() in (0, 1) and np.isfinite(bs.get_solution()["controls"]).all()
    bs.close()


def test_setter_refusals(hip_lib, monkeypatch):
    case = _ecase("cartpole20_model")
    _env(monkeypatch, case)
    bs = _solver(case)
    bs.set_x0(case["x0"])
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))      # noqa: E731
    C, L = np.ascontiguousarray(np.zeros(20)), np.ascontiguousarray(np.zeros(20))
    for ny in (0, 5, -1):
        assert bs.lib.tinympc_set_estimator(bs.h, dp(C), ny, dp(L), 0) == -1 and b"1 <= ny <= nx" in bs.lib.tinympc_last_error()
    assert bs.lib.tinympc_set_estimator(bs.h, dp(C), 2, None, 0) == -1 and b"expected both" in bs.lib.tinympc_last_error()
    assert bs.lib.tinympc_set_estimator(bs.h, None, 2, dp(L), 0) == -1 and b"expected both" in bs.lib.tinympc_last_error()
    assert bs.lib.tinympc_set_estimator(bs.h, dp(C), 2, dp(L), 2) == -1 and b"per_instance is 0" in bs.lib.tinympc_last_error()
    with pytest.raises(t.TinyMPCError, match="expected both"):
        bs.set_estimator(case["C"], None)
    for bad in ((np.zeros((2, 4)), np.zeros((4, 3))), (np.zeros((2, 3)), np.zeros((3, 2))), (np.zeros((2, 4, B - 1)), np.zeros((4, 2, B - 1))), (np.zeros(4), np.zeros(4))):
        with pytest.raises(t.TinyMPCError, match="expected C"):
            bs.set_estimator(*bad)
    with pytest.raises(t.TinyMPCError, match="no estimator is installed"):
        bs.set_estimator_state(case["xhat0"])
    with pytest.raises(t.TinyMPCError, match="no estimator is installed"):
        bs.get_estimator_state()
    assert bs.estimator_mode() == 0
    bs.set_estimator(case["C"], case["L"])
    with pytest.raises(t.TinyMPCError, match="expected xhat"):
        bs.set_estimator_state(np.zeros((4, B + 1)))
    bs.set_estimator_state(case["xhat0"][:, 0])      # (a vector: shared by the batch)
    assert np.array_equal(bs.get_estimator_state(), np.repeat(case["xhat0"][:, :1], B, axis=1))
    for fn in (bs.lib.tinympc_get_mpc_estimate, bs.lib.tinympc_get_mpc_outputs):
        assert fn(bs.h, dp(np.zeros(4 * STEPS * B))) == -1 and b"no mpc_rollout with an estimator has run" in bs.lib.tinympc_last_error()
    assert bs.solve() in (0, 1) and np.isfinite(bs.get_solution()["controls"]).all()
    bs.close()


def test_global_forms(hip_lib, monkeypatch):
    """the process-global solver: the setters, mpc_rollout's xhat and yout, the library's own shape checks, and the refusal under
    set_gpus (one device, listed twice)"""
    case = _ecase("cartpole20_model")
    _env(monkeypatch, case)
    monkeypatch.delenv(SPLIT, raising=False)
    monkeypatch.delenv("TINYMPC_HIP_SHARD_DEVICES", raising=False)
    prob = case["prob"]
    s = t.TinyMPCSolver()
    try:
        t.setup(s, prob.A, prob.B, None, prob.Q, prob.R, prob.rho, 4, 1, prob.N, batch=B, **case["kw"])
        t.set_bound_constraints(s, prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        assert t.estimator_mode(s) == 0
        t.set_process_noise(s, case["gw"], SEED_W)
        t.set_measurement_noise(s, case["gv"], SEED_V)
        with pytest.raises(t.TinyMPCError, match="expected C"):
            t.set_estimator(s, np.zeros((2, 3)), np.zeros((3, 2)))
        t.set_estimator(s, case["C"], case["L"])
        assert t.estimator_mode(s) == 1
        with pytest.raises(t.TinyMPCError, match="expected xhat"):
            t.set_estimator_state(s, np.zeros((3, B)))
        t.set_estimator_state(s, case["xhat0"])
        assert np.array_equal(t.get_estimator_state(s), case["xhat0"])
        t.set_x0(s, case["x0"])
        log = t.mpc_rollout(s, STEPS)
        ref = _run(monkeypatch, case)
        assert "y" not in log
        for key in ("x", "u", "xhat", "yout", "iter", "solved"):
            assert np.array_equal(log[key], ref["log"][key]), key
        assert np.array_equal(t.get_estimator_state(s), ref["est"])
        t.set_estimator(s, None)
        assert t.estimator_mode(s) == 0 and "y" in t.mpc_rollout(s, STEPS)
        t.set_estimator(s, case["C"], case["L"])
        t.set_batch_size(s, B + 3)                                # re-batching drops the estimator as it drops the noise
        assert t.estimator_mode(s) == 0 and t.noise_mode(s) == 0
        t.set_batch_size(s, B)
        monkeypatch.setenv("TINYMPC_HIP_SHARD_DEVICES", "0,0")
        t.set_gpus(s, 2)
        for call, word in ((lambda: t.set_estimator(s, case["C"], case["L"]), "set_estimator"), (lambda: t.set_estimator_state(s, None), "set_estimator_state"),
                           (lambda: t.estimator_mode(s), "estimator_mode"), (lambda: t.get_estimator_state(s), "get_estimator_state")):
            with pytest.raises(t.TinyMPCError, match=word + ": not available on a sharded solver"):
                call()
        t.set_x0(s, case["x0"])
        assert t.solve(s) in (0, 1)
    finally:
        t.cleanup()
