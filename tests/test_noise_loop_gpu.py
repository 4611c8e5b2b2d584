"""mpc_rollout under seeded process and measurement noise drawn on the device (BatchSolver.set_process_noise /
set_measurement_noise; csrc/noise.h, csrc/solver.hip: noise_fill_kernel, measure_kernel, plant_step_kernel<true>).

The rule, with the noise cursor c and loop step s, t = c + s: the solve of step s starts from float32(x_t + G_v xi_v[b][t]), x_t
the fp64 plant state; the plant step is x+ = ((f_p + A_p x + B_p u0) + w) + G_w xi_w[b][t]; the x log, x0d and x0 hold the true
state; the cursor is left c + steps.  The reference is orc64 stepped by that rule in numpy fp64 and fed the DEVICE's own draws
(get_noise), compared as tests/test_plant_loop_gpu.py compares: every instance at FP32_TOL, an instance whose (iteration count,
solved flag) differs at a step replayed with the GPU's decision imposed.  The generator itself is held to tinympc_host_noise at
1e-12 max(1, ||G||_inf) (tests/test_noise.py holds that to a numpy restatement of the rule).

Noise scale: G = diag(0.003 scale_r), scale_r the largest |x0| of row r over the batch (per instance: times a factor in
[0.5, 1.5]), so most draws stay within the +-1 % of tests/test_plant_loop_gpu.py's disturbance.  The oracle's states are asserted
finite and bounded (row by row at most twice the excursion of the undisturbed model-plant loops) first.

 (a) get_noise of both kinds against host_noise: nx = 4 and 12, shared and per-instance G, t0 = 0 and 7
 (b) process noise alone is set_disturbance(get_noise(0, 0, 5)), bit for bit
 (c) against orc64: every kernel family, precision 2 at 1e-6, precision 1 against the host-stepped loop, a reference trajectory
 (d) the y log: float32(x_true + v); bit-equal to what a host-stepped run uploads; the x log is the true state
 (e) the cursor: 3 + 2 = 5 bit for bit, set_noise_cursor, another seed
 (f) no change without noise: dropping, an all-zero G, the closed-loop switches
 (g) refusals, by a word of their message, each followed by a plain solve

Batch 70 (one full stream workgroup and a ragged wavefront), 5 steps.  Every test fails without the feature: the setters do not
exist there."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.test_plant_loop_gpu import B, STEPS, SWITCHES, TIGHT, _case, _env, _model, _plant_of, _solver, _stack, _w_of
from tests.test_stream_loop_gpu import _collect, _configure, _f32, _identical, _launches, _rel
from tests.util import FP32_TOL, nrel

pytestmark = pytest.mark.gpu

GEN_TOL = 1e-12
SEED_W, SEED_V = 0x1234_5678_9ABC_DEF1, 77


# ---------------------------------------------------------------------------------------------------------------------------
# the cases: one of tests/test_plant_loop_gpu.py's (plant, disturbance, references, kernel) plus the noise factors
# ---------------------------------------------------------------------------------------------------------------------------
def _diag(x0, per_instance=False, seed=0):
    sig = 0.003 * np.abs(x0).max(axis=1)
    assert (sig > 0.0).all()
    if not per_instance:
        return np.diag(sig)
    f = np.random.default_rng(900 + seed).uniform(0.5, 1.5, B)
    return np.asfortranarray(np.diag(sig)[:, :, None] * f[None, None, :])


def _trajectory_case():
    """cartpole N = 20 along a per-instance reference trajectory (the cart position on a sinusoid of per-instance amplitude and
    phase), the model as the plant"""
    base = _case("cartpole20")
    prob = base["prob"]
    rng = np.random.default_rng(41)
    L = STEPS + prob.N + 2
    amp, phase = rng.uniform(0.05, 0.3, B), rng.uniform(0.0, 2.0 * np.pi, B)
    wave = np.sin(0.15 * np.arange(L)[:, None] + phase[None, :])
    xt, ut = np.zeros((prob.nx, L, B), order="F"), np.zeros((prob.nu, L - 1, B), order="F")
    xt[0] = amp[None, :] * wave
    ut[0] = 0.05 * amp[None, :] * wave[:L - 1]
    return dict(prob=prob, x0=base["x0"], kw=base["kw"], xt=xt, ut=ut)


def _without(case, *keys):
    return {k: v for k, v in case.items() if k not in keys}


def _build(name):
    if name == "cartpole20":                      # per-instance plant, an uploaded disturbance, both noises (per-instance G_v)
        c = dict(_case("cartpole20"))
        return dict(c, gw=_diag(c["x0"]), gv=_diag(c["x0"], True, 1))
    if name == "quadrotor10_sequence":            # fixed 10 iterations, shared G, a reference sequence
        c = dict(_case("quadrotor10_sequence"))
        return dict(c, gw=_diag(c["x0"]), gv=_diag(c["x0"]))
    if name == "rocket12":                        # stream4<6,3>: cones, affine term, references
        c = dict(_case("rocket12"))
        return dict(c, gw=_diag(c["x0"], True, 2), gv=_diag(c["x0"]))
    if name == "cartpole17_generic":
        c = dict(_case("cartpole17_generic"))
        return dict(c, gw=_diag(c["x0"]), gv=_diag(c["x0"]))
    if name == "quadrotor10_p2":
        c = dict(_case("quadrotor10_p2"))
        return dict(c, gw=_diag(c["x0"]), gv=_diag(c["x0"]))
    if name == "cartpole17_plant":
        c = dict(_case("cartpole17_plant"))
        return dict(c, gw=_diag(c["x0"]), gv=_diag(c["x0"], True, 3))
    if name == "cartpole20_trajectory":
        c = _trajectory_case()
        return dict(c, gw=_diag(c["x0"]), gv=_diag(c["x0"]))
    if name == "cartpole20_model":                # the model as the plant, process noise alone
        c = _without(_case("cartpole20"), "plant", "w")
        return dict(c, gw=_diag(c["x0"], True, 4))
    if name == "cartpole20_own":                  # the per-instance plant, process noise alone
        c = _without(_case("cartpole20"), "w")
        return dict(c, gw=_diag(c["x0"]))
    if name == "quadrotor10_process":             # shared plant with f_p, reference sequence, fixed iterations, process noise alone
        c = _without(_case("quadrotor10_sequence"), "w")
        return dict(c, gw=_diag(c["x0"]))
    raise KeyError(name)


_CASES = {}


def _ncase(name):
    if name not in _CASES:
        _CASES[name] = dict(_build(name), id="noise_" + name)
    return _CASES[name]


def _install_noise(bs, case, seed_w=SEED_W, seed_v=SEED_V):
    if "xt" in case:
        bs.set_ref_trajectory(case["xt"], case["ut"])
    if "gw" in case:
        bs.set_process_noise(case["gw"], seed_w)
    if "gv" in case:
        bs.set_measurement_noise(case["gv"], seed_v)


def _mode(case):
    m = 0
    if "gw" in case:
        m |= 2 if case["gw"].ndim == 3 else 1
    if "gv" in case:
        m |= 8 if case["gv"].ndim == 3 else 4
    return m


def _draws(bs, case, t0, steps):
    """the device's own realised noise of the steps t0 .. t0 + steps - 1: (process | None, measurement | None)"""
    return (bs.get_noise(0, t0, steps) if "gw" in case else None, bs.get_noise(1, t0, steps) if "gv" in case else None)


_RUNS = {}


def _run(monkeypatch, case, steps=STEPS, extra=(), cursor=0, seeds=(SEED_W, SEED_V), split=None, keep=True):
    key = (case["id"], steps, tuple(extra), cursor, seeds, split)
    if keep and key in _RUNS:
        return _RUNS[key]
    _env(monkeypatch, case)
    for name in extra:
        monkeypatch.setenv(name, "1")
    bs = _solver(case)
    _install_noise(bs, case, *seeds)
    assert bs.noise_mode() == _mode(case) and bs.noise_cursor() == 0
    if cursor:
        bs.set_noise_cursor(cursor)
    bs.set_x0(case["x0"])
    logs, done = [], 0
    for n in (split or (steps,)):
        if done and "w" in case:      # (the uploaded disturbance is read from row 0 whatever the cursor: its rows of this part)
            bs.set_disturbance(np.asfortranarray(case["w"][:, done:done + n]))
        logs.append(bs.mpc_rollout(n))
        done += n
        assert _launches(bs) == n, (_launches(bs), n)
        assert ("y" in logs[-1]) == ("gv" in case)
    log = {k: np.concatenate([l[k] for l in logs], axis=0 if k in ("iter", "solved") else 1) for k in logs[0] if k != "status"}
    log["status"] = logs[-1]["status"]
    out = _collect(bs, log)
    out["cursor"], out["launched"] = bs.noise_cursor(), bs.last_launch_name
    out["nw"], out["nv"] = _draws(bs, case, cursor, steps)
    if "xt" in case:
        out["ref_cursor"] = bs.ref_cursor()
    bs.close()
    if keep:
        _RUNS[key] = out
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's loops, stepped by the rule with the device's draws
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle_loop(oracle, case, b, steps, nw, nv, forced=None):
    prob = case["prob"]
    o = _configure(oracle.CpuSolver("orc64", *_model(case, b), prob.N), case)
    Ap, Bp, fp = _plant_of(case, b)
    x = np.array(_f32(case["x0"][:, b]), dtype=np.float64)      # (the loop's fp64 state starts from the fp32 x0 the solver holds)
    u_log, x_log, y_log = np.zeros((prob.nu, steps)), np.zeros((prob.nx, steps)), np.zeros((prob.nx, steps))
    it, so = np.zeros(steps, dtype=int), np.zeros(steps, dtype=int)
    r = None
    for k in range(steps):
        if forced is not None:
            o.set_forced_exit(int(forced[k][0]) if forced[k][1] else -1)
        y = _f32(x if nv is None else x + nv[:, k, b])
        o.set_x0(y)
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
        u_log[:, k], x_log[:, k], y_log[:, k], it[k], so[k] = u0, x, y, r["iter"], r["solved"]
    ws = o.get_state()
    o.close()
    return dict(u=u_log, x=x_log, y=y_log, iter=it, solved=so, last_x=np.array(r["x"]), last_u=np.array(r["u"]), ws=ws)


_ORACLE = {}


def _oracle_loops(oracle, case, run):
    key = case["id"]
    if key not in _ORACLE:
        loops = [_oracle_loop(oracle, case, b, STEPS, run["nw"], run["nv"]) for b in range(B)]
        x = _stack(loops, "x")
        nominal = _without(case, "plant", "w")
        xn = np.stack([_oracle_loop(oracle, nominal, b, STEPS, None, None)["x"] for b in range(B)], axis=-1)
        bound = 2.0 * np.maximum(np.abs(xn).max(axis=(1, 2)), np.abs(case["x0"]).max(axis=1))
        assert np.isfinite(x).all() and (np.abs(x).max(axis=(1, 2)) <= bound).all(), (key, np.abs(x).max(axis=(1, 2)) / bound)
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
    eu, ex = _rel(log["u"], _stack(loops, "u")), _rel(log["x"], _stack(loops, "x"))
    print(f"{tag}: worst applied control {eu.max():.3e}, worst plant state {ex.max():.3e}")
    assert eu.max() <= tol, f"{tag}: applied controls, worst {eu.max():.3e} (instance {eu.argmax()})"
    assert ex.max() <= tol, f"{tag}: plant states, worst {ex.max():.3e} (instance {ex.argmax()})"
    if "gv" in case:
        ey = _rel(log["y"], _stack(loops, "y"))
        print(f"{tag}: worst measured state {ey.max():.3e}")
        assert ey.max() <= tol, f"{tag}: measured states, worst {ey.max():.3e} (instance {ey.argmax()})"
    wx = max(nrel(run["sol"]["states"][:, :, b], loops[b]["last_x"]) for b in range(B))
    wu = max(nrel(run["sol"]["controls"][:, :, b], loops[b]["last_u"]) for b in range(B))
    print(f"{tag}: last solve, worst states {wx:.3e}, worst controls {wu:.3e}")
    assert wx <= tol and wu <= tol, f"{tag}: last solve, states {wx:.3e} controls {wu:.3e}"
    assert np.array_equal(run["st"]["iter"], log["iter"][-1]) and np.array_equal(run["st"]["solved"], log["solved"][-1])
    assert np.array_equal(run["x0"], log["x"][:, -1, :].T.astype(np.float32)), f"{tag}: x0 is not the last TRUE plant state"
    return loops


def _noise_acts(case, run):
    """the draws are there and of the intended size: non-zero, distinct per instance, most within 1 % of the row's scale"""
    scale = np.abs(case["x0"]).max(axis=1)[:, None, None]
    for n in (run["nw"], run["nv"]):
        if n is not None:
            assert np.isfinite(n).all() and (n != 0.0).all() and len(np.unique(n[0])) == n[0].size
            assert np.mean(np.abs(n) <= 0.01 * scale) > 0.9 and np.abs(n).max() <= 0.05 * scale.max()


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the generator on the device
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_instance", [False, True], ids=["shared", "per_instance"])
@pytest.mark.parametrize("work", ["cartpole", "quadrotor"])
def test_get_noise_is_host_noise(hip_lib, monkeypatch, work, per_instance):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    prob = t.problems.cartpole(20, u_bound=0.5) if work == "cartpole" else t.problems.quadrotor(10)
    nx = prob.nx
    rng = np.random.default_rng(5 + nx)
    G = [np.asfortranarray(rng.standard_normal((nx, nx, B) if per_instance else (nx, nx))) for _ in range(2)]
    seeds = (0xFEDC_BA98_7654_3210, 3)
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    with pytest.raises(t.TinyMPCError, match="has to be installed"):
        bs.get_noise(0, 0, 3)
    bs.set_process_noise(G[0], seeds[0])
    bs.set_measurement_noise(G[1], seeds[1])
    assert bs.noise_mode() == (10 if per_instance else 5) and bs.noise_cursor() == 0 and bs.plant_mode() == 0
    worst = 0.0
    for which in (0, 1):
        for t0 in (0, 7):
            got = bs.get_noise(which, t0, 3)
            assert got.shape == (nx, 3, B)
            for b in range(B):
                Gb = G[which][:, :, b] if per_instance else G[which]
                tol = GEN_TOL * max(1.0, np.abs(Gb).sum(axis=1).max())
                for s in range(3):
                    err = np.abs(got[:, s, b] - t.host_noise(seeds[which], which, b, t0 + s, nx, Gb)).max()
                    worst = max(worst, err / tol * GEN_TOL)
                    assert err <= tol, (which, t0, b, s, err)
    print(f"{work} {'per-instance' if per_instance else 'shared'} G: device vs host draws, worst |delta| / max(1, ||G||_inf) = {worst:.3e}")
    # steps overlap: t0 = 7's first row is what t0 = 5 calls its third
    assert np.array_equal(bs.get_noise(0, 7, 1)[:, 0, :], bs.get_noise(0, 5, 3)[:, 2, :])
    assert bs.noise_cursor() == 0
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (b) process noise alone is an uploaded disturbance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole20_model", "cartpole20_own", "quadrotor10_process"])
def test_process_noise_is_the_uploaded_disturbance(hip_lib, monkeypatch, name):
    case = _ncase(name)
    mine = _run(monkeypatch, case)
    assert mine["cursor"] == STEPS
    _noise_acts(case, mine)
    _env(monkeypatch, case)
    bs = _solver(dict(_without(case, "gw"), w=np.asfortranarray(mine["nw"])))
    assert bs.noise_mode() == 0 and bs.plant_mode() & 8
    bs.set_x0(case["x0"])
    uploaded = _collect(bs, bs.mpc_rollout(STEPS))
    assert _launches(bs) == STEPS and bs.last_launch_name == mine["launched"] and bs.noise_cursor() == 0
    bs.close()
    _identical(mine, uploaded, name)
    if case["kw"]["abs_pri_tol"] == 0.0:
        assert np.all(mine["log"]["iter"] == case["kw"]["max_iter"])


# ---------------------------------------------------------------------------------------------------------------------------
# (c) against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole20", "quadrotor10_sequence", "rocket12", "cartpole17_generic", "cartpole20_trajectory"])
def test_noisy_chain_vs_oracle(hip_lib, oracle_built, monkeypatch, name):
    case = _ncase(name)
    run = _run(monkeypatch, case)
    if "name" in case:
        assert run["launched"] == case["name"], run["launched"]
    assert run["cursor"] == STEPS
    _noise_acts(case, run)
    fixed = case["kw"]["abs_pri_tol"] == 0.0
    _check_vs_oracle(oracle_built, case, run, FP32_TOL, exact=fixed)
    if fixed:
        assert np.all(run["log"]["iter"] == case["kw"]["max_iter"]) and not run["log"]["solved"].any()
    if "xt" in case:        # both cursors advance
        assert run["ref_cursor"] == STEPS


def test_precision2(hip_lib, oracle_built, monkeypatch):
    case = _ncase("quadrotor10_p2")
    run = _run(monkeypatch, case)
    assert run["launched"] == "generic<f64>"
    loops = _check_vs_oracle(oracle_built, case, run, TIGHT, exact=True)
    for key in ("d", "y", "g", "v", "z"):
        e = max(np.abs(run["ws"][key][:, :, b] - loops[b]["ws"][key]).max() / max(np.abs(loops[b]["ws"][key]).max(), 1e-2) for b in range(B))
        assert e <= TIGHT, f"workspace {key} {e:.3e}"


def test_precision1_vs_host_stepped(hip_lib, monkeypatch):
    """precision 1: the chain against the loop a caller steps on the same solver, the same rule with the GPU's fp32 controls and the
    draws get_noise returns"""
    case = _ncase("cartpole17_plant")
    _env(monkeypatch, case)
    bs = _solver(case, precision=1)
    _install_noise(bs, case)
    bs.set_x0(case["x0"])
    log = bs.mpc_rollout(STEPS)
    assert bs.last_launch_name == "stream4<4,1>" and bs.effective_precision == 1 and _launches(bs) == STEPS and bs.noise_cursor() == STEPS
    sol = bs.get_solution()
    nw, nv = _draws(bs, case, 0, STEPS)
    bs.close()
    hs = _solver(case, precision=1, own=False)
    Ap, Bp = case["plant"]
    x = np.array(case["x0"], dtype=np.float64)
    u, xl, yl = np.zeros((1, STEPS, B)), np.zeros((4, STEPS, B)), np.zeros((4, STEPS, B))
    it, so = np.zeros((STEPS, B), dtype=int), np.zeros((STEPS, B), dtype=int)
    for k in range(STEPS):
        yl[:, k, :] = _f32(x + nv[:, k, :])
        hs.set_x0(yl[:, k, :])
        hs.solve()
        s, st = hs.get_solution(), hs.get_status()
        u[:, k, :] = s["controls"][:, 0, :]
        x = ((np.einsum("ijb,jb->ib", Ap, x) + np.einsum("ijb,jb->ib", Bp, u[:, k, :])) + case["w"][:, k, :]) + nw[:, k, :]
        xl[:, k, :], it[k], so[k] = x, st["iter"], st["solved"]
    assert np.array_equal(it, log["iter"]) and np.array_equal(so, log["solved"])
    assert 0 < so.sum() < so.size, "one kind of exit only"
    eu, ex, ey = _rel(log["u"], u), _rel(log["x"], xl), _rel(log["y"], yl)
    print(f"precision 1: chain vs host-stepped loop, controls {eu.max():.3e} states {ex.max():.3e} measured {ey.max():.3e}")
    assert eu.max() <= FP32_TOL and ex.max() <= FP32_TOL and ey.max() <= FP32_TOL
    assert max(nrel(sol["controls"][:, :, b], s["controls"][:, :, b]) for b in range(B)) <= FP32_TOL
    assert max(nrel(sol["states"][:, :, b], s["states"][:, :, b]) for b in range(B)) <= FP32_TOL
    hs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (d) measurement noise
# ---------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))      # (one rounding, to nearest even: an fp64 fma)


def _device_step(Ap, Bp, fp, x, u0, w, n):
    """the plant-step kernel's arithmetic, to the bit: row r is f_p[r], then A_p's row and B_p's by ascending column, one fma each,
    then + w, then + n"""
    out = np.zeros_like(x)
    for r in range(x.size):
        acc = float(fp[r])
        for j in range(x.size):
            acc = _fma(Ap[r, j], x[j], acc)
        for a in range(u0.size):
            acc = _fma(Bp[r, a], u0[a], acc)
        out[r] = (acc + w[r]) + n[r]
    return out


def test_measured_states(hip_lib, oracle_built, monkeypatch):
    case = _ncase("cartpole20")
    run = _run(monkeypatch, case)
    log, nw, nv = run["log"], run["nw"], run["nv"]
    loops = _oracle_loops(oracle_built, case, run)
    # float32(x_true + v), recomputed from the oracle's run
    want = np.stack([_f32(np.concatenate([_f32(case["x0"][:, b:b + 1]), loops[b]["x"][:, :-1]], axis=1) + nv[:, :, b]) for b in range(B)], axis=-1)
    ey = _rel(log["y"], want)
    print(f"measured states against float32(oracle's true state + v): worst {ey.max():.3e}")
    assert ey.max() <= FP32_TOL
    # the loop a caller steps itself: the same launches from the same uploads, the plant step in the kernel's own arithmetic
    _env(monkeypatch, case)
    hs = _solver(case, own=False)
    x = np.array(_f32(case["x0"]), dtype=np.float64)
    for k in range(STEPS):
        y = _f32(x + nv[:, k, :])
        assert np.array_equal(y, log["y"][:, k, :]), f"step {k}: the measured state is not what a host-stepped run uploads"
        hs.set_x0(y)
        hs.solve()
        u0 = hs.get_solution()["controls"][:, 0, :]
        assert np.array_equal(u0, log["u"][:, k, :]), f"step {k}: applied controls"
        for b in range(B):
            x[:, b] = _device_step(*_plant_of(case, b), x[:, b], u0[:, b], _w_of(case, b, k), nw[:, k, b])
        assert np.array_equal(_f32(x), log["x"][:, k, :]), f"step {k}: the x log is not the true state"
    assert hs.last_launch_name == run["launched"]
    hs.close()
    # the x log is the true state, never the measurement: they differ wherever G_v != 0 (here: every row)
    assert (np.diagonal(case["gv"]) != 0.0).all()
    assert np.all(log["y"][:, 1:, :] != log["x"][:, :-1, :]) and np.all(log["y"][:, 0, :] != _f32(case["x0"]))
    assert np.array_equal(run["x0"], _f32(x).T.astype(np.float32)), "x0 after the loop is not the rounding of the last true state"


# ---------------------------------------------------------------------------------------------------------------------------
# (e) the cursor
# ---------------------------------------------------------------------------------------------------------------------------
def _same(a, c, tag):
    _identical(a, c, tag)
    if "y" in a["log"]:
        assert np.array_equal(a["log"]["y"], c["log"]["y"]), f"{tag}: log y"


@pytest.mark.parametrize("name", ["cartpole20", "cartpole17_plant"])
def test_two_rollouts_are_one(hip_lib, monkeypatch, name):
    case = _ncase(name)
    whole = _run(monkeypatch, case)
    halves = _run(monkeypatch, case, split=(3, 2))
    assert whole["cursor"] == STEPS and halves["cursor"] == STEPS
    _same(halves, whole, f"{name} 3 + 2 vs 5")


def test_set_noise_cursor_and_seed(hip_lib, monkeypatch):
    case = _ncase("cartpole20")
    whole = _run(monkeypatch, case)
    _env(monkeypatch, case)
    bs = _solver(case)
    _install_noise(bs, case)
    bs.set_x0(case["x0"])
    bs.mpc_rollout(3)                              # (step 3's state: workspace, fp64 plant state, x0)
    assert bs.noise_cursor() == 3
    bs.set_noise_cursor(40)
    assert bs.noise_cursor() == 40
    bs.set_process_noise(case["gw"], SEED_W)       # (a newly installed noise leaves the cursor alone)
    assert bs.noise_cursor() == 40
    bs.set_noise_cursor(3)
    bs.set_disturbance(np.asfortranarray(case["w"][:, 3:5]))      # (the disturbance is read from row 0 whatever the cursor)
    tail = bs.mpc_rollout(2)
    assert bs.noise_cursor() == 5
    for key in ("x", "u", "y"):
        assert np.array_equal(tail[key], whole["log"][key][:, 3:5]), key
    assert np.array_equal(tail["iter"], whole["log"]["iter"][3:5]) and np.array_equal(tail["solved"], whole["log"]["solved"][3:5])
    assert np.array_equal(bs.get_noise(1, 3, 2), whole["nv"][:, 3:5])
    bs.close()
    # another cursor, another seed: other draws, other logs
    moved = _run(monkeypatch, case, cursor=STEPS)
    assert moved["cursor"] == 2 * STEPS
    other = _run(monkeypatch, case, seeds=(SEED_W + 1, SEED_V))
    third = _run(monkeypatch, case, seeds=(SEED_W, SEED_V + 1))
    for r in (moved, other, third):
        assert not np.array_equal(r["log"]["x"], whole["log"]["x"]) and not np.array_equal(r["log"]["u"][:, 1:], whole["log"]["u"][:, 1:])
    assert np.array_equal(other["nv"], whole["nv"]) and not np.any(other["nw"] == whole["nw"])
    assert np.array_equal(third["nw"], whole["nw"]) and not np.any(third["nv"] == whole["nv"])
    assert not np.any(moved["nw"] == whole["nw"])


# ---------------------------------------------------------------------------------------------------------------------------
# (f) no change without noise
# ---------------------------------------------------------------------------------------------------------------------------
def test_dropping_returns_the_solver(hip_lib, monkeypatch):
    case = _without(_ncase("cartpole20"), "plant", "w")
    _env(monkeypatch, case)
    fresh = _solver(case)
    fresh.set_x0(case["x0"])
    want = _collect(fresh, fresh.mpc_rollout(STEPS))
    assert _launches(fresh) == 1 and "y" not in want["log"]
    name = fresh.last_launch_name
    fresh.close()
    bs = _solver(case)
    _install_noise(bs, case)
    bs.set_precision(1)                            # (a change of precision keeps the noise)
    assert bs.noise_mode() == 9
    bs.set_precision(0)
    bs.set_x0(case["x0"])
    assert "y" in bs.mpc_rollout(STEPS) and _launches(bs) == STEPS
    bs.set_process_noise(None)
    assert bs.noise_mode() == 8 and bs.plant_mode() == 0
    bs.set_measurement_noise(None)
    assert bs.noise_mode() == 0 and bs.noise_cursor() == STEPS
    bs.reset()
    bs.set_x0(case["x0"])
    got = _collect(bs, bs.mpc_rollout(STEPS))
    assert _launches(bs) == 1 and bs.last_launch_name == name and "y" not in got["log"] and bs.noise_cursor() == STEPS
    _identical(got, want, "after dropping")
    with pytest.raises(t.TinyMPCError, match="no mpc_rollout with measurement noise"):
        bs._chk(bs.lib.tinympc_get_mpc_measured(bs.h, np.zeros(4 * STEPS * B).ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "get_mpc_measured")
    bs.close()


@pytest.mark.parametrize("kind", ["process", "measurement"])
@pytest.mark.parametrize("name", ["cartpole20", "cartpole17_plant"])
def test_zero_factor_is_the_plain_chain(hip_lib, monkeypatch, name, kind):
    base = _without(_ncase(name), "gw", "gv")
    _env(monkeypatch, base)
    bs = _solver(base)
    bs.set_x0(base["x0"])
    plain = _collect(bs, bs.mpc_rollout(STEPS))
    assert _launches(bs) == STEPS
    bs.close()
    zero = np.zeros((4, 4, B)) if name == "cartpole20" else np.zeros((4, 4))
    case = dict(base, id=f"zero_{kind}_{name}", **({"gw": zero} if kind == "process" else {"gv": zero}))
    mine = _run(monkeypatch, case, keep=False)
    _identical(mine, plain, f"{name}: all-zero {kind} factor")
    if kind == "measurement":       # what every solve started from: the rounding of the true state
        assert np.array_equal(mine["log"]["y"][:, 1:], mine["log"]["x"][:, :-1]) and np.array_equal(mine["log"]["y"][:, 0], _f32(base["x0"]))


@pytest.mark.parametrize("extra", [("TINYMPC_HIP_LEAN_WS",), ("TINYMPC_HIP_STREAM_MPC",), ("TINYMPC_HIP_LEAN_WS", "TINYMPC_HIP_LEAN_LOOP"),
                                   ("TINYMPC_HIP_STREAM_MPC", "TINYMPC_HIP_STREAM_LOOP"), ("TINYMPC_HIP_NOISE_SPLIT",)],
                         ids=lambda e: "+".join(n[len("TINYMPC_HIP_"):] for n in e))
@pytest.mark.parametrize("name", ["cartpole20", "cartpole17_plant"])
def test_switches_keep_the_chain(hip_lib, monkeypatch, name, extra):
    case = _ncase(name)
    chain = _run(monkeypatch, case)
    switched = _run(monkeypatch, case, extra=extra)      # (`steps` launches: asserted in _run)
    for n in extra:
        monkeypatch.delenv(n, raising=False)
    _same(switched, chain, "+".join(extra))


# ---------------------------------------------------------------------------------------------------------------------------
# (g) refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["adaptive", "cold", "instance_bounds", "overflow"])
def test_rollout_refusals(hip_lib, monkeypatch, what):
    case = _without(_ncase("cartpole17_plant"), "plant", "w")
    _env(monkeypatch, case)
    bs = _solver(case)
    _install_noise(bs, case)
    bs.set_x0(case["x0"])
    cursor = 0
    if what == "adaptive":
        bs.set_adaptive_rho(True)
        want = "noise is not available with adaptive rho"
    elif what == "cold":
        bs.set_warm_start(False)
        want = "needs the persistent workspace"
    elif what == "instance_bounds":
        bs.set_instance_bounds(np.full((4, B), -1e17), np.full((4, B), 1e17), np.full((1, B), -0.5), np.full((1, B), 0.5))
        want = "per-instance bounds have no closed loop by default"
    else:
        cursor = 2 ** 31 - 1 - (STEPS - 1)
        bs.set_noise_cursor(cursor)
        want = "the noise cursor would pass the largest int"
    with pytest.raises(t.TinyMPCError, match=want):
        bs.mpc_rollout(STEPS)
    assert _launches(bs) == -1 and bs.noise_cursor() == cursor and bs.noise_mode() == _mode(case)
    if what == "adaptive":
        bs.set_adaptive_rho(False)
    assert bs.solve() in (0, 1) and np.isfinite(bs.get_solution()["controls"]).all()
    if what == "overflow":          # one step fewer fits: the last step index is the largest int
        bs.set_noise_cursor(cursor - 1)
        bs.mpc_rollout(STEPS)
        assert bs.noise_cursor() == 2 ** 31 - 1
    bs.close()


def test_setter_refusals(hip_lib, monkeypatch):
    case = _ncase("cartpole17_plant")
    _env(monkeypatch, case)
    bs = _solver(case)
    bs.set_x0(case["x0"])
    with pytest.raises(t.TinyMPCError, match="negative"):
        bs.set_noise_cursor(-1)
    G = np.ascontiguousarray(np.eye(4).reshape(-1))
    dp = G.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    for fn in (bs.lib.tinympc_set_process_noise, bs.lib.tinympc_set_measurement_noise):
        for per in (2, -1):
            assert fn(bs.h, dp, per, 1) == -1
            assert b"per_instance is 0" in bs.lib.tinympc_last_error()
    for bad in (np.eye(3), np.zeros((4, 4, B + 1)), np.zeros(5), np.zeros((4, 3))):
        with pytest.raises(t.TinyMPCError, match="expected G"):
            bs.set_process_noise(bad, 1)
        with pytest.raises(t.TinyMPCError, match="expected G"):
            bs.set_measurement_noise(bad, 1)
    bs.set_process_noise(np.full(4, 0.01), 1)        # (a 1-D array is diag(sigma))
    assert np.abs(bs.get_noise(0, 0, 1)[:, 0, 3] - t.host_noise(1, 0, 3, 0, 4, np.full(4, 0.01))).max() <= GEN_TOL
    for args in ((0, -1, 2), (0, 0, 0), (0, 2 ** 31 - 2, 3), (1, 0, 2), (2, 0, 2)):
        with pytest.raises(t.TinyMPCError):
            bs.get_noise(*args)
    assert bs.noise_mode() == 1 and bs.noise_cursor() == 0 and bs.plant_mode() == 10
    assert bs.solve() in (0, 1)
    bs.close()


def test_global_forms(hip_lib, monkeypatch):
    """the process-global solver: the setters, the cursor, get_noise, mpc_rollout's y, the library's own shape checks, and the
    refusal under set_gpus (one device, listed twice)"""
    case = dict(_without(_ncase("cartpole20"), "plant", "w"), id="noise_cartpole20_model_both")
    _env(monkeypatch, case)
    monkeypatch.delenv("TINYMPC_HIP_SHARD_DEVICES", raising=False)
    prob = case["prob"]
    s = t.TinyMPCSolver()
    try:
        t.setup(s, prob.A, prob.B, None, prob.Q, prob.R, prob.rho, 4, 1, prob.N, batch=B, **case["kw"])
        t.set_bound_constraints(s, prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        assert t.noise_mode(s) == 0 and t.noise_cursor(s) == 0
        t.set_process_noise(s, case["gw"], SEED_W)
        t.set_measurement_noise(s, case["gv"], SEED_V)
        assert t.noise_mode(s) == 9
        with pytest.raises(t.TinyMPCError, match="expected G"):
            t.set_process_noise(s, np.zeros((4, 4, B - 1)), 1)
        with pytest.raises(t.TinyMPCError, match="negative"):
            t.set_noise_cursor(s, -2)
        t.set_x0(s, case["x0"])
        log = t.mpc_rollout(s, STEPS)
        assert t.noise_cursor(s) == STEPS
        ref = _run(monkeypatch, case)
        for key in ("x", "u", "y", "iter", "solved"):
            assert np.array_equal(log[key], ref["log"][key]), key
        assert np.array_equal(t.get_noise(s, 1, 0, STEPS), ref["nv"])
        t.set_noise_cursor(s, 2)
        assert t.noise_cursor(s) == 2
        t.set_process_noise(s, None)
        t.set_measurement_noise(s, None)
        assert t.noise_mode(s) == 0 and "y" not in t.mpc_rollout(s, STEPS)
        monkeypatch.setenv("TINYMPC_HIP_SHARD_DEVICES", "0,0")
        t.set_gpus(s, 2)
        for call, word in ((lambda: t.set_process_noise(s, case["gw"], 1), "set_process_noise"), (lambda: t.set_measurement_noise(s, case["gv"], 1), "set_measurement_noise"),
                           (lambda: t.set_noise_cursor(s, 1), "set_noise_cursor"), (lambda: t.noise_cursor(s), "noise_cursor"), (lambda: t.noise_mode(s), "noise_mode")):
            with pytest.raises(t.TinyMPCError, match=word + ": not available on a sharded solver"):
                call()
        t.set_x0(s, case["x0"])
        assert t.solve(s) in (0, 1)
    finally:
        t.cleanup()
