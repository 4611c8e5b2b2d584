"""mpc_rollout against a plant of its own (BatchSolver.set_plant) and under an additive disturbance (set_disturbance): the chain
of `steps` ordinary kept-workspace launches with plant_step_kernel between them (csrc/solver.hip, rollout_chain), on
whatever kernel such a solve takes — no environment switch.

The step rule: the plant state is carried in fp64, the applied control is the fp32 value the solution holds,
x+ = f_p + A_p x + B_p u0 (+ w), and the next solve starts from the fp32 rounding of x+.  The reference is orc64 (the
controller's model) stepped by that rule in numpy fp64, one persistent oracle per instance; the comparison is
tests/test_stream_loop_gpu.py's: every instance at FP32_TOL, an instance whose (iteration count, solved flag) differs at a step
is replayed with the GPU's decision imposed and may differ by one iteration; tolerance-terminated cases take max_iter from the
oracle's own counts so that both exits occur at some step, asserted from those counts.

Perturbations: A_p = A o (1 + 0.02 U), B_p = B o (1 + 0.1 U), U uniform in [-1, 1] per entry (and per instance where the plant
is per instance); w uniform within +-1 % of each state's scale in x0 (the largest |x0| of the row over the batch).  The oracle's
states are asserted finite and bounded (row by row at most twice the excursion of the undisturbed model-plant loops) first.

 (a) cartpole N = 20, input bound, per-instance plant and disturbance: the kernel a kept-workspace solve takes, `steps` launches
 (b) quadrotor N = 10, fixed 10 iterations, shared plant with f_p != 0, shared disturbance, a reference sequence: counts exact
 (c) rocket N = 12, cones, affine term, references, per-instance plant on stream4<6,3> — refused without the plant
 (d) cartpole N = 17 on the generic kernel, disturbance only; and a per-instance-family solver under a disturbance alone, whose
     plant is every instance's own A_b, B_b
 (e) precision 2 on generic<f64> at 1e-6 with exact counts; precision 1 against the host-stepped loop of the same solver
 (f) identity: the model as the plant, or an all-zero disturbance, is today's stream chain bit for bit
 (g) dropping both returns the solver to its own routes: one launch, bit-equal to a fresh solver's
 (h) the stream kernel's in-kernel loop takes no own plant: under both switches an own-plant solver keeps the chain (`steps`
     launches) and its results
 (i) mpc_rollout(3) twice with the disturbance re-set to rows 3..5 in between is mpc_rollout(6), bit for bit
 (j) refusals, by a word of their message, each followed by a plain solve
 (k) the step rule to the bit: the chain against the same launches stepped from the host, the plant step in libm's fma in the
     documented order — every log, the status and x0 equal element for element

Batch 70 (one full stream workgroup and a ragged wavefront), 5 steps.  Every test fails without the feature: set_plant does not
exist there."""
import ctypes

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


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def _perturbed(prob, rng, per_instance):
    sh = (B,) if per_instance else ()
    A = prob.A.reshape(prob.A.shape + (1,) * len(sh)) * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, prob.A.shape + sh))
    Bm = prob.B.reshape(prob.B.shape + (1,) * len(sh)) * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, prob.B.shape + sh))
    return np.asfortranarray(A), np.asfortranarray(Bm)


def _disturbance(x0, rng, steps, per_instance):
    scale = np.abs(x0).max(axis=1)
    sh = (x0.shape[0], steps) + ((B,) if per_instance else ())
    return np.asfortranarray(0.01 * scale.reshape((-1,) + (1,) * (len(sh) - 1)) * rng.uniform(-1.0, 1.0, sh))


def _cartpole20():
    prob = t.problems.cartpole(20, u_bound=0.5)
    rng = np.random.default_rng(31)
    x0 = t.problems.cartpole_x0(B, seed=7)
    return dict(prob=prob, x0=x0, kw=_tol(8), plant=_perturbed(prob, rng, True), w=_disturbance(x0, rng, 6, True))


def _quadrotor10():
    prob = t.problems.quadrotor(10)
    rng = np.random.default_rng(32)
    x0 = t.problems.quadrotor_x0(B, seed=5)
    kw = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=10, check_termination=1)
    fp = 0.005 * np.abs(x0).max(axis=1) * rng.uniform(-1.0, 1.0, 12)
    return dict(prob=prob, x0=x0, kw=kw, seq=quadrotor_tracking_refs(10, STEPS), plant=_perturbed(prob, rng, False) + (fp,),
                w=_disturbance(x0, rng, STEPS, False))


def _rocket12():
    prob = t.problems.rocket(12)
    xr, ur = t.problems.rocket_refs(12)
    rng = np.random.default_rng(33)

    def ext(o):
        o.set_fdyn(prob.fdyn)
        o.set_cone_constraints(*ROCKET_CONES)
        o.set_x_ref(xr)
        o.set_u_ref(ur)
    A, Bm = _perturbed(prob, rng, True)
    fp = np.asfortranarray(np.repeat(prob.fdyn[:, None], B, axis=1) * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (6, B))))
    return dict(prob=prob, x0=t.problems.rocket_x0(B, seed=5), kw=_tol(40), ext=ext, f=prob.fdyn, plant=(A, Bm, fp), name="stream4<6,3>",
                env={"TINYMPC_HIP_NO_MFMAT": "1"})


def _cartpole17(generic):
    prob = t.problems.cartpole(17, u_bound=0.5)
    rng = np.random.default_rng(34)
    x0 = t.problems.cartpole_x0(B, seed=7)
    c = dict(prob=prob, x0=x0, kw=_tol(12), w=_disturbance(x0, rng, STEPS, True), name="stream4<4,1>")
    return dict(c, name="generic", env={"TINYMPC_HIP_NO_STREAM": "1"}) if generic else c


def _cartpole17_plant():
    c = _cartpole17(False)
    return dict(c, plant=_perturbed(c["prob"], np.random.default_rng(36), True), w=_disturbance(c["x0"], np.random.default_rng(37), 6, True))


def _rocket12_dist():
    c = _rocket12()
    return dict(c, w=_disturbance(c["x0"], np.random.default_rng(38), 6, True), env={})


def _cartpole_families():
    """one model per instance (tests/test_stream_loop_gpu.py's families) under a disturbance alone: the plant is every instance's own"""
    base = t.problems.cartpole(17, u_bound=0.5)
    rng = np.random.default_rng(3)
    A = np.repeat(base.A[:, :, None], B, axis=2) * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, (4, 4, B)))
    Bm = np.repeat(base.B[:, :, None], B, axis=2) * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, (4, 1, B)))
    Q, R = np.repeat(base.Q[:, :, None], B, axis=2), np.repeat(base.R[:, :, None], B, axis=2)
    fam = tuple(np.asfortranarray(m) for m in (A, Bm, Q, R)) + (np.full(B, base.rho),)
    x0 = t.problems.cartpole_x0(B, seed=11)
    return dict(prob=base, x0=x0, kw=_tol(12), fam=fam, w=_disturbance(x0, np.random.default_rng(39), STEPS, True), name="stream4<4,1>")


def _quadrotor10_p2():
    prob = t.problems.quadrotor(10)
    prob.x_min, prob.x_max = np.full((12, 10), -0.5), np.full((12, 10), 0.5)
    rng = np.random.default_rng(35)
    x0 = _f32(t.problems.quadrotor_x0(B, seed=8))
    return dict(prob=prob, x0=x0, kw=_tol(40), precision=2, name="generic<f64>", plant=_perturbed(prob, rng, True),
                w=_disturbance(x0, rng, STEPS, True))


CASES = dict(cartpole20=_cartpole20, quadrotor10_sequence=_quadrotor10, rocket12=_rocket12, cartpole17_generic=lambda: _cartpole17(True),
             cartpole17=lambda: _cartpole17(False), cartpole17_plant=_cartpole17_plant, rocket12_dist=_rocket12_dist, cartpole_families=_cartpole_families, quadrotor10_p2=_quadrotor10_p2)
_CASE_CACHE = {}


def _case(name):
    if name not in _CASE_CACHE:
        _CASE_CACHE[name] = dict(CASES[name](), id=name)
    return _CASE_CACHE[name]


def _plant_of(case, b):
    """instance b's (A_p, B_p, f_p): the installed plant, else the model with its affine term"""
    prob = case["prob"]
    if "plant" not in case:
        A, Bm = _model(case, b)[:2]
        return A, Bm, np.asarray(case.get("f", np.zeros(prob.nx)), dtype=np.float64)
    A, Bm = case["plant"][:2]
    f = case["plant"][2] if len(case["plant"]) > 2 else np.zeros(prob.nx)
    if A.ndim == 3:
        return A[:, :, b], Bm[:, :, b], (f[:, b] if f.ndim == 2 else f)
    return A, Bm, f


def _model(case, b):
    if "fam" in case:
        A, Bm, Q, R, rho = case["fam"]
        return A[:, :, b], Bm[:, :, b], Q[:, :, b], R[:, :, b], float(rho[b])
    p = case["prob"]
    return p.A, p.B, p.Q, p.R, p.rho


def _w_of(case, b, k):
    w = case.get("w")
    if w is None:
        return 0.0
    return w[:, k, b] if w.ndim == 3 else w[:, k]


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
        if "seq" in case:
            o.set_x_ref(case["seq"][0][:, :, k])
            o.set_u_ref(case["seq"][1][:, :, k])
        o.solve()
        r = o.get_solution()
        u0 = _f32(r["u"][:, 0])
        x = Ap @ x + Bp @ u0 + fp + _w_of(case, b, k)
        u_log[:, k], x_log[:, k], it[k], so[k] = u0, x, r["iter"], r["solved"]
    ws = o.get_state()
    o.close()
    return dict(u=u_log, x=x_log, iter=it, solved=so, last_x=np.array(r["x"]), last_u=np.array(r["u"]), ws=ws)


def _oracle_loops(oracle, case, steps=STEPS):
    key = (case["id"], steps)
    if key not in _ORACLE:
        loops = [_oracle_loop(oracle, case, b, steps) for b in range(B)]
        so, x = np.stack([r["solved"] for r in loops], axis=-1), np.stack([r["x"] for r in loops], axis=-1)
        if case["kw"]["abs_pri_tol"] > 0.0:      # both exits in the batch at some step, by the oracle's own counts
            assert any(0 < so[k].sum() < B for k in range(steps)), (key, so.sum(axis=1))
        # finite, and bounded: row by row at most twice the excursion of the same loops on the model plant without disturbance
        # (a 2 % / 10 % mismatch and a 1 % disturbance over a handful of steps perturb the closed loop, they do not double it)
        nominal = {k: v for k, v in case.items() if k not in ("plant", "w")}
        xn = np.stack([_oracle_loop(oracle, nominal, b, steps)["x"] for b in range(B)], axis=-1)
        bound = 2.0 * np.maximum(np.abs(xn).max(axis=(1, 2)), np.abs(case["x0"]).max(axis=1))
        assert np.isfinite(x).all() and (np.abs(x).max(axis=(1, 2)) <= bound).all(), (key, np.abs(x).max(axis=(1, 2)) / bound)
        _ORACLE[key] = loops
    return _ORACLE[key]


def _stack(loops, key):
    return np.stack([r[key] for r in loops], axis=-1)


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU's runs
# ---------------------------------------------------------------------------------------------------------------------------
def _env(monkeypatch, case, mpc=False, loop=False):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in case.get("env", {}).items():
        monkeypatch.setenv(name, v)
    if mpc:
        monkeypatch.setenv("TINYMPC_HIP_STREAM_MPC", "1")
    if loop:
        monkeypatch.setenv("TINYMPC_HIP_STREAM_LOOP", "1")


def _solver(case, precision=None, own=True):
    prob = case["prob"]
    if "fam" in case:
        bs = t.BatchSolver.from_families(*case["fam"], prob.N)
    else:
        bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    _configure(bs, case)
    if "seq" in case:
        bs.set_ref_sequence(*case["seq"])
    bs.set_warm_start(True)
    precision = case.get("precision", 0) if precision is None else precision
    if precision:
        bs.set_precision(precision)
        if precision == 1:
            bs.set_strict_precision(True)
    if own:
        _install(bs, case)
    return bs


def _install(bs, case, rows=None):
    if "plant" in case:
        bs.set_plant(*case["plant"])
    if "w" in case:
        bs.set_disturbance(case["w"] if rows is None else np.asfortranarray(case["w"][:, rows[0]:rows[1]]))


def _mode(case):
    m = 0
    if "plant" in case:
        m |= 2 if case["plant"][0].ndim == 3 else 1
    if "w" in case:
        m |= 8 if case["w"].ndim == 3 else 4
    return m


def _plain_launch_name(case):
    """the kernel a kept-workspace solve of the case's solver takes (no plant installed)"""
    bs = _solver(case, own=False)
    bs.set_x0(case["x0"])
    bs.solve()
    name = bs.last_launch_name
    bs.close()
    return name


def _join(logs):
    return dict(status=logs[-1]["status"], x=np.concatenate([l["x"] for l in logs], axis=1), u=np.concatenate([l["u"] for l in logs], axis=1),
                iter=np.concatenate([l["iter"] for l in logs], axis=0), solved=np.concatenate([l["solved"] for l in logs], axis=0))


def _run(monkeypatch, case, steps=STEPS, mpc=False, loop=False, own=True):
    _env(monkeypatch, case, mpc, loop)
    want = _plain_launch_name(case)
    if "name" in case:
        assert want == case["name"], want
    bs = _solver(case, own=own)
    assert bs.plant_mode() == (_mode(case) if own else 0)
    bs.set_x0(case["x0"])
    log = bs.mpc_rollout(steps)
    assert bs.last_launch_name == want, (bs.last_launch_name, want)
    if own:
        assert _launches(bs) == steps, (_launches(bs), steps)
    out = _collect(bs, log)
    out["launches"] = _launches(bs)
    bs.close()
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


def _plant_acts(case, run):
    """the first step's x+ is the PLANT's, not the model's: it differs from the model's step by far more than fp32 rounding"""
    prob, x1, u0 = case["prob"], run["log"]["x"][:, 0, :], run["log"]["u"][:, 0, :]
    model = prob.A @ case["x0"] + prob.B @ u0 + np.asarray(case.get("f", np.zeros(prob.nx)))[:, None]
    assert np.abs(x1 - model).max() > 1e-4 * np.abs(x1).max()


# ---------------------------------------------------------------------------------------------------------------------------
# (a) - (d) against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole20", "quadrotor10_sequence", "rocket12", "cartpole17_generic", "cartpole_families"])
def test_own_plant_chain_vs_oracle(hip_lib, oracle_built, monkeypatch, name):
    case = _case(name)
    run = _run(monkeypatch, case)
    fixed = case["kw"]["abs_pri_tol"] == 0.0
    _check_vs_oracle(oracle_built, case, run, FP32_TOL, exact=fixed)
    if fixed:
        assert np.all(run["log"]["iter"] == case["kw"]["max_iter"]) and not run["log"]["solved"].any()
    if "fam" in case:       # (the disturbed plant is every instance's own model: the first step's x+ - A_b x0 - B_b u0 is w, to fp32 rounding)
        A, Bm = case["fam"][:2]
        x1, u0 = run["log"]["x"][:, 0, :], run["log"]["u"][:, 0, :]
        rest = x1 - np.einsum("ijb,jb->ib", A, case["x0"]) - np.einsum("ijb,jb->ib", Bm, u0)
        assert np.abs(rest - case["w"][:, 0, :]).max() <= 1e-6 * np.abs(x1).max()
    else:
        _plant_acts(case, run)


def test_refused_without_the_plant(hip_lib, monkeypatch):
    """(c)'s shape has no closed loop of its own: the same solver without a plant is refused as before"""
    case = _case("rocket12")
    _env(monkeypatch, case)
    bs = _solver(case, own=False)
    bs.set_x0(case["x0"])
    with pytest.raises(t.TinyMPCError, match="no kernel with a fused closed loop"):
        bs.mpc_rollout(STEPS)
    assert bs.solve() in (0, 1) and bs.last_launch_name == "stream4<6,3>"
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (e) precision 2 and precision 1
# ---------------------------------------------------------------------------------------------------------------------------
def test_precision2(hip_lib, oracle_built, monkeypatch):
    case = _case("quadrotor10_p2")
    run = _run(monkeypatch, case)
    loops = _check_vs_oracle(oracle_built, case, run, TIGHT, exact=True)
    for key in ("d", "y", "g", "v", "z"):
        e = max(np.abs(run["ws"][key][:, :, b] - loops[b]["ws"][key]).max() / max(np.abs(loops[b]["ws"][key]).max(), 1e-2) for b in range(B))
        assert e <= TIGHT, f"workspace {key} {e:.3e}"
    _plant_acts(case, run)


def test_precision1_vs_host_stepped(hip_lib, monkeypatch):
    """precision 1: the chain against the loop a caller steps on the same solver, the same rule with the GPU's fp32 controls"""
    case = _case("cartpole17_plant")
    _env(monkeypatch, case)
    bs = _solver(case, precision=1)
    bs.set_x0(case["x0"])
    log = bs.mpc_rollout(STEPS)
    assert bs.last_launch_name == "stream4<4,1>" and bs.effective_precision == 1 and _launches(bs) == STEPS
    sol = bs.get_solution()
    bs.close()
    hs = _solver(case, precision=1, own=False)
    Ap, Bp = case["plant"]
    x = np.array(case["x0"], dtype=np.float64)
    u, xl = np.zeros((1, STEPS, B)), np.zeros((4, STEPS, B))
    it, so = np.zeros((STEPS, B), dtype=int), np.zeros((STEPS, B), dtype=int)
    for k in range(STEPS):
        hs.set_x0(_f32(x))
        hs.solve()
        s, st = hs.get_solution(), hs.get_status()
        u[:, k, :] = s["controls"][:, 0, :]
        x = np.einsum("ijb,jb->ib", Ap, x) + np.einsum("ijb,jb->ib", Bp, u[:, k, :]) + case["w"][:, k, :]
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
# (f) identity
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["model_as_plant", "zero_disturbance"])
@pytest.mark.parametrize("name", ["cartpole17", "rocket12"])
def test_identity(hip_lib, monkeypatch, name, what):
    """under TINYMPC_HIP_STREAM_MPC=1: the model installed as the plant, or an all-zero disturbance, is the stream chain"""
    base = _case(name)
    prob = base["prob"]
    case = {k: v for k, v in base.items() if k not in ("plant", "w", "env")}
    if what == "model_as_plant":
        own = dict(case, plant=(prob.A, prob.B, np.asarray(case.get("f", np.zeros(prob.nx)), dtype=np.float64)))
    else:
        own = dict(case, w=np.zeros((prob.nx, STEPS)))
    today = _run(monkeypatch, case, mpc=True, own=False)
    assert today["launches"] == STEPS
    mine = _run(monkeypatch, own, mpc=True)
    _identical(mine, today, f"{name} {what}")
    assert np.abs(today["log"]["u"]).max() > 0.0 and len(np.unique(today["log"]["x"][:, -1, :])) > B


# ---------------------------------------------------------------------------------------------------------------------------
# (g) dropping
# ---------------------------------------------------------------------------------------------------------------------------
def test_dropping_returns_the_solver(hip_lib, monkeypatch):
    case = _case("cartpole20")
    _env(monkeypatch, case)
    fresh = _solver(case, own=False)
    fresh.set_x0(case["x0"])
    want = _collect(fresh, fresh.mpc_rollout(STEPS))
    assert _launches(fresh) == 1
    name = fresh.last_launch_name
    fresh.close()
    bs = _solver(case)
    bs.set_x0(case["x0"])
    bs.mpc_rollout(STEPS)
    assert _launches(bs) == STEPS
    bs.set_plant(None, None)
    assert bs.plant_mode() == 8
    bs.set_disturbance(None)
    assert bs.plant_mode() == 0
    bs.reset()
    bs.set_x0(case["x0"])
    got = _collect(bs, bs.mpc_rollout(STEPS))
    assert _launches(bs) == 1 and bs.last_launch_name == name
    _identical(got, want, "after dropping")
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (h) under the stream kernel's switches an own-plant solver keeps the chain
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole17_plant", "rocket12_dist"])
def test_switches_keep_the_chain(hip_lib, monkeypatch, name):
    case = _case(name)
    chain = _run(monkeypatch, case)
    both = _run(monkeypatch, case, mpc=True, loop=True)      # (`steps` launches: asserted in _run)
    _identical(both, chain, name)


# ---------------------------------------------------------------------------------------------------------------------------
# (i) continuation
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole20", "cartpole17_plant"])
def test_two_rollouts_are_one(hip_lib, monkeypatch, name):
    case = _case(name)
    whole = _run(monkeypatch, case, steps=6)
    _env(monkeypatch, case)
    bs = _solver(case)
    bs.set_x0(case["x0"])
    logs = [bs.mpc_rollout(3)]
    _install(bs, case, rows=(3, 6))
    logs.append(bs.mpc_rollout(3))
    halves = _collect(bs, _join(logs))
    bs.close()
    _identical(halves, whole, f"{name} 3 + 3 vs 6")


# ---------------------------------------------------------------------------------------------------------------------------
# (j) refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["short_disturbance", "adaptive", "cold"])
def test_rollout_refusals(hip_lib, monkeypatch, what):
    case = _case("cartpole20")
    _env(monkeypatch, case)
    bs = _solver(case)
    bs.set_x0(case["x0"])
    if what == "short_disturbance":
        bs.set_disturbance(np.asfortranarray(case["w"][:, :3]))
        want = "the disturbance holds 3 steps"
    elif what == "adaptive":
        bs.set_adaptive_rho(True)
        want = "not available with adaptive rho"
    else:
        bs.set_warm_start(False)
        want = "needs the persistent workspace"
    with pytest.raises(t.TinyMPCError, match=want):
        bs.mpc_rollout(STEPS)
    assert _launches(bs) == -1
    assert bs.solve() in (0, 1) and np.isfinite(bs.get_solution()["controls"]).all()
    bs.close()


def test_wrong_shapes(hip_lib, monkeypatch):
    case = _case("cartpole20")
    _env(monkeypatch, case)
    prob = case["prob"]
    bs = _solver(case, own=False)
    bs.set_x0(case["x0"])
    A, Bm = case["plant"]
    for args in ((prob.A[:3], prob.B), (prob.A, prob.B.T), (A[:, :, :B - 1], Bm[:, :, :B - 1]), (A, prob.B), (prob.A, prob.B, np.zeros(5)),
                 (prob.A, None)):
        with pytest.raises(t.TinyMPCError, match="expected"):
            bs.set_plant(*args)
    for w in (np.zeros((3, STEPS)), np.zeros((4, STEPS, B + 1)), np.zeros(4), np.zeros((4, 0))):
        with pytest.raises(t.TinyMPCError, match="expected"):
            bs.set_disturbance(w)
    assert bs.plant_mode() == 0
    assert bs.solve() in (0, 1)
    bs.close()


def test_global_forms(hip_lib, monkeypatch):
    """the process-global solver: set_plant / set_disturbance / plant_mode, the library's own shape checks, and the refusal under
    set_gpus (one device, listed twice)"""
    case = _case("cartpole20")
    _env(monkeypatch, case)
    monkeypatch.delenv("TINYMPC_HIP_SHARD_DEVICES", raising=False)
    prob = case["prob"]
    A, Bm = case["plant"]
    s = t.TinyMPCSolver()
    try:
        t.setup(s, prob.A, prob.B, None, prob.Q, prob.R, prob.rho, 4, 1, prob.N, batch=B, **case["kw"])
        t.set_bound_constraints(s, prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        t.set_plant(s, A, Bm)
        t.set_disturbance(s, case["w"])
        assert t.plant_mode(s) == 10
        with pytest.raises(t.TinyMPCError, match="expected"):
            t.set_plant(s, A[:, :, :B - 1], Bm[:, :, :B - 1])
        with pytest.raises(t.TinyMPCError, match="expected"):
            t.set_disturbance(s, np.zeros((3, STEPS)))
        t.set_x0(s, case["x0"])
        log = t.mpc_rollout(s, STEPS)
        bs = _solver(case)
        bs.set_x0(case["x0"])
        ref = bs.mpc_rollout(STEPS)
        bs.close()
        for key in ("x", "u", "iter", "solved"):
            assert np.array_equal(log[key], ref[key]), key
        t.set_plant(s, None, None)
        t.set_disturbance(s, None)
        assert t.plant_mode(s) == 0
        monkeypatch.setenv("TINYMPC_HIP_SHARD_DEVICES", "0,0")
        t.set_gpus(s, 2)
        for call, word in ((lambda: t.set_plant(s, A, Bm), "set_plant"), (lambda: t.set_disturbance(s, case["w"]), "set_disturbance"),
                           (lambda: t.plant_mode(s), "plant_mode")):
            with pytest.raises(t.TinyMPCError, match=word + ": not available on a sharded solver"):
                call()
        t.set_x0(s, case["x0"])
        assert t.solve(s) in (0, 1)
    finally:
        t.cleanup()


# ---------------------------------------------------------------------------------------------------------------------------
# (k) the step rule, to the bit
# ---------------------------------------------------------------------------------------------------------------------------
_LIBM_FMA = ctypes.CDLL("libm.so.6").fma
_LIBM_FMA.restype = ctypes.c_double
_LIBM_FMA.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double]


def _rule_row(A, Bm, f, x, u0, r):
    """row r of f + A x + B u0 as plant_step_kernel sums it: from f[r], A's row by ascending column, then B's, one fma each"""
    acc = float(f[r])
    for j in range(x.size):
        acc = _LIBM_FMA(A[r, j], x[j], acc)
    for a in range(u0.size):
        acc = _LIBM_FMA(Bm[r, a], u0[a], acc)
    return acc


def _bits_case(name):
    """(case, under TINYMPC_HIP_STREAM_MPC): the builders above; the noise factors are tests/test_noise_loop_gpu.py's"""
    if name == "rocket12_model":
        return {k: v for k, v in _case("rocket12").items() if k != "plant"}, True
    if name == "cartpole17_plant_noise":
        from tests.test_noise_loop_gpu import _ncase
        return _ncase("cartpole17_plant"), False
    return _case(name), False


@pytest.mark.parametrize("name", ["cartpole17_plant", "rocket12_model", "cartpole_families", "cartpole17_plant_noise"])
def test_step_rule_bits(hip_lib, monkeypatch, name):
    """mpc_rollout(STEPS) on the stream kernel (precision 0, every launch from the fp32 d_x0) against the same loop stepped from
    the host on a second, identical solver — set_x0 of the fp32 state, solve, the fp32 controls[:, 0, :] — advanced by the rule in
    fp64 on the host: acc = f[r], A's row by ascending column, B's row, one libm fma each, + w[r], + (G_w xi_w)[r] last; the next
    solve from (float)(acc + (G_v xi_v[t + 1])[r]).  The realised G xi are get_noise's, the device's own function.  Everything is
    equal element for element.  Batch 70: at nx = 4 one full 64-instance workgroup of the step kernel and a ragged one, at
    nx = 6 42 instances per workgroup and 4 idle lanes.
      cartpole17_plant        per-instance plant and per-instance disturbance
      rocket12_model          no plant installed, TINYMPC_HIP_STREAM_MPC=1: the model with f != 0, cones
      cartpole_families       a disturbance alone: every instance's own model block
      cartpole17_plant_noise  process (shared G_w) and measurement (per-instance G_v) noise; the measured log too"""
    case, mpc = _bits_case(name)
    prob = case["prob"]
    _env(monkeypatch, case, mpc=mpc)
    bs = _solver(case)
    if "gw" in case:
        from tests.test_noise_loop_gpu import _install_noise
        _install_noise(bs, case)
    bs.set_x0(case["x0"])
    log = bs.mpc_rollout(STEPS)
    assert bs.last_launch_name == case["name"] and _launches(bs) == STEPS and bs.effective_precision == 0
    got = _collect(bs, log)
    nw, nv = (bs.get_noise(0, 0, STEPS), bs.get_noise(1, 0, STEPS)) if "gw" in case else (None, None)
    bs.close()

    hs = _solver(case, own=False)
    x = np.array(_f32(case["x0"]), dtype=np.float64)
    plants = [_plant_of(case, b) for b in range(B)]
    for k in range(STEPS):
        y = _f32(x if nv is None else x + nv[:, k, :])
        hs.set_x0(y)
        hs.solve()
        u0, st = hs.get_solution()["controls"][:, 0, :], hs.get_status()
        nxt = np.zeros_like(x)
        for b in range(B):
            A, Bm, f = plants[b]
            for r in range(prob.nx):
                acc = _rule_row(A, Bm, f, x[:, b], u0[:, b], r)
                if "w" in case:
                    acc = acc + float(_w_of(case, b, k)[r])
                if nw is not None:
                    acc = acc + float(nw[r, k, b])
                nxt[r, b] = acc
        x = nxt
        if nv is not None:
            assert np.array_equal(log["y"][:, k, :], y), f"{name}: step {k}, measured state"
        assert np.array_equal(log["u"][:, k, :], u0), f"{name}: step {k}, u log"
        assert np.array_equal(log["x"][:, k, :], _f32(x)), f"{name}: step {k}, x log"
        assert np.array_equal(log["iter"][k], st["iter"]) and np.array_equal(log["solved"][k], st["solved"]), f"{name}: step {k}, iter / solved"
    assert hs.last_launch_name == case["name"]
    hs.close()
    assert np.array_equal(got["x0"], _f32(x).T.astype(np.float32)), f"{name}: x0 after the loop"
    assert np.abs(log["u"]).max() > 0.0 and len(np.unique(log["x"][:, -1, :])) > B
