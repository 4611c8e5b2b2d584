"""mpc_rollout on the stream and generic kernels (csrc/admm_streamg.hip.h, csrc/admm_generic.hip.h) behind
TINYMPC_HIP_STREAM_MPC=1 — the chain of `steps` workspace-carrying launches with the generalised plant step between them
(Solver::rollout_chain, plant_step_kernel) — and, with TINYMPC_HIP_STREAM_LOOP=1 beside it, ONE launch of the stream
kernel's in-kernel loop (admm_streamg_mpc_kernel) where one is built.

The step rule at every precision: the plant state is carried in fp64, the applied control is the fp32 value the solution
holds, x+ = f + A x + B u0, and the next solve starts from the fp32 rounding of x+.  The reference is orc64 stepped by exactly
that rule, one persistent oracle per instance.

 (a) the chain against the oracle, EVERY instance at FP32_TOL (applied controls, plant states, the last solve), by the method
     of tests/test_ref_sequence_gpu.py::_check_vs_oracle: an instance whose (iteration count, solved flag) differs at some
     step is replayed with the GPU's decisions imposed and may differ by at most one iteration; fixed-iteration cases agree
     on every count.  Precision 1 is held to the host-stepped loop of the same solver at FP32_TOL.
 (b) precision 2 on generic<f64> and stream4<12,4;f64>, at tests/test_stream_f64_gpu.py's bars: 1e-6 on logs, last solution
     and workspace, iteration counts and solved flags exact.
 (c) the loop against the chain: bit-identical logs, last solution, status, residuals, workspace and the x0 left behind —
     the loop does the chain's arithmetic in the chain's order.  A case without a loop kernel reports `steps` launches.
 (d) mpc_rollout(3) twice is mpc_rollout(6), bit for bit, on both forms.
 (e) with the switches off the parent's two refusals are raised unchanged and a plain solve follows.

Batch 70: one full stream workgroup (64 instances) and a ragged wavefront.  The tolerance-terminated cases take max_iter
from the oracle's own iteration counts so that converged and max_iter exits both occur in the batch at some step; the mix is
asserted from the oracle's counts.  Tests (a)-(d) fail without the feature: mpc_rollout raises there.

Loop kernels that are not built (csrc/streamg_entry.hip.h, streamg_mpc_built) and so keep the chain here: every fp32-state
form of (12, 4) — the quadrotor case — and the generic kernel; precision 1 has no loop form."""
import ctypes

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.test_ref_sequence import quadrotor_tracking_refs
from tests.util import FP32_TOL, load_golden, nrel, problem_of

pytestmark = pytest.mark.gpu

B, STEPS = 70, 5
TIGHT = 1e-6
ROCKET_CONES = ([0], [3], [0.25], [0], [3], [0.5])


def _f32(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float32).astype(np.float64))


def _launches(bs):
    f = ctypes.CDLL(t.LIB_PATH).tmpc_last_rollout_launches
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p]
    return f(bs.h)


def _tol(max_iter):
    return dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=max_iter, check_termination=1)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases: problem, inputs, how a solver (GPU or oracle: the setters have the same names) is configured, where it runs
# ---------------------------------------------------------------------------------------------------------------------------
def _cartpole17():
    prob = t.problems.cartpole(17, u_bound=0.5)
    return dict(prob=prob, x0=t.problems.cartpole_x0(B, seed=7), kw=_tol(12), name="stream4<4,1>", loop=True)


def _cartpole17_generic():
    return dict(_cartpole17(), name="generic", env={"TINYMPC_HIP_NO_STREAM": "1"}, loop=False, key="cartpole17")


def _quadrotor7():
    prob = t.problems.quadrotor(7)
    xs, us = quadrotor_tracking_refs(7, STEPS)
    kw = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=10, check_termination=1)
    return dict(prob=prob, x0=t.problems.quadrotor_x0(B, seed=5), kw=kw, seq=(xs, us), name="stream4<12,4>", loop=False)


def _rocket12():
    prob = t.problems.rocket(12)
    xr, ur = t.problems.rocket_refs(12)

    def ext(o):
        o.set_fdyn(prob.fdyn)
        o.set_cone_constraints(*ROCKET_CONES)
        o.set_x_ref(xr)
        o.set_u_ref(ur)
    return dict(prob=prob, x0=t.problems.rocket_x0(B, seed=5), kw=_tol(40), ext=ext, f=prob.fdyn, name="stream4<6,3>", loop=True)


def _cartpole_rows():
    g = load_golden("X3_cartpole_linear_rows")
    prob = problem_of(g)
    lin = (np.array(g["lin"]["Ax"]), np.array(g["lin"]["bx"]), np.array(g["lin"]["Au"]), np.array(g["lin"]["bu"]))
    return dict(prob=prob, x0=t.problems.cartpole_x0(B, seed=9), kw=_tol(15), ext=lambda o: o.set_linear_constraints(*lin),
                name="stream4<4,1>", loop=True)


def _cartpole_families():
    base = t.problems.cartpole(17, u_bound=0.5)
    rng = np.random.default_rng(3)
    A = np.repeat(base.A[:, :, None], B, axis=2) * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, (4, 4, B)))
    Bm = np.repeat(base.B[:, :, None], B, axis=2) * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, (4, 1, B)))
    Q = np.repeat(base.Q[:, :, None], B, axis=2)
    R = np.repeat(base.R[:, :, None], B, axis=2)
    fam = tuple(np.asfortranarray(m) for m in (A, Bm, Q, R)) + (np.full(B, base.rho),)
    return dict(prob=base, x0=t.problems.cartpole_x0(B, seed=11), kw=_tol(12), fam=fam, name="stream4<4,1>", loop=True)


def _quadrotor10_p2(stream):
    """the state-bounded quadrotor of tests/test_stream_f64_gpu.py::test_workspace_kept_closed_loop, precision 2"""
    prob = t.problems.quadrotor(10)
    prob.x_min, prob.x_max = np.full((12, 10), -0.5), np.full((12, 10), 0.5)
    c = dict(prob=prob, x0=_f32(t.problems.quadrotor_x0(B, seed=8)), kw=_tol(40), precision=2, key="quadrotor10_p2")
    if stream:
        return dict(c, name="stream4<12,4;f64>", env={"TINYMPC_HIP_STREAM_F64": "1"}, loop=True)
    return dict(c, name="generic<f64>", loop=False)


CASES = dict(cartpole17=_cartpole17, cartpole17_generic=_cartpole17_generic, quadrotor7_sequence=_quadrotor7, rocket12_cones_fdyn=_rocket12,
             cartpole_linear_rows=_cartpole_rows, cartpole_families=_cartpole_families,
             quadrotor10_p2_generic=lambda: _quadrotor10_p2(False), quadrotor10_p2_stream=lambda: _quadrotor10_p2(True))
_CASE_CACHE = {}


def _case(name):
    if name not in _CASE_CACHE:
        _CASE_CACHE[name] = dict(CASES[name](), id=name)
    return _CASE_CACHE[name]


def _configure(o, case):
    prob = case["prob"]
    o.update_settings(**case["kw"])
    o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if "ext" in case:
        case["ext"](o)
    return o


def _model(case, b):
    if "fam" in case:
        A, Bm, Q, R, rho = case["fam"]
        return A[:, :, b], Bm[:, :, b], Q[:, :, b], R[:, :, b], float(rho[b])
    p = case["prob"]
    return p.A, p.B, p.Q, p.R, p.rho


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's loops: computed once per case, shared between the tests, never written to
# ---------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_loop(oracle, case, b, steps, forced=None):
    """one instance through the step rule on orc64: u (nu, steps) applied (fp32 values), x (nx, steps) plant states (fp64),
    iter, solved (steps,), the last solve's trajectories and the workspace it left"""
    prob = case["prob"]
    A, Bm, Q, R, rho = _model(case, b)
    o = _configure(oracle.CpuSolver("orc64", A, Bm, Q, R, rho, prob.N), case)
    f = np.asarray(case.get("f", np.zeros(prob.nx)), dtype=np.float64)
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
        x = A @ x + Bm @ u0 + f
        u_log[:, k], x_log[:, k], it[k], so[k] = u0, x, r["iter"], r["solved"]
    ws = o.get_state()
    o.close()
    return dict(u=u_log, x=x_log, iter=it, solved=so, last_x=np.array(r["x"]), last_u=np.array(r["u"]), ws=ws)


def _oracle_loops(oracle, case, steps=STEPS):
    key = (case.get("key", case["id"]), steps)
    if key not in _ORACLE:
        loops = [_oracle_loop(oracle, case, b, steps) for b in range(B)]
        so = np.stack([r["solved"] for r in loops], axis=-1)
        if case["kw"]["abs_pri_tol"] > 0.0:      # both exits in the batch at some step, by the oracle's own counts
            assert any(0 < so[k].sum() < B for k in range(steps)), (key, so.sum(axis=1))
        _ORACLE[key] = loops
    return _ORACLE[key]


def _stack(loops, key):
    return np.stack([r[key] for r in loops], axis=-1)


def _rel(a, ref):
    den = np.abs(ref).max(axis=(0, 1))
    return np.abs(a - ref).max(axis=(0, 1)) / np.where(den == 0.0, 1.0, den)


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU's runs: one per (case, form, steps), kept for the tests that compare them
# ---------------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _env(monkeypatch, case, mpc, loop):
    for name in ("TINYMPC_HIP_STREAM_MPC", "TINYMPC_HIP_STREAM_LOOP", "TINYMPC_HIP_NO_STREAM", "TINYMPC_HIP_STREAM_F64"):
        monkeypatch.delenv(name, raising=False)
    for name, v in case.get("env", {}).items():
        monkeypatch.setenv(name, v)
    if mpc:
        monkeypatch.setenv("TINYMPC_HIP_STREAM_MPC", "1")
    if loop:
        monkeypatch.setenv("TINYMPC_HIP_STREAM_LOOP", "1")


def _solver(case, precision=None):
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
    return bs


def _x0_left(bs):
    import torch
    from tinympc_julia_amd import sharding
    x0 = sharding.device_tensor(bs.device_buffers()["x0"], (bs.batch, bs.nx), torch.float32, torch.device("cuda", 0))
    return x0.cpu().numpy().copy()


def _collect(bs, log):
    return dict(log=log, sol=bs.get_solution(), st=bs.get_status(), ws=bs.get_workspace(), status=bs.solve_status(), x0=_x0_left(bs))


def _run(monkeypatch, case, loop, steps=STEPS, split=None):
    """mpc_rollout(steps) — split = (a, b): mpc_rollout(a) then mpc_rollout(b), the logs joined — with the kernel, the launch
    and the number of solve launches asserted"""
    key = (case["id"], loop, steps, split)
    if key in _RUNS:
        return _RUNS[key]
    _env(monkeypatch, case, True, loop)
    bs = _solver(case)
    bs.set_x0(case["x0"])
    assert _launches(bs) == -1
    one = loop and case["loop"]
    logs = []
    for n in (split or (steps,)):
        logs.append(bs.mpc_rollout(n))
        assert bs.kernel_name == case["name"] and bs.last_launch_name == case["name"], (bs.kernel_name, bs.last_launch_name)
        assert _launches(bs) == (1 if one else n), (_launches(bs), n)
    log = dict(status=logs[-1]["status"], x=np.concatenate([l["x"] for l in logs], axis=1), u=np.concatenate([l["u"] for l in logs], axis=1),
               iter=np.concatenate([l["iter"] for l in logs], axis=0), solved=np.concatenate([l["solved"] for l in logs], axis=0))
    out = _collect(bs, log)
    bs.close()
    for a in (out["log"], out["sol"], out["st"], out["ws"]):
        for v in a.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    _RUNS[key] = out
    return out


def _identical(a, c, tag):
    for key in ("x", "u", "iter", "solved"):
        assert np.array_equal(a["log"][key], c["log"][key]), f"{tag}: log {key}"
    assert a["log"]["status"] == c["log"]["status"] and a["status"] == c["status"], tag
    for key in ("states", "controls"):
        assert np.array_equal(a["sol"][key], c["sol"][key]), f"{tag}: last solution, {key}"
    for key in ("iter", "solved", "residuals"):
        assert np.array_equal(a["st"][key], c["st"][key]), f"{tag}: {key}"
    for key in ("d", "y", "g", "v", "z"):
        assert np.array_equal(a["ws"][key], c["ws"][key]), f"{tag}: workspace {key}"
    assert np.array_equal(a["x0"], c["x0"]), f"{tag}: the x0 left behind"


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the chain against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def _check_vs_oracle(oracle, case, run, tol, exact):
    """every instance against its oracle loop at `tol`; exact: every (iteration count, solved flag) must be the oracle's"""
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


CHAIN_CASES = ["cartpole17", "cartpole17_generic", "quadrotor7_sequence", "rocket12_cones_fdyn", "cartpole_linear_rows", "cartpole_families"]


@pytest.mark.parametrize("name", CHAIN_CASES)
def test_chain_vs_oracle(hip_lib, oracle_built, monkeypatch, name):
    case = _case(name)
    run = _run(monkeypatch, case, loop=False)
    fixed = case["kw"]["abs_pri_tol"] == 0.0
    _check_vs_oracle(oracle_built, case, run, FP32_TOL, exact=fixed)
    if fixed:
        assert np.all(run["log"]["iter"] == case["kw"]["max_iter"]) and not run["log"]["solved"].any()
    if "fam" in case:
        assert len(np.unique(run["log"]["iter"])) > 3, "the families do not differ"
    if name == "rocket12_cones_fdyn":       # (the plant carries f: the first step's x+ - A x0 - B u0 is f, to fp32 rounding of x+)
        prob, x1, u0 = case["prob"], run["log"]["x"][:, 0, :], run["log"]["u"][:, 0, :]
        rest = x1 - prob.A @ case["x0"] - prob.B @ u0
        assert np.abs(rest - prob.fdyn[:, None]).max() <= 1e-6 * np.abs(x1).max() and np.abs(prob.fdyn).max() > 0.4


def test_chain_precision1_vs_host_stepped(hip_lib, monkeypatch):
    """precision 1 (fp32 recurrences, "stream4<4,1>" with strict precision): the chain against the loop a caller steps on
    the same solver — set_x0 of the fp32 rounding, solve, u0 from the solution, the plant in fp64 on the host"""
    case = _case("cartpole17")
    prob = case["prob"]
    _env(monkeypatch, case, True, True)      # (both switches: precision 1 has no loop kernel, the chain takes it)
    bs = _solver(case, precision=1)
    bs.set_x0(case["x0"])
    log = bs.mpc_rollout(STEPS)
    assert bs.kernel_name == "stream4<4,1>" and bs.last_launch_name == "stream4<4,1>" and bs.effective_precision == 1
    assert _launches(bs) == STEPS
    sol = bs.get_solution()
    bs.close()
    hs = _solver(case, precision=1)
    x = np.array(case["x0"], dtype=np.float64)
    u, xl = np.zeros((prob.nu, STEPS, B)), np.zeros((prob.nx, STEPS, B))
    it, so = np.zeros((STEPS, B), dtype=int), np.zeros((STEPS, B), dtype=int)
    for k in range(STEPS):
        hs.set_x0(_f32(x))
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
# (b) precision 2
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quadrotor10_p2_generic", "quadrotor10_p2_stream"])
def test_chain_precision2(hip_lib, oracle_built, monkeypatch, name):
    case = _case(name)
    run = _run(monkeypatch, case, loop=False)
    loops = _check_vs_oracle(oracle_built, case, run, TIGHT, exact=True)
    for key in ("d", "y", "g", "v", "z"):
        e = max(np.abs(run["ws"][key][:, :, b] - loops[b]["ws"][key]).max() / max(np.abs(loops[b]["ws"][key]).max(), 1e-2) for b in range(B))
        assert e <= TIGHT, f"{name}: workspace {key} {e:.3e}"
    assert np.abs(run["ws"]["g"]).max() > 1.0       # (the state bounds act: duals far above the trajectory's scale)


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the loop against the chain
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES])
def test_loop_is_the_chain(hip_lib, monkeypatch, name):
    """bit-identical wherever a loop kernel exists (one launch); elsewhere TINYMPC_HIP_STREAM_LOOP changes nothing: `steps`
    launches (asserted in _run) and the chain's results"""
    case = _case(name)
    chain = _run(monkeypatch, case, loop=False)
    loop = _run(monkeypatch, case, loop=True)
    _identical(loop, chain, name)
    assert np.abs(chain["log"]["u"]).max() > 0.0 and len(np.unique(chain["log"]["x"][:, -1, :])) > B


# ---------------------------------------------------------------------------------------------------------------------------
# (d) continuation
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", [False, True], ids=["chain", "loop"])
@pytest.mark.parametrize("name", ["cartpole17", "rocket12_cones_fdyn"])
def test_two_rollouts_are_one(hip_lib, monkeypatch, name, loop):
    """mpc_rollout(3) twice is mpc_rollout(6): the second loop goes on from the fp64 plant state and the workspace the first left"""
    case = _case(name)
    whole = _run(monkeypatch, case, loop, steps=6)
    halves = _run(monkeypatch, case, loop, steps=6, split=(3, 3))
    _identical(halves, whole, f"{name} 3 + 3 vs 6")
    other = _run(monkeypatch, case, not loop, steps=6)
    _identical(whole, other, f"{name} 6 steps, loop vs chain")


def test_new_x0_between_two_rollouts(hip_lib, monkeypatch):
    """a caller's set_x0 between two loops starts the second from that x0, not from the plant state the first left"""
    case = _case("cartpole17")
    _env(monkeypatch, case, True, True)
    bs = _solver(case)
    bs.set_x0(case["x0"])
    bs.mpc_rollout(2)
    x_new = t.problems.cartpole_x0(B, seed=23)
    bs.set_x0(x_new)
    log = bs.mpc_rollout(1)
    u0 = log["u"][:, 0, :]
    want = case["prob"].A @ _f32(x_new) + case["prob"].B @ u0
    assert np.abs(log["x"][:, 0, :] - want).max() <= 1e-6 * np.abs(want).max()
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (e) switches off
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,want", [("cartpole17", "mpc_rollout: this problem shape / option set has no kernel with a fused closed loop"),
                                       ("quadrotor10_p2_generic", r"precision 2 has no fused closed loop \(step it from the host\)")])
@pytest.mark.parametrize("loop_alone", [False, True], ids=["none", "loop_alone"])
def test_switches_off(hip_lib, monkeypatch, name, want, loop_alone):
    """without TINYMPC_HIP_STREAM_MPC (TINYMPC_HIP_STREAM_LOOP alone has no effect) the two refusals are raised as before, and a
    plain solve follows"""
    case = _case(name)
    _env(monkeypatch, case, False, loop_alone)
    bs = _solver(case)
    bs.set_x0(case["x0"])
    with pytest.raises(t.TinyMPCError, match=want):
        bs.mpc_rollout(STEPS)
    assert _launches(bs) == -1
    assert bs.solve() in (0, 1)
    assert bs.kernel_name == case["name"] and np.isfinite(bs.get_solution()["controls"]).all()
    bs.close()


@pytest.mark.parametrize("what", ["adaptive", "cold", "per-instance+sequence", "families_p2"])
def test_refusals_that_stay(hip_lib, monkeypatch, what):
    """with both switches set: adaptive rho, a solver without the persistent workspace, per-instance references beside a
    sequence and families at precision 2 keep their messages"""
    case = _case("quadrotor7_sequence" if what == "per-instance+sequence" else ("cartpole_families" if what == "families_p2" else "cartpole17"))
    _env(monkeypatch, case, True, True)
    bs = _solver(case)
    bs.set_x0(case["x0"])
    if what == "adaptive":
        bs.set_adaptive_rho(True)
        want = "no kernel with a fused closed loop"
    elif what == "cold":
        bs.set_warm_start(False)
        want = r"needs the persistent workspace \(set_warm_start\(1\)\)"
    elif what == "per-instance+sequence":
        bs.set_x_ref(np.repeat(case["seq"][0][:, :, :1], B, axis=2))
        want = "cannot be combined with per-instance references"
    else:
        want = "precision 2 is not available on a per-instance-family solver"
    if what == "families_p2":
        with pytest.raises(t.TinyMPCError, match=want):
            bs.set_precision(2)
            bs.mpc_rollout(STEPS)
        bs.set_precision(0)
    else:
        with pytest.raises(t.TinyMPCError, match=want):
            bs.mpc_rollout(STEPS)
    assert bs.solve() in (0, 1)
    bs.close()
