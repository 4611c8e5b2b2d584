"""Closed loops that follow a moving reference (set_ref_sequence + mpc_rollout) beyond the transposed-sets kernel:

 * inside the launch on the lanes-per-instance kernels (csrc/admm_quad.hip.h) at horizons up to 20: the step's shared
   references are re-staged in LDS before the step's first iteration — by every wavefront into its own image behind a
   wavefront-scope fence (22 G = 4 / G = 2 kernels whose state is all in registers: the cartpole G = 4 cases here), or by the
   workgroup into its one image between two barriers (every G = 1 kernel, and the kernels that keep state or coefficient
   rows in LDS: the G = 2, G = 1 and quadrotor cases here);
 * launch by launch on the chained loops (Solver::rollout_steps): the matrix-core kernel of the box-only shapes (mfma) and,
   behind TINYMPC_HIP_LEAN_WS=1, the lean kernel's workspace-keeping form — each launch reads its step's slice of the sequence.

The reference is the fp64 oracle stepped through the caller's loop on the host (set_x0 -> set_x_ref / set_u_ref of the step
-> solve -> x+ = A x + B u0: examples/cartpole_example_mpc.jl:35-51 with the reference shift of
examples/rocket_landing_constraints.jl:107-115), and the fixture G10 from the compiled reference itself.  The pattern is
tests/test_mfmat_gpu.py::test_mfmat_fused_rocket_loop_vs_oracle.  Every test here fails before the feature: mpc_rollout
raised "per-step references need the transposed-sets kernel (mfmat)".
"""
import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.test_ref_sequence import cartpole_tracking_refs, oracle_tracking_loop, quadrotor_tracking_refs
from tests.util import FP32_TOL, cm, load_golden, nrel, problem_of

pytestmark = pytest.mark.gpu

FIXED = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=12, check_termination=1)
TOL30 = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=30, check_termination=1)
TOL10 = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=10, check_termination=1)
X_NEAR, X_FAR = np.array([0.1, 0.0, 0.0, 0.0]), np.array([0.3, 0.0, 0.05, 0.0])   # (G10's x0 is the far one)


def _solver(prob, B, kw, xs=None, us=None, seq=True):
    """a warm-started solver of the family; with xs / us: the sequence (seq) or step 0's references alone"""
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    bs.update_settings(**kw)
    if prob.has_bounds():
        bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if xs is not None and seq:
        bs.set_ref_sequence(xs, us)
    elif xs is not None:
        bs.set_x_ref(xs[:, :, 0])
        bs.set_u_ref(us[:, :, 0])
    return bs


def _rel(a, ref):
    """per-instance norm-relative error of (rows, steps, B) logs"""
    den = np.abs(ref).max(axis=(0, 1))
    return np.abs(a - ref).max(axis=(0, 1)) / np.where(den == 0.0, 1.0, den)


_ORACLE_CACHE = {}


def _oracle_loops(oracle, key, prob, kw, x0, xs, us, steps):
    """the fp64 oracle's loops of a batch, computed once per test session and left unchanged (key names the case)"""
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = [oracle_tracking_loop(oracle, "orc64", prob, kw, x0[:, b], xs, us, steps) for b in range(x0.shape[1])]
    return _ORACLE_CACHE[key]


def _stack(loops, key):
    return np.stack([r[key] for r in loops], axis=-1)


def _check_vs_oracle(oracle, key, prob, kw, x0, xs, us, steps, bs, log, min_same, tag):
    """EVERY instance against the oracle's loop at FP32_TOL: applied controls, plant states and the last solve.  Instances
    whose (iteration count, solved flag) differ from the oracle's at some step are not dropped: the oracle's loop is replayed
    with the GPU's termination decisions imposed (CpuSolver.set_forced_exit).  min_same: the share that must agree without
    replay (None: all — fixed iterations have no termination decisions); no count may differ by more than 1."""
    loops = list(_oracle_loops(oracle, key, prob, kw, x0, xs, us, steps))
    B = x0.shape[1]
    it, so = _stack(loops, "iter"), _stack(loops, "solved")
    same = np.all((log["iter"] == it) & (log["solved"] == so), axis=0)
    print(f"{tag}: {int(same.sum())} of {B} closed loops took the oracle's own iteration counts")
    assert same.mean() >= (1.0 if min_same is None else min_same), f"{tag}: {same.mean():.3f}"
    for b in np.nonzero(~same)[0]:
        assert np.abs(log["iter"][:, b] - it[:, b]).max() <= 1, f"{tag}: instance {b}"
        loops[b] = oracle_tracking_loop(oracle, "orc64", prob, kw, x0[:, b], xs, us, steps,
                                        forced=[(log["iter"][k, b], log["solved"][k, b]) for k in range(steps)])
        assert np.array_equal(loops[b]["iter"], log["iter"][:, b]) and np.array_equal(loops[b]["solved"], log["solved"][:, b])
    eu, ex = _rel(log["u"], _stack(loops, "u")), _rel(log["x"], _stack(loops, "x"))
    print(f"{tag}: worst applied control {eu.max():.3e}, worst plant state {ex.max():.3e}")
    assert eu.max() <= FP32_TOL, f"{tag}: applied controls, worst {eu.max():.3e} (instance {eu.argmax()})"
    assert ex.max() <= FP32_TOL, f"{tag}: plant states, worst {ex.max():.3e} (instance {ex.argmax()})"
    sol = bs.get_solution()                                    # the last solve is what get_solution describes
    for b in range(B):
        assert nrel(sol["states"][:, :, b], loops[b]["last_x"]) <= FP32_TOL, f"{tag}: last solve's states, instance {b}"
        assert nrel(sol["controls"][:, :, b], loops[b]["last_u"]) <= FP32_TOL, f"{tag}: last solve's controls, instance {b}"
    return same.mean()


def _host_stepped(bs, prob, x0, xs, us, steps):
    """the loop a caller without the fused entry point runs: set_x_ref, set_u_ref, set_x0, solve per step"""
    x = x0.copy()
    u, it = np.zeros((prob.nu, steps, x0.shape[1])), np.zeros((steps, x0.shape[1]), dtype=int)
    for k in range(steps):
        bs.set_x_ref(xs[:, :, k])
        bs.set_u_ref(us[:, :, k])
        bs.set_x0(x)
        bs.solve()
        u[:, k, :] = bs.get_solution()["controls"][:, 0, :]
        it[k] = bs.get_status()["iter"]
        x = prob.A @ x + prob.B @ u[:, k, :]
    return u, it


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the fixture from the compiled reference, on the quad kernel
# ---------------------------------------------------------------------------------------------------------------------------
def test_g10_tracking_loop_on_the_quad_kernel(hip_lib):
    """G10 (the reference's own loop with a reference that moves every step), batch 1, fused with the sequence: iteration
    count and solved flag of every step equal the fixture's, applied control and plant state within FP32_TOL"""
    g = load_golden("G10_cartpole_tracking_loop")
    prob = problem_of(g)
    steps = len(g["steps"])
    xs = np.asarray(g["x_ref_seq"]).reshape((prob.nx, prob.N, steps), order="F")
    us = np.asarray(g["u_ref_seq"]).reshape((prob.nu, prob.N - 1, steps), order="F")
    bs = _solver(prob, 1, g["settings"], xs, us)
    bs.set_x0(np.array(g["x0"]))
    log = bs.mpc_rollout(steps)
    assert bs.kernel_name.startswith("quad<4,1,10") and bs.last_launch_name == bs.kernel_name, bs.kernel_name
    assert log["status"] == g["steps"][-1]["status"]
    for k, step in enumerate(g["steps"]):
        u_all = np.array(step["u"])
        eu = np.abs(log["u"][:, k, 0] - u_all[: prob.nu]).max() / max(1.0, np.abs(u_all).max())
        print(f"step {k}: iter {int(log['iter'][k, 0])} ({step['iter']}), solved {int(log['solved'][k, 0])} ({step['solved']}), control off by {eu:.3e}")
        assert int(log["iter"][k, 0]) == step["iter"], f"step {k}"
        assert int(log["solved"][k, 0]) == step["solved"], f"step {k}"
        assert eu <= FP32_TOL, f"step {k}: applied control off by {eu:.3e}"
        if k + 1 < steps:
            xn = np.array(g["steps"][k + 1]["x0"])
            ex = np.abs(log["x"][:, k, 0] - xn).max() / max(1.0, np.abs(xn).max())
            assert ex <= FP32_TOL, f"step {k}: plant state off by {ex:.3e}"
    sol = bs.get_solution()
    last = g["steps"][-1]
    assert nrel(sol["states"][:, :, 0], cm(last["x"], prob.nx, prob.N)) <= FP32_TOL
    assert nrel(sol["controls"][:, :, 0], cm(last["u"], prob.nu, prob.N - 1)) <= FP32_TOL
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. quad kernel, every lane grouping
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [4, 2, 1])
def test_quad_every_lane_grouping(hip_lib, oracle_built, monkeypatch, group):
    """cartpole N = 10, batch 150 (G = 4: two full workgroups and a ragged one), 8 steps, the reference moves every step, the
    input bound is active, fixed iterations: every instance against the oracle's loop; a sequence that repeats step 0's
    references is bit-equal to no sequence; the host-stepped loop on the same kernel agrees within FP32_TOL"""
    monkeypatch.setenv("TINYMPC_HIP_GROUP", str(group))
    N, B, steps = 10, 150, 8
    prob = t.problems.cartpole(N, u_bound=0.5)
    x0 = t.problems.cartpole_x0(B, seed=7)
    xs, us = cartpole_tracking_refs(N, steps)
    name = f"quad<4,1,10,g{group}>"
    bs = _solver(prob, B, FIXED, xs, us)
    bs.set_x0(x0)
    log = bs.mpc_rollout(steps)
    assert bs.kernel_name == name and bs.last_launch_name == name, (bs.kernel_name, bs.last_launch_name)
    assert np.all(log["iter"] == FIXED["max_iter"]) and not log["solved"].any()
    assert (np.abs(np.abs(log["u"]) - 0.5) < 1e-7).mean() > 0.1, "the input bound is not active"
    _check_vs_oracle(oracle_built, "cartpole10", prob, FIXED, x0, xs, us, steps, bs, log, None, name)
    # (a) the same references at every step: the loop with no sequence, bit for bit
    xc, uc = np.repeat(xs[:, :, :1], steps, axis=2), np.repeat(us[:, :, :1], steps, axis=2)
    runs = []
    for seq in (True, False):
        b2 = _solver(prob, B, FIXED, xc, uc, seq=seq)
        b2.set_x0(x0)
        runs.append((b2.mpc_rollout(steps), b2.get_solution()))
        assert b2.last_launch_name == name
        b2.close()
    for key in ("u", "x", "iter", "solved"):
        assert np.array_equal(runs[0][0][key], runs[1][0][key]), f"constant sequence vs no sequence: {key}"
    for key in ("states", "controls"):
        assert np.array_equal(runs[0][1][key], runs[1][1][key]), f"constant sequence vs no sequence: {key}"
    assert not np.array_equal(runs[0][0]["u"], log["u"])       # (and the moving reference does change the loop)
    # (b) the host-stepped loop on the same kernel (it rounds the plant state to fp32 every step)
    b3 = _solver(prob, B, FIXED)
    u3, it3 = _host_stepped(b3, prob, x0, xs, us, steps)
    assert b3.last_launch_name == name and np.array_equal(it3, log["iter"])
    e3 = _rel(u3, log["u"])
    print(f"{name}: host-stepped loop vs fused loop {e3.max():.3e}")
    assert e3.max() <= FP32_TOL, f"host-stepped loop vs fused loop: {e3.max():.3e}"
    bs.close(); b3.close()


def test_quad_quadrotor_lds_state(hip_lib, oracle_built, monkeypatch):
    """quad<12,4,20,g4> — trajectories and coefficient rows in LDS, four lanes per instance, nu > 1 — quadrotor N = 20, batch 24,
    5 steps, position references moving every step, fixed iterations.
    The shape's closed loop runs on the matrix-core chain by default, and mpc_rollout refuses a solver without the persistent
    workspace (set_warm_start(0): "mpc_rollout needs the persistent workspace"), so the kernel is reached the way the suite
    holds the family on it elsewhere: TINYMPC_HIP_GROUP=4."""
    monkeypatch.setenv("TINYMPC_HIP_GROUP", "4")
    N, B, steps = 20, 24, 5
    prob = t.problems.quadrotor(N)
    x0 = t.problems.quadrotor_x0(B, seed=11)
    xs, us = quadrotor_tracking_refs(N, steps)
    bs = _solver(prob, B, FIXED, xs, us)
    bs.set_x0(x0)
    log = bs.mpc_rollout(steps)
    assert bs.kernel_name == "quad<12,4,20,g4>" and bs.last_launch_name == "quad<12,4,20,g4>", bs.kernel_name
    _check_vs_oracle(oracle_built, "quadrotor20", prob, FIXED, x0, xs, us, steps, bs, log, None, "quad<12,4,20,g4>")
    bc = _solver(prob, B, FIXED, xs, us)
    bc.set_warm_start(0)
    bc.set_x0(x0)
    with pytest.raises(t.TinyMPCError, match="persistent workspace"):
        bc.mpc_rollout(steps)
    bs.close(); bc.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. wavefronts of one workgroup at different steps
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [4, 1])
def test_wavefronts_at_different_steps(hip_lib, oracle_built, monkeypatch, group):
    """Tolerance-terminated instances leave the iteration loop at different iterations, so the wavefronts of a workgroup
    reach a step at different times.  Two x0, one near the reference and one far, wavefront by wavefront (wavefront w of
    every workgroup gets x0 number w mod 2), three workgroups and a ragged fourth: every instance must be bit-equal to the
    same x0 in a uniform batch of the same size.  A reference image shared between wavefronts, or a barrier that couples
    them wrongly, shows here."""
    monkeypatch.setenv("TINYMPC_HIP_GROUP", str(group))
    N, steps = 10, 12
    per_wave = 64 // group
    B = 3 * 4 * per_wave + per_wave + 3
    prob = t.problems.cartpole(N, u_bound=0.5)
    xs, us = cartpole_tracking_refs(N, steps)
    near = oracle_tracking_loop(oracle_built, "orc64", prob, TOL30, X_NEAR, xs, us, steps)
    far = oracle_tracking_loop(oracle_built, "orc64", prob, TOL30, X_FAR, xs, us, steps)
    assert np.abs(near["iter"] - far["iter"]).max() >= 5, (near["iter"], far["iter"])
    which = (np.arange(B) // per_wave) % 4 % 2                  # wavefront w of its workgroup: x0 number w mod 2
    x_pair = np.stack([X_NEAR, X_FAR], axis=1)
    out = {}
    for tag, x0 in (("mixed", x_pair[:, which]), ("near", np.repeat(x_pair[:, :1], B, axis=1)), ("far", np.repeat(x_pair[:, 1:], B, axis=1))):
        bs = _solver(prob, B, TOL30, xs, us)
        bs.set_x0(x0)
        log = bs.mpc_rollout(steps)
        assert bs.last_launch_name == f"quad<4,1,10,g{group}>", bs.last_launch_name
        out[tag] = dict(log, **bs.get_solution())
        bs.close()
    assert np.abs(out["near"]["iter"][:, 0] - out["far"]["iter"][:, 0]).max() >= 5      # ... on the GPU as on the oracle
    for key in ("u", "x", "iter", "solved", "states", "controls"):
        want = np.where(which == 0, out["near"][key], out["far"][key])
        assert np.array_equal(out["mixed"][key], want), f"{key}: a wavefront's loop depends on its neighbours'"
    # and the uniform batches are the oracle's loops (G10's x0 is the far one)
    for tag, ref in (("near", near), ("far", far)):
        assert np.array_equal(out[tag]["iter"][:, 0], ref["iter"]) and np.array_equal(out[tag]["solved"][:, 0], ref["solved"]), tag
        assert np.abs(out[tag]["u"][:, :, 0] - ref["u"]).max() <= FP32_TOL * np.abs(ref["u"]).max(), tag


# ---------------------------------------------------------------------------------------------------------------------------
# 5. many workgroups
# ---------------------------------------------------------------------------------------------------------------------------
def test_many_workgroups_identical_instances(hip_lib, oracle_built, monkeypatch):
    """identical x0 in 1 000 instances (G = 4: 16 workgroups, the last one ragged), 6 steps, fixed iterations: every
    instance bit-equal to instance 0, instance 0 the oracle's loop"""
    monkeypatch.setenv("TINYMPC_HIP_GROUP", "4")
    N, B, steps = 10, 1000, 6
    prob = t.problems.cartpole(N, u_bound=0.5)
    xs, us = cartpole_tracking_refs(N, steps)
    x0 = np.repeat(X_FAR[:, None], B, axis=1)
    bs = _solver(prob, B, FIXED, xs, us)
    bs.set_x0(x0)
    log = bs.mpc_rollout(steps)
    sol = bs.get_solution()
    assert bs.last_launch_name == "quad<4,1,10,g4>"
    for key, a in (("u", log["u"]), ("x", log["x"]), ("states", sol["states"]), ("controls", sol["controls"])):
        assert np.array_equal(a, np.repeat(a[:, :, :1], B, axis=2)), f"{key}: instances differ between workgroups"
    ref = oracle_tracking_loop(oracle_built, "orc64", prob, FIXED, X_FAR, xs, us, steps)
    assert np.abs(log["u"][:, :, 0] - ref["u"]).max() <= FP32_TOL * np.abs(ref["u"]).max()
    assert np.abs(log["x"][:, :, 0] - ref["x"]).max() <= FP32_TOL * np.abs(ref["x"]).max()
    assert nrel(sol["states"][:, :, 0], ref["last_x"]) <= FP32_TOL and nrel(sol["controls"][:, :, 0], ref["last_u"]) <= FP32_TOL
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the chain on the matrix-core kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _orc32_share(oracle, key, prob, kw, x0, xs, us, steps):
    """share of the batch on which an all-fp32 oracle loop takes the fp64 oracle's (iteration count, solved flag) at every
    step: how well conditioned the case's termination decisions are (orc32 is a harsher proxy than the kernels' arithmetic)"""
    r64 = _oracle_loops(oracle, key, prob, kw, x0, xs, us, steps)
    n = 0
    for b in range(x0.shape[1]):
        r32 = oracle_tracking_loop(oracle, "orc32", prob, kw, x0[:, b], xs, us, steps)
        n += np.array_equal(r32["iter"], r64[b]["iter"]) and np.array_equal(r32["solved"], r64[b]["solved"])
    return n / x0.shape[1]


@pytest.mark.parametrize("setting", ["fixed", "tol"])
def test_chain_on_mfma(hip_lib, oracle_built, setting):
    """quadrotor N = 10, batch 40 (two and a half 16-instance tiles), 8 steps, position references moving every step: the
    stream-ordered chain of mfma launches and plant updates, each launch on its step's slice of the sequence.  Compared as
    test_fused_mpc_rollout_batch_vs_oracle compares; at least 0.85 of the instances agree with the oracle's iteration counts
    without replay and none differs by more than 1 (the rocket-loop test's limits).
    The case is chosen so that its termination decisions are not marginal: an all-fp32 oracle loop (orc32) takes the fp64
    oracle's iteration counts at every step on 40 of the 40 instances (share 1.0; required here: >= 0.95)."""
    N, B, steps = 10, 40, 8
    prob = t.problems.quadrotor(N)
    x0 = t.problems.quadrotor_x0(B, seed=5)
    xs, us = quadrotor_tracking_refs(N, steps)
    kw = dict(FIXED, max_iter=10) if setting == "fixed" else TOL10
    key = "quadrotor10-" + setting
    if setting == "tol":
        share = _orc32_share(oracle_built, key, prob, kw, x0, xs, us, steps)
        print(f"orc32 agrees with orc64 on the iteration counts of {share:.3f} of the instances")
        assert share >= 0.95
    bs = _solver(prob, B, kw, xs, us)
    bs.set_x0(x0)
    log = bs.mpc_rollout(steps)
    assert bs.kernel_name.startswith("mfma<12,4,10") and bs.last_launch_name.startswith("mfma<12,4,10"), bs.kernel_name
    _check_vs_oracle(oracle_built, key, prob, kw, x0, xs, us, steps, bs, log, None if setting == "fixed" else 0.85, "mfma " + setting)
    if setting == "tol":
        assert len(np.unique(log["iter"])) > 2, "every step of every instance stopped at the same iteration"
    # step 0's references are the solver's own afterwards: a plain solve runs on them
    bs.set_x0(x0)
    bs.solve()
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the chain on the lean kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["fixed", "tol", "tol-state-bound"])
def test_chain_on_lean(hip_lib, oracle_built, monkeypatch, setting):
    """TINYMPC_HIP_LEAN_WS=1, one lane per instance, cartpole N = 20, batch 130 (ragged third wavefront), 8 steps: the chain of
    workspace-keeping lean launches, each forming its scaled reference terms from its step's slice of the sequence — fixed
    iterations, tolerance-terminated, and with a finite state bound (the XB + shared-references variant).  Compared as the
    mfma chain is."""
    monkeypatch.setenv("TINYMPC_HIP_LEAN_WS", "1")
    monkeypatch.setenv("TINYMPC_HIP_GROUP", "1")
    N, B, steps = 20, 130, 8
    prob = t.problems.cartpole(N, u_bound=0.5)
    if setting == "tol-state-bound":
        prob.x_min, prob.x_max = prob.x_min.copy(), prob.x_max.copy()
        prob.x_min[0, :], prob.x_max[0, :] = -0.3, 0.3
    x0 = t.problems.cartpole_x0(B, seed=17)
    xs, us = cartpole_tracking_refs(N, steps)
    kw = dict(FIXED, max_iter=10) if setting == "fixed" else TOL10
    bs = _solver(prob, B, kw, xs, us)
    bs.set_x0(x0)
    log = bs.mpc_rollout(steps)
    assert bs.kernel_name == "quad<4,1,20,g1>" and bs.last_launch_name.startswith("lean<4,1,20"), (bs.kernel_name, bs.last_launch_name)
    _check_vs_oracle(oracle_built, "cartpole20-" + setting, prob, kw, x0, xs, us, steps, bs, log, None if setting == "fixed" else 0.85,
                     "lean " + setting)
    if setting == "tol-state-bound":
        assert np.abs(bs.get_workspace()["g"]).max() > 1e-4, "the state bound never acted"
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["short", "per-instance", "adaptive", "precision2", "long-horizon"])
def test_refusals_name_the_condition(hip_lib, case):
    """what no route offers raises TinyMPCError with a message that names the condition, and leaves the solver usable: a
    plain solve follows"""
    N, B, steps = (30 if case == "long-horizon" else 10), 8, 4
    prob = t.problems.cartpole(N, u_bound=0.5)
    xs, us = cartpole_tracking_refs(N, steps)
    bs = _solver(prob, B, TOL10, xs, us)
    bs.set_x0(t.problems.cartpole_x0(B, seed=3))
    if case == "short":
        want, n = "sequence holds 4 steps, the loop asks for 5", steps + 1
    elif case == "per-instance":
        bs.set_x_ref(np.repeat(xs[:, :, :1], B, axis=2))         # (nx, N, B): one reference per instance
        want, n = "per-instance", steps
    elif case == "adaptive":
        bs.set_adaptive_rho(True)
        want, n = "adaptive rho", steps
    elif case == "precision2":
        bs.set_precision(2)
        want, n = "precision 2", steps
    else:                                                        # quad<4,1,30,g4>: compiled as without the feature (it is at the register limit)
        want, n = "horizons up to 20", steps
    with pytest.raises(t.TinyMPCError, match=want):
        bs.mpc_rollout(n)
    assert bs.solve() in (0, 1)
    assert np.isfinite(bs.get_solution()["controls"]).all()
    bs.close()
