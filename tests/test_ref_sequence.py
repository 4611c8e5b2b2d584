"""Closed loops that follow a moving reference, CPU part: the fp64 oracle restatement stepped through the loop of the fixture
G10 (scripts/make_golden_tracking.py: the compiled reference driven through examples/cartpole_example_mpc.jl:35-51 with
set_x_ref / set_u_ref of a moving reference before every solve) reproduces it at the bar of tests/test_oracle.py — and the
helpers the GPU part (tests/test_ref_sequence_gpu.py) shares: the reference sequences and the oracle's loop.
"""
import numpy as np

from tests.util import FP64_TOL, cm, load_golden, nrel, problem_of


def cartpole_tracking_refs(N, steps, ramp=0.005):
    """x_ref_seq (4, N, steps), u_ref_seq (1, N-1, steps) as G10 has them: knot i of step k (0-based) asks for the cart at
    ramp (i + k) and for a small input that fades along the same ramp"""
    xs, us = np.zeros((4, N, steps)), np.zeros((1, N - 1, steps))
    ik = np.arange(N)[:, None] + np.arange(steps)[None, :]
    xs[0] = ramp * ik
    us[0] = 0.05 - 0.002 * ik[: N - 1]
    return xs, us


def quadrotor_tracking_refs(N, steps, ramp=0.002):
    """(12, N, steps), (4, N-1, steps): the position reference on a ramp in i + k — x forward, y at half the rate, z up at a
    quarter — with the matching constant velocity reference; inputs at zero"""
    xs, us = np.zeros((12, N, steps)), np.zeros((4, N - 1, steps))
    ik = np.arange(N)[:, None] + np.arange(steps)[None, :]
    for row, rate in ((0, 1.0), (1, 0.5), (2, 0.25)):
        xs[row] = ramp * rate * ik
        xs[6 + row] = ramp * rate / 0.05                      # (the model's step is 0.05 s)
    return xs, us


def oracle_tracking_loop(oracle, kind, prob, kw, x0, xs, us, steps, forced=None):
    """the caller's loop on a CPU oracle: set_x0 -> set_x_ref / set_u_ref of the step -> solve -> x+ = A x + B u0.
    forced = [(iter, solved)] per step imposes termination decisions (CpuSolver.set_forced_exit).
    Returns u (nu, steps) applied, x (nx, steps) plant state after each step, iter, solved (steps,) and the last solve's
    trajectories last_x, last_u."""
    o = oracle.CpuSolver(kind, prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
    o.update_settings(**kw)
    if prob.has_bounds():
        o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    x = np.array(x0, dtype=np.float64)
    u_log, x_log = np.zeros((prob.nu, steps)), np.zeros((prob.nx, steps))
    it, so = np.zeros(steps, dtype=int), np.zeros(steps, dtype=int)
    r = None
    for k in range(steps):
        if forced is not None:
            o.set_forced_exit(int(forced[k][0]) if forced[k][1] else -1)
        o.set_x0(x)
        o.set_x_ref(xs[:, :, k])
        o.set_u_ref(us[:, :, k])
        o.solve()
        r = o.get_solution()
        x = prob.A @ x + prob.B @ r["u"][:, 0]
        u_log[:, k], x_log[:, k], it[k], so[k] = r["u"][:, 0], x, r["iter"], r["solved"]
    o.close()
    return dict(u=u_log, x=x_log, iter=it, solved=so, last_x=np.array(r["x"]), last_u=np.array(r["u"]))


def test_orc64_reproduces_the_tracking_fixture(oracle_built):
    """G10, step by step: plant state, iteration count, solved flag and status exactly, trajectories to 1e-12"""
    g = load_golden("G10_cartpole_tracking_loop")
    prob = problem_of(g)
    steps = len(g["steps"])
    assert (prob.N, steps) == (10, 12) and g["settings"] == dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=30, check_termination=1)
    xs = np.asarray(g["x_ref_seq"]).reshape((prob.nx, prob.N, steps), order="F")
    us = np.asarray(g["u_ref_seq"]).reshape((prob.nu, prob.N - 1, steps), order="F")
    assert np.array_equal(xs, cartpole_tracking_refs(prob.N, steps)[0]) and np.array_equal(us, cartpole_tracking_refs(prob.N, steps)[1])
    assert all(np.any(xs[:, :, k] != xs[:, :, k - 1]) for k in range(1, steps)), "the reference does not move every step"
    s = oracle_built.CpuSolver("orc64", prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
    s.update_settings(**g["settings"])
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    x = np.array(g["x0"], dtype=np.float64)
    on_bound = 0
    for k, step in enumerate(g["steps"]):
        assert np.abs(x - np.array(step["x0"])).max() <= 1e-12, f"step {k}"
        s.set_x0(x)
        s.set_x_ref(xs[:, :, k])
        s.set_u_ref(us[:, :, k])
        status = s.solve()
        o = s.get_solution()
        assert (status, o["iter"], o["solved"]) == (step["status"], step["iter"], step["solved"]), f"step {k}"
        assert nrel(o["x"], cm(step["x"], prob.nx, prob.N)) <= FP64_TOL, f"step {k}"
        assert nrel(o["u"], cm(step["u"], prob.nu, prob.N - 1)) <= FP64_TOL, f"step {k}"
        on_bound += abs(abs(o["u"][0, 0]) - prob.u_max[0, 0]) < 1e-12
        x = prob.A @ x + prob.B @ o["u"][:, 0]
    s.close()
    its = [step["iter"] for step in g["steps"]]
    assert on_bound >= 3 and len(set(its)) >= 4, "the fixture is meant to hold an active input bound and early exits at different iterations"
    # the shared helper is the same loop
    r = oracle_tracking_loop(oracle_built, "orc64", prob, g["settings"], g["x0"], xs, us, steps)
    assert list(r["iter"]) == its and np.abs(r["u"][0] - np.array([st["u"][0] for st in g["steps"]])).max() <= 1e-12
