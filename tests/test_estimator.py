"""Output feedback through a state estimator, CPU part: the entry points exist (declared in include/tinympc_hip.h, exported by the
built library, bound by the Python mirror, present in the Julia module) and refuse what needs no device to refuse;
tinympc_host_estimator_step — csrc/estimator.h compiled for the host, the text the device kernel compiles — against a numpy fp64
restatement of the rule written here; tinympc_host_kalman_gain against a numpy iteration of the same recursion.

The rule: y = C x + v; e = y - C xhat-; xhat = xhat- + L e; xhat-+ = f + A xhat + B u (the model's), row by row with one fma per
term in ascending order.

Bound of host_estimator_step against the restatement: 1e-12 max(1, scale), scale the largest magnitude among the step's inputs and
outputs times the largest row sum of the matrices involved — the two differ only in how a dot product of at most nx + nu + 1 <= 17
terms is rounded (fma chain against numpy's pairwise sums), a few 1e-16 of that scale.
Gain: the recursion's own residual at 1e-9 |P|, agreement with the numpy iteration at 1e-9, a stable A (I - L C).
Every test fails without the feature: neither the symbols nor the helpers exist there."""
import ctypes
import os
import re

import numpy as np
import pytest

import tinympc_julia_amd as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = ("tinympc_set_estimator", "tinympc_set_estimator_state", "tinympc_estimator_mode", "tinympc_estimator_outputs", "tinympc_get_estimator_state",
          "tinympc_get_mpc_estimate", "tinympc_get_mpc_outputs", "tinympc_host_estimator_step", "tinympc_host_kalman_gain")
GLOBAL = ("set_estimator", "set_estimator_state", "estimator_mode", "estimator_outputs", "get_estimator_state", "get_mpc_estimate", "get_mpc_outputs")
RULE_TOL = 1e-12
GAIN_TOL = 1e-9


# ---------------------------------------------------------------------------------------------------------------------------
# symbols
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_python_binds():
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    for sym in HANDLE + GLOBAL:
        assert re.search(r"\bint %s\(" % sym, header), sym
    from tinympc_julia_amd import tinympc
    for sym in HANDLE + GLOBAL:
        assert sym in tinympc.SIGNATURES, sym
    for name in ("set_estimator", "set_estimator_state", "estimator_mode", "get_estimator_state", "host_estimator_step", "kalman_gain"):
        assert hasattr(tinympc.BatchSolver, name), name
        assert callable(getattr(t, name)), name
    julia = open(os.path.join(ROOT, "tinympc-julia_amd", "julia", "TinyMPC.jl")).read()
    for name in ("set_estimator", "set_estimator_state", "estimator_mode", "get_estimator_state", "host_estimator_step", "kalman_gain"):
        assert "function %s(" % name in julia, name
    csrc = os.path.join(ROOT, "tinympc-julia_amd", "csrc")
    assert os.path.isfile(os.path.join(csrc, "estimator.h")) and "estimator_step_kernel" in open(os.path.join(csrc, "estimator.hip")).read()


def test_built_library_exports_and_refuses(hip_lib):
    raw = ctypes.CDLL(t.LIB_PATH)
    for sym in HANDLE + GLOBAL:
        assert hasattr(raw, sym), sym
        assert getattr(hip_lib, sym).restype is ctypes.c_int
    # without a solver the global forms fail cleanly
    hip_lib.cleanup_solver()
    assert hip_lib.estimator_mode() == -1 and hip_lib.set_estimator_state(None, 0, 0) == -1
    assert b"not initialized" in hip_lib.tinympc_last_error()
    # a null handle; the host exports' own argument checks
    assert hip_lib.tinympc_estimator_mode(None) == -1 and hip_lib.tinympc_set_estimator(None, None, 0, None, 0) == -1
    A, Bm, C, L = np.eye(4), np.ones((4, 1)), np.eye(4)[:2], np.zeros((4, 2))
    x = np.zeros(4)
    with pytest.raises(t.TinyMPCError, match="needs A, B and u"):
        t.host_estimator_step(x, C=C, L=L, x=x)
    with pytest.raises(t.TinyMPCError, match="needs C, L and the true state"):
        t.host_estimator_step(x, A=A, B=Bm, u=np.zeros(1))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))      # noqa: E731
    xh, y = np.zeros(4), np.zeros(4)
    for ny in (0, 5):
        assert hip_lib.tinympc_host_estimator_step(4, 1, ny, 0, 1, None, None, None, dp(np.zeros(20)), dp(np.zeros(20)), None, dp(x), None, dp(xh), dp(y)) == -1
        assert b"1 <= ny <= nx" in hip_lib.tinympc_last_error()
    assert hip_lib.tinympc_host_estimator_step(4, 1, 2, 0, 0, None, None, None, None, None, None, None, None, dp(xh), dp(y)) == -1
    with pytest.raises(t.TinyMPCError, match="expected A"):
        t.host_kalman_gain(np.eye(4), np.eye(3)[:2], np.eye(4), np.eye(2))
    with pytest.raises(t.TinyMPCError, match="pivot"):
        t.host_kalman_gain(np.eye(2), np.eye(2)[:1], np.eye(2), -np.eye(1) * 4.0)      # (C W C' + V = 1 - 4 < 0)


# ---------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------
def restated(xhat, A, Bm, f, u, C, L, x, v, predict, correct):
    xm = f + A @ xhat + Bm @ u if predict else xhat
    if not correct:
        return xm, None
    y = C @ x + (0.0 if v is None else v)
    return xm + L @ (y - C @ xm), y


@pytest.mark.parametrize("per_instance", [False, True], ids=["shared", "per_instance"])
@pytest.mark.parametrize("nx, ny", [(4, 2), (5, 1), (12, 6), (6, 6)])
def test_host_step_matches_the_restatement(hip_lib, nx, ny, per_instance):
    rng = np.random.default_rng(1000 * nx + ny + (7 if per_instance else 0))
    n, nu = 9, max(1, nx // 3)
    sh = (n,) if per_instance else ()
    A, Bm, f = rng.standard_normal((nx, nx) + sh), rng.standard_normal((nx, nu) + sh), rng.standard_normal((nx,) + sh)
    C, L = rng.standard_normal((ny, nx) + sh), 0.3 * rng.standard_normal((nx, ny) + sh)
    xhat, x, u, v = 3.0 * rng.standard_normal((nx, n)), 3.0 * rng.standard_normal((nx, n)), rng.standard_normal((nu, n)), 0.1 * rng.standard_normal((ny, n))
    pick = lambda M, b: M[..., b] if per_instance else M      # noqa: E731
    worst = 0.0
    for predict, correct in ((True, False), (False, True), (True, True)):
        for noise in ((v, None) if correct else (None,)):
            got_x, got_y = t.host_estimator_step(xhat, A=A, B=Bm, f=f, u=u, C=C, L=L, x=x, v=noise, predict=predict, correct=correct)
            assert got_x.shape == (nx, n) and (got_y is None) == (not correct)
            for b in range(n):
                Ab, Bb, fb, Cb, Lb = (pick(M, b) for M in (A, Bm, f, C, L))
                want_x, want_y = restated(xhat[:, b], Ab, Bb, fb, u[:, b], Cb, Lb, x[:, b], None if noise is None else noise[:, b], predict, correct)
                rows = max(np.abs(M).sum(axis=1).max() for M in (np.hstack([Ab, Bb]), Cb, Lb))
                mag = max(np.abs(q).max() for q in (xhat[:, b], x[:, b], u[:, b], fb, want_x))
                tol = RULE_TOL * max(1.0, rows * rows * mag)      # (L e: a row sum of L times a row sum of C times the states)
                err = np.abs(got_x[:, b] - want_x).max()
                if correct:
                    err = max(err, np.abs(got_y[:, b] - want_y).max())
                worst = max(worst, err / tol)
                assert err <= tol, (predict, correct, b, err, tol)
            # one instance alone, and the 1-D calling form
            one_x, one_y = t.host_estimator_step(xhat[:, 3], A=pick(A, 3), B=pick(Bm, 3), f=pick(f, 3), u=u[:, 3], C=pick(C, 3), L=pick(L, 3), x=x[:, 3],
                                                 v=None if noise is None else noise[:, 3], predict=predict, correct=correct)
            assert one_x.shape == (nx,) and np.array_equal(one_x, got_x[:, 3]) and (one_y is None or np.array_equal(one_y, got_y[:, 3]))
    print(f"nx = {nx}, ny = {ny}: host_estimator_step against the restatement, worst error / bound = {worst:.3e}")
    # predict then correct in two calls is the fused step, bit for bit; f = None is a zero affine term
    xm, _ = t.host_estimator_step(xhat, A=A, B=Bm, f=f, u=u, predict=True, correct=False)
    two, y2 = t.host_estimator_step(xm, C=C, L=L, x=x, v=v, predict=False, correct=True)
    both, y1 = t.host_estimator_step(xhat, A=A, B=Bm, f=f, u=u, C=C, L=L, x=x, v=v)
    assert np.array_equal(two, both) and np.array_equal(y1, y2)
    assert np.array_equal(t.host_estimator_step(xhat, A=A, B=Bm, u=u, correct=False)[0], t.host_estimator_step(xhat, A=A, B=Bm, f=np.zeros_like(f), u=u, correct=False)[0])


# ---------------------------------------------------------------------------------------------------------------------------
# the gain
# ---------------------------------------------------------------------------------------------------------------------------
def riccati_step(A, C, W, V, P):
    S = C @ P @ C.T + V
    return A @ (P - P @ C.T @ np.linalg.solve(S, C @ P)) @ A.T + W


def numpy_gain(A, C, W, V):
    P = W.copy()
    for _ in range(100000):
        Pn = riccati_step(A, C, W, V, P)
        Pn = 0.5 * (Pn + Pn.T)
        done = np.abs(Pn - P).sum(axis=1).max() <= 1e-13 * np.abs(Pn).sum(axis=1).max()
        P = Pn
        if done:
            break
    else:
        raise AssertionError("the numpy recursion did not converge")
    return P @ C.T @ np.linalg.inv(C @ P @ C.T + V), P


def _gain_case(work):
    if work == "cartpole":
        prob, rows = t.problems.cartpole(20, u_bound=0.5), [0, 2]      # cart position and pole angle
        scale = np.abs(t.problems.cartpole_x0(70, seed=7)).max(axis=1)
    else:
        prob, rows = t.problems.quadrotor(10), [0, 1, 2, 3, 4, 5]      # the six pose rows
        scale = np.abs(t.problems.quadrotor_x0(70, seed=5)).max(axis=1)
    C = np.eye(prob.nx)[rows]
    G = np.diag(0.003 * scale)
    return prob, C, G, G


@pytest.mark.parametrize("work", ["cartpole", "quadrotor"])
def test_kalman_gain(hip_lib, work):
    prob, C, Gw, Gv = _gain_case(work)
    ny = C.shape[0]
    W, V = Gw @ Gw.T, Gv[:ny] @ Gv[:ny].T
    L, P = t.host_kalman_gain(prob.A, C, W, V)
    assert L.shape == (prob.nx, ny) and P.shape == (prob.nx, prob.nx) and np.isfinite(L).all() and np.isfinite(P).all()
    norm = np.abs(P).sum(axis=1).max()
    res = np.abs(riccati_step(prob.A, C, W, V, P) - P).sum(axis=1).max()
    Ln, Pn = numpy_gain(prob.A, C, W, V)
    dP, dL = np.abs(P - Pn).max() / np.abs(Pn).max(), np.abs(L - Ln).max() / max(1.0, np.abs(Ln).max())
    rad = np.abs(np.linalg.eigvals(prob.A @ (np.eye(prob.nx) - L @ C))).max()
    print(f"{work}: Riccati residual {res / norm:.3e} |P|, against numpy P {dP:.3e} L {dL:.3e}, spectral radius of A (I - L C) {rad:.6f}")
    assert res <= GAIN_TOL * norm
    assert dP <= GAIN_TOL and dL <= GAIN_TOL
    assert rad < 1.0
    assert np.allclose(L, P @ C.T @ np.linalg.inv(C @ P @ C.T + V), rtol=0.0, atol=GAIN_TOL * max(1.0, np.abs(L).max()))
    assert np.array_equal(t.kalman_gain(prob.A, C, Gw, Gv), L)                      # W = Gw Gw', V = Gv[:ny] Gv[:ny]'
    assert np.array_equal(t.kalman_gain(prob.A, C, np.diagonal(Gw), np.diagonal(Gv)), L)      # (1-D: diag(sigma))


def test_undetectable_pair_is_refused(hip_lib):
    """an unstable mode (1.1) that C never reaches: the covariance of that mode grows without bound"""
    A = np.diag([0.9, 1.1, 0.5])
    A[0, 2] = 0.2
    C = np.array([[1.0, 0.0, 0.0]])
    with pytest.raises(t.TinyMPCError, match="not detectable"):
        t.host_kalman_gain(A, C, 0.01 * np.eye(3), 0.01 * np.eye(1))
    # the same A seen through the unstable row is fine
    L, _ = t.host_kalman_gain(A, np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]), 0.01 * np.eye(3), 0.01 * np.eye(2))
    assert np.abs(np.linalg.eigvals(A @ (np.eye(3) - L @ np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])))).max() < 1.0
