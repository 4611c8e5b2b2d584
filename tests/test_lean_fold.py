"""CPU tests of the scaled sparse form with C folded into the costate's scale (csrc/admm_lean.hip.h: FOLD; csrc/admm_params.h:
lean_cost_folded; csrc/kernels.hip: lean_scaled_block), reached through the library's test hooks tmpc_lean_folded_cost and
tmpc_lean_scaled_block, which include/tinympc_hip.h does not declare.

With one input C = -rho Quu_inv is a nonzero scalar c.  The scaled recursion carries pv = c p^ instead of p^ = S^-1 p~:
d_k = c r~_k + B^' pv_{k+1}, pv_k = Wv x^_k + A^' pv_{k+1} - K^' d_k, pv_{N-1} = Wv x^_{N-1} with Wv = c S^-2 — the product
d = C t, the one chain of the iteration without a free start, goes: cartpole 24 fp64 per knot for 25.  The pack keeps its
layout; only its w entries change.  The algebra is settled by a numpy replica of the folded sweeps against the unfolded scaled
replica of tests/test_lean_scaled.py (fp64 sweeps, fp32 slack and dual): d, u and x^ are the same numbers up to fp64 rounding,
so the two are held to the tolerance that test holds scaled against unscaled to (1e-12 on trajectories of order 1; the random
models' trajectories are held to it relative to their own magnitude where that exceeds 1)."""
import ctypes

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.test_lean_scaled import _replica
from tests.test_lean_scaled import hooks  # noqa: F401  (the module's fixture of the scaled form's hooks)


@pytest.fixture(scope="module")
def fold(hip_lib):
    lib = ctypes.CDLL(t.LIB_PATH)
    dp, u64 = ctypes.POINTER(ctypes.c_double), ctypes.c_ulonglong
    lib.tmpc_lean_folded_cost.restype = ctypes.c_int
    lib.tmpc_lean_folded_cost.argtypes = [ctypes.c_int, ctypes.c_int, u64]
    lib.tmpc_lean_scaled_block.restype = ctypes.c_int
    lib.tmpc_lean_scaled_block.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp, dp, dp, u64, dp, ctypes.c_int]

    class F:
        cost = staticmethod(lambda nx, nu, sz: lib.tmpc_lean_folded_cost(nx, nu, sz))

        @staticmethod
        def block(A, B, K, C, built=0):
            """the pack's scaled block of the row-major model as (A^, K^, B^, C, w), or None where the model keeps the
            unscaled sweeps"""
            A, B, K, C = (np.ascontiguousarray(m, dtype=np.float64) for m in (A, B, K, C))
            nx, nu = B.shape
            n = nx * nx + 2 * nu * nx + nu * nu + nx
            out = np.zeros(n)
            got = lib.tmpc_lean_scaled_block(nx, nu, A.ctypes.data_as(dp), B.ctypes.data_as(dp), K.ctypes.data_as(dp),
                                             C.ctypes.data_as(dp), built, out.ctypes.data_as(dp), n)
            assert got in (0, n)
            if not got:
                return None
            cut = np.cumsum([nx * nx, nu * nx, nx * nu, nu * nu])
            a, k, b, c, w = np.split(out, cut)
            return a.reshape(nx, nx), k.reshape(nu, nx), b.reshape(nx, nu), c.reshape(nu, nu), w
    return F


def _cartpole(u_bound=0.5):
    prob = t.problems.cartpole(20, u_bound=u_bound)
    c = t.host_precompute(prob.A, prob.B, prob.Q, prob.R, prob.rho)
    K, C = np.array(c["Kinf"], dtype=np.float64), -prob.rho * np.array(c["Quu_inv"], dtype=np.float64)
    return prob, np.asarray(prob.A, dtype=np.float64), np.asarray(prob.B, dtype=np.float64), K, C


def test_folded_cost(hooks, fold):  # noqa: F811
    p = t.problems.cartpole(20)
    sp = hooks.pattern(p.A, p.B)
    sz = hooks.scaled_pattern(4, 1, sp)
    assert fold.cost(4, 1, sz) == 24
    assert hooks.scaled_cost(4, 1, sz) == 25 and hooks.sparse_cost(4, 1, sp) == 27      # neither has moved
    assert fold.cost(4, 1, sp) == -1                                                   # (not a scaled pattern)
    # more than one input: C is a matrix, nothing folds
    rng = np.random.default_rng(7)
    A2, B2 = np.triu(rng.standard_normal((3, 3))), rng.standard_normal((3, 2))
    sz2 = hooks.scaled_pattern(3, 2, hooks.pattern(A2, B2))
    assert sz2 and fold.cost(3, 2, sz2) == hooks.scaled_cost(3, 2, sz2)


def test_packed_block(hooks, fold):  # noqa: F811
    prob, A, B, K, C = _cartpole()
    sz, s, Ah, Bh = hooks.scale(A, B)
    assert sz
    blk = fold.block(A, B, K, C)
    assert blk is not None
    a, k, b, c, w = blk
    # A^ = S A S^-1, B^ = S B (units exact), K^ = Kinf S^-1 and C: what the block held before the fold
    assert np.array_equal(a, Ah) and np.array_equal(b, Bh)
    assert np.array_equal(k, K / s[None, :]) and np.array_equal(c, C)
    assert a[0, 1] == 1.0 and a[1, 2] == 1.0 and a[2, 3] == 1.0 and b[3, 0] == 1.0
    want = C[0, 0] / (s * s)
    assert C[0, 0] != 0.0 and np.all(np.abs(w - want) <= 2 * np.spacing(np.abs(want)))
    # two inputs: w stays S^-2
    rng = np.random.default_rng(11)
    for _ in range(50):
        A2 = rng.standard_normal((3, 3)) * (rng.random((3, 3)) < 0.6)
        B2 = rng.standard_normal((3, 2)) * (rng.random((3, 2)) < 0.6)
        sz2, s2, _, _ = hooks.scale(A2, B2)
        if sz2:
            break
    assert sz2
    K2, C2 = rng.standard_normal((2, 3)), rng.standard_normal((2, 2))
    w2 = fold.block(A2, B2, K2, C2)[4]
    assert np.all(np.abs(w2 - 1.0 / (s2 * s2)) <= 2 * np.spacing(1.0 / (s2 * s2)))


# ---- the algebra: the folded sweeps beside tests/test_lean_scaled.py's _replica ----
def _replica_folded(A, B, K, c, wv, s, x0, lo, hi, iters, N):
    """_replica with the costate carried as pv = c p^: d = c r~ + B' pv, pv = Wv x^ + A' pv - K' d, pv_{N-1} = Wv x^_{N-1}
    (nu = 1, c the scalar C, wv = c / s^2)"""
    nx, nu = B.shape
    assert nu == 1
    nb = x0.shape[1]
    X = np.zeros((N, nx, nb))
    X[0] = s[:, None] * x0.astype(np.float32).astype(np.float64)
    Y, Z = np.zeros((N - 1, nu, nb), np.float32), np.zeros((N - 1, nu, nb), np.float32)
    D = np.zeros((N - 1, nu, nb))
    lo, hi = np.float32(lo)[:, None], np.float32(hi)[:, None]
    for _ in range(iters):
        for k in range(N - 1):
            u = -(K @ X[k]) - D[k]
            X[k + 1] = A @ X[k] + B @ u
            tt = u.astype(np.float32) + Y[k]
            zn = np.minimum(np.maximum(tt, lo), hi)
            Y[k], Z[k] = tt - zn, zn
        p = wv[:, None] * X[N - 1]
        for k in range(N - 2, -1, -1):
            D[k] = c * (Z[k] - Y[k]).astype(np.float64) + B.T @ p
            p = wv[:, None] * X[k] + A.T @ p - K.T @ D[k]
    return X / s[None, :, None], Z.astype(np.float64)


def test_replica_of_the_folded_sweeps(hooks, fold):  # noqa: F811
    prob, A, B, K, C = _cartpole(0.5)
    x0 = t.problems.cartpole_x0(64, seed=92)
    lo, hi = np.asarray(prob.u_min)[:, 0], np.asarray(prob.u_max)[:, 0]
    sz, s, Ah, Bh = hooks.scale(A, B)
    assert sz
    a, k, b, c, w = fold.block(A, B, K, C)                       # the coefficients as packed
    xs, us = _replica(Ah, Bh, K / s[None, :], C, 1.0 / (s * s), s, x0, lo, hi, 100, prob.N)
    xf, uf = _replica_folded(a, b, k, c[0, 0], w, s, x0, lo, hi, 100, prob.N)
    ex, eu = np.abs(xf - xs).max(), np.abs(uf - us).max()
    print(f"folded against unfolded scaled replica, 64 instances, 100 iterations: states {ex:.3e}, controls {eu:.3e}")
    assert np.abs(us).max() > 0.4 and np.abs(xs).max() > 0.1      # (the clamp is active, the states are not trivial)
    assert ex <= 1e-12 and eu <= 1e-12


def test_random_single_input_models(hooks, fold):  # noqa: F811
    """tests/test_lean_scaled.py's generator at nu = 1, the models the scaled form is offered for: 10 iterations, horizon 10,
    8 instances, the clamp at 0.5.  A draw is skipped where the Riccati recursion fails on it or the unscaled replica leaves
    1e6 (an unstable model under the clamp); fewer than half may be."""
    rng = np.random.default_rng(2200)
    N, nb, tried, skipped, worst = 10, 8, 0, 0, 0.0
    while tried < 40:
        nx = int(rng.integers(1, 5))
        A = rng.standard_normal((nx, nx)) * (rng.random((nx, nx)) < rng.uniform(0.2, 0.9))
        B = rng.standard_normal((nx, 1)) * (rng.random((nx, 1)) < rng.uniform(0.2, 0.9))
        for i in range(nx):
            if rng.random() < 0.4:
                A[i, i] = 1.0
            if rng.random() < 0.1:
                A[i, int(rng.integers(0, nx))] = 1.0
        x0 = rng.uniform(-0.5, 0.5, (nx, nb))
        sz, s, Ah, Bh = hooks.scale(A, B)
        if not sz:
            continue                                              # (not offered: nothing to compare)
        tried += 1
        try:
            cache = t.host_precompute(A, B, np.eye(nx), np.eye(1), 1.0)
        except t.TinyMPCError:
            skipped += 1
            continue
        K, C = np.array(cache["Kinf"], dtype=np.float64), -1.0 * np.array(cache["Quu_inv"], dtype=np.float64)
        lo, hi = np.array([-0.5]), np.array([0.5])
        one = np.ones(nx)
        with np.errstate(all="ignore"):
            xr, ur = _replica(A, B, K, C, one, one, x0, lo, hi, 10, N)
        if not (np.all(np.isfinite(K)) and np.all(np.isfinite(xr)) and np.abs(xr).max() <= 1e6):
            skipped += 1
            continue
        blk = fold.block(A, B, K, C)
        assert blk is not None
        a, k, b, c, w = blk
        xs, us = _replica(Ah, Bh, K / s[None, :], C, 1.0 / (s * s), s, x0, lo, hi, 10, N)
        xf, uf = _replica_folded(a, b, k, c[0, 0], w, s, x0, lo, hi, 10, N)
        scale = max(1.0, np.abs(xs).max())
        ex, eu = np.abs(xf - xs).max() / scale, np.abs(uf - us).max()
        worst = max(worst, ex, eu)
        assert ex <= 1e-12 and eu <= 1e-12, (tried, nx, ex, eu)
    print(f"{tried} single-input models offered the scaled form, {skipped} skipped as unstable; worst difference {worst:.3e}")
    assert skipped < tried / 2
