"""CPU tests of the lean kernel's scaled sparse form (csrc/admm_params.h: lean_pattern_scaled, lean_cost_scaled; csrc/kernels.hip:
lean_scale_model), reached through the library's test hooks tmpc_lean_scaled_pattern / _scaled_cost / _scale_model, which
include/tinympc_hip.h does not declare.

The diagonal change of coordinates x^ = S x turns off-diagonal nonzeros of A (an acyclic set) and one nonzero of B into exact
units, which gives forward rows a free start: cartpole 25 fp64 per knot for 27.  The pattern is chosen from positions alone;
the scaling follows a model's values and is refused where a chosen entry is zero or nothing is gained.  The algebra of the
scaled sweeps (p^ = S^-1 p~, W = S^-2, K^ = Kinf S^-1) is settled here by a numpy fp64 replica of both sweeps, with the fp32
slack and dual of the kernel, against the same replica on the model as given."""
import ctypes

import numpy as np
import pytest

import tinympc_julia_amd as t

UNIT, BBIT, ON, SCALED, BU, BU_ON = 16, 32, 48, 49, 50, 54


@pytest.fixture(scope="module")
def hooks(hip_lib):
    lib = ctypes.CDLL(t.LIB_PATH)
    dp, u64 = ctypes.POINTER(ctypes.c_double), ctypes.c_ulonglong
    lib.tmpc_lean_pattern.restype = u64
    lib.tmpc_lean_pattern.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp]
    lib.tmpc_lean_costs.restype = ctypes.c_int
    lib.tmpc_lean_costs.argtypes = [ctypes.c_int, ctypes.c_int, u64, ctypes.POINTER(ctypes.c_int)]
    lib.tmpc_lean_scaled_pattern.restype = u64
    lib.tmpc_lean_scaled_pattern.argtypes = [ctypes.c_int, ctypes.c_int, u64]
    lib.tmpc_lean_scaled_cost.restype = ctypes.c_int
    lib.tmpc_lean_scaled_cost.argtypes = [ctypes.c_int, ctypes.c_int, u64]
    lib.tmpc_lean_scale_model.restype = u64
    lib.tmpc_lean_scale_model.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp, u64, dp, dp, dp]

    class H:
        @staticmethod
        def pattern(A, B):
            A, B = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
            return lib.tmpc_lean_pattern(B.shape[0], B.shape[1], A.ctypes.data_as(dp), B.ctypes.data_as(dp))

        @staticmethod
        def sparse_cost(nx, nu, sp):
            out = (ctypes.c_int * 3)()
            assert lib.tmpc_lean_costs(nx, nu, sp, out) == 0
            return out[0]

        scaled_pattern = staticmethod(lambda nx, nu, sp: lib.tmpc_lean_scaled_pattern(nx, nu, sp))
        scaled_cost = staticmethod(lambda nx, nu, sz: lib.tmpc_lean_scaled_cost(nx, nu, sz))

        @staticmethod
        def scale(A, B, built=0):
            """(scaled pattern or 0, s, A^, B^) of the row-major model under the kernel of lean_pattern_scaled(built)"""
            A, B = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
            nx, nu = B.shape
            s, Ah, Bh = np.zeros(nx), np.zeros((nx, nx)), np.zeros((nx, nu))
            sz = lib.tmpc_lean_scale_model(nx, nu, A.ctypes.data_as(dp), B.ctypes.data_as(dp), built, s.ctypes.data_as(dp),
                                           Ah.ctypes.data_as(dp), Bh.ctypes.data_as(dp))
            return sz, s, Ah, Bh
    return H


def _bits(sp, base, n):
    return [i for i in range(n) if (sp >> (base + i)) & 1]


def _units(sz, nx, nu):
    """the unit positions of a scaled pattern: [(i, j)] of A, [(i, a)] of B"""
    ua = [(e // nx, e % nx) for e in _bits(sz, UNIT, nx * nx)]
    ub = [divmod((sz >> BU) & 15, nu)] if (sz >> BU_ON) & 1 else []
    return ua, ub


def test_cartpole_scaled_pattern(hooks):
    p = t.problems.cartpole(20)
    sp = hooks.pattern(p.A, p.B)
    sz = hooks.scaled_pattern(4, 1, sp)
    assert (sz >> SCALED) & 1 and (sz >> ON) & 1 and not (sp >> SCALED) & 1
    assert _bits(sz, 0, 16) == _bits(sp, 0, 16) and _bits(sz, BBIT, 16) == _bits(sp, BBIT, 16)   # the nonzeros stay
    ua, ub = _units(sz, 4, 1)
    assert ua == [(0, 0), (0, 1), (1, 1), (1, 2), (2, 3)] and ub == [(3, 0)]   # A00, A11 carried over; A01, A12, A23, B3 chosen
    assert hooks.scaled_cost(4, 1, sz) == 25
    assert hooks.sparse_cost(4, 1, sp) == 27                                      # the unscaled form's cost has not moved
    assert hooks.scaled_pattern(4, 1, sz) == 0 and hooks.scaled_pattern(4, 1, 0) == 0
    got, s, Ah, Bh = hooks.scale(p.A, p.B)
    assert got == sz
    assert Ah[0, 1] == 1.0 and Ah[1, 2] == 1.0 and Ah[2, 3] == 1.0 and Bh[3, 0] == 1.0
    assert np.array_equal(np.diag(Ah), np.diag(p.A))


def _acyclic(edges, nx):
    comp = list(range(nx))
    for i, j in edges:
        if comp[i] == comp[j]:
            return False
        ci, cj = comp[i], comp[j]
        comp = [ci if c == cj else c for c in comp]
    return True


def test_random_models(hooks):
    rng = np.random.default_rng(2100)
    offered = refused = 0
    for trial in range(200):
        nx, nu = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        A = rng.standard_normal((nx, nx)) * (rng.random((nx, nx)) < rng.uniform(0.2, 0.9))
        B = rng.standard_normal((nx, nu)) * (rng.random((nx, nu)) < rng.uniform(0.2, 0.9))
        for i in range(nx):                                     # (some exact units, on and off the diagonal)
            if rng.random() < 0.4:
                A[i, i] = 1.0
            if rng.random() < 0.1:
                A[i, int(rng.integers(0, nx))] = 1.0
        sp = hooks.pattern(A, B)
        sz = hooks.scaled_pattern(nx, nu, sp)
        assert sz != 0
        ua, ub = _units(sz, nx, nu)
        chosen = [(i, j) for i, j in ua if i != j]
        assert all(A[i, j] != 0.0 for i, j in chosen) and all(B[i, a] != 0.0 for i, a in ub)
        assert all(A[i, i] == 1.0 for i, j in ua if i == j) and len([1 for i, j in ua if i == j]) == sum(A[i, i] == 1.0 for i in range(nx))
        assert _acyclic(chosen, nx) and len(chosen) <= nx - 1 and len(ub) <= 1
        cheaper = hooks.scaled_cost(nx, nu, sz) < hooks.sparse_cost(nx, nu, sp)
        got, s, Ah, Bh = hooks.scale(A, B)
        assert (got == sz) if cheaper else (got == 0), (trial, hex(sp), hex(sz))    # offered only where it is cheaper
        if not got:
            refused += 1
            continue
        offered += 1
        assert np.all(np.isfinite(s)) and np.all(s != 0.0)
        for i, j in ua:
            assert Ah[i, j] == 1.0
        for i, a in ub:
            assert Bh[i, a] == 1.0
        assert np.array_equal((Ah != 0.0), (A != 0.0)) and np.array_equal((Bh != 0.0), (B != 0.0))
        back_a, back_b = Ah * s[None, :] / s[:, None], Bh / s[:, None]              # S^-1 A^ S, S^-1 B^
        assert np.all(np.abs(back_a - A) <= 8 * np.finfo(float).eps * np.abs(A)), trial
        assert np.all(np.abs(back_b - B) <= 8 * np.finfo(float).eps * np.abs(B)), trial
        # the same kernel (the pattern as built) refuses the model with a chosen entry zeroed
        i, j = chosen[0] if chosen else (None, None)
        if chosen:
            A0 = A.copy()
            A0[i, j] = 0.0
            assert hooks.scale(A0, B, built=sp)[0] == 0
        if ub:
            B0 = B.copy()
            B0[ub[0]] = 0.0
            assert hooks.scale(A, B0, built=sp)[0] == 0
    print(f"scaled form offered for {offered} of 200 random models, refused for {refused}")
    assert offered >= 20 and refused >= 20


def test_zero_inside_the_pattern_is_refused(hooks):
    p = t.problems.cartpole(20)
    sp = hooks.pattern(p.A, p.B)
    A = p.A.copy()
    A[0, 1] = 0.0                                              # tests/test_lean_sparse_gpu.py::test_zero_inside_the_pattern
    A[2, 3] = 0.012
    assert hooks.scale(A, p.B, built=sp)[0] == 0
    A = p.A.copy()
    A[3, 2] = 0.0                                              # a nonzero the scaling did not choose may vanish
    assert hooks.scale(A, p.B, built=sp)[0] == hooks.scaled_pattern(4, 1, sp)


# ---- the algebra: a replica of the sweeps (fp64 recurrences, fp32 slack and dual; csrc/admm_lean.hip.h) ----
def _replica(A, B, K, C, w, s, x0, lo, hi, iters, N):
    """states [N][nx][batch] in the ORIGINAL coordinates and controls [N-1][nu][batch] after `iters` cold-started iterations
    of x^+ = A x^ + B u, u = -K x^ - d; t = r~ + B' p^, d = C t, p^ = W x^ + A' p^ - K' t, p^_{N-1} = W x^_{N-1}; x^_0 = S x0"""
    nx, nu = B.shape
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
        p = w[:, None] * X[N - 1]
        for k in range(N - 2, -1, -1):
            tk = (Z[k] - Y[k]).astype(np.float64) + B.T @ p
            D[k] = C @ tk
            p = w[:, None] * X[k] + A.T @ p - K.T @ tk
    return X / s[None, :, None], Z.astype(np.float64)


def test_replica_of_the_scaled_sweeps(hooks):
    prob = t.problems.cartpole(20, u_bound=0.5)
    x0 = t.problems.cartpole_x0(64, seed=92)
    c = t.host_precompute(prob.A, prob.B, prob.Q, prob.R, prob.rho)
    K, C = np.asarray(c["Kinf"]), -prob.rho * np.asarray(c["Quu_inv"])
    A, B = np.asarray(prob.A, dtype=np.float64), np.asarray(prob.B, dtype=np.float64)
    lo, hi = np.asarray(prob.u_min)[:, 0], np.asarray(prob.u_max)[:, 0]
    one = np.ones(4)
    xr, ur = _replica(A, B, K, C, one, one, x0, lo, hi, 100, prob.N)
    sz, s, Ah, Bh = hooks.scale(A, B)
    assert sz
    xs, us = _replica(Ah, Bh, K / s[None, :], C, 1.0 / (s * s), s, x0, lo, hi, 100, prob.N)
    ex, eu = np.abs(xs - xr).max(), np.abs(us - ur).max()
    print(f"scaled against unscaled replica, 64 instances, 100 iterations: states {ex:.3e}, controls {eu:.3e}")
    assert np.abs(ur).max() > 0.4 and np.abs(xr).max() > 0.1      # (the clamp is active, the states are not trivial)
    assert ex <= 1e-12 and eu <= 1e-12
