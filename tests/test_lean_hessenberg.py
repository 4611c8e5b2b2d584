"""CPU tests of the controller-Hessenberg (staircase) reduction the lean kernel's fixed-iteration variants iterate in
(csrc/host_setup.cpp: staircase_form, reached through the library's test hook tmpc_lean_staircase, which
include/tinympc_hip.h does not declare): an orthogonal T with T' B upper trapezoidal and T' M T of lower bandwidth nu,
entries outside that pattern exactly zero, on the cartpole family and on random (nx, nu) pairs up to nx = 12, complex
eigenvalues and uncontrollable pairs included."""
import ctypes

import numpy as np
import pytest

import tinympc_julia_amd as t


@pytest.fixture(scope="module")
def staircase(hip_lib):
    lib = ctypes.CDLL(t.LIB_PATH)
    f = lib.tmpc_lean_staircase
    f.restype = ctypes.c_int
    dp = ctypes.POINTER(ctypes.c_double)
    f.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp, dp, dp, dp]

    def run(M, B):
        nx, nu = B.shape
        M, B = np.ascontiguousarray(M, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
        T, Mh, Bh = np.zeros((nx, nx)), np.zeros((nx, nx)), np.zeros((nx, nu))
        args = [a.ctypes.data_as(dp) for a in (M, B, T, Mh, Bh)]
        assert f(nx, nu, *args) == 0
        return T, Mh, Bh
    return run


def _check(run, M, B):
    nx, nu = B.shape
    T, Mh, Bh = run(M, B)
    assert np.abs(T.T @ T - np.eye(nx)).max() <= 1e-14
    sm, sb = max(np.abs(M).max(), 1e-300), max(np.abs(B).max(), 1e-300)
    assert np.abs(T.T @ M @ T - Mh).max() <= 1e-13 * sm
    assert np.abs(T.T @ B - Bh).max() <= 1e-13 * sb
    m, j = np.indices((nx, nx))
    assert np.all(Mh[j < m - nu] == 0.0)                    # lower bandwidth nu
    m, a = np.indices((nx, nu))
    assert np.all(Bh[m > a] == 0.0)                         # upper trapezoidal
    return T, Mh, Bh


def test_cartpole_reduction(staircase):
    prob = t.problems.cartpole(20)
    # M = A - B Kinf for some gain: the reduction depends only on the pair, take a fixed one
    K = np.array([[-3.1, -4.2, 25.0, 6.3]])
    M = prob.A - prob.B @ K
    T, Mh, Bh = _check(staircase, M, prob.B)
    assert np.count_nonzero(Bh) == 1 and np.count_nonzero(Mh) <= 13


def _random_pair(rng, nx, nu, kind):
    if kind == "dense":
        M, B = rng.standard_normal((nx, nx)), rng.standard_normal((nx, nu))
    elif kind == "complex":                                 # rotation blocks: complex-conjugate eigenvalues
        M = np.zeros((nx, nx))
        for i in range(0, nx - 1, 2):
            th, r = rng.uniform(0.1, 3.0), rng.uniform(0.5, 1.05)
            M[i:i + 2, i:i + 2] = r * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        if nx % 2:
            M[-1, -1] = rng.uniform(-1, 1)
        Q, _ = np.linalg.qr(rng.standard_normal((nx, nx)))
        M, B = Q @ M @ Q.T, rng.standard_normal((nx, nu))
    else:                                                   # uncontrollable: a decoupled block B does not reach
        c = int(rng.integers(1, nx))
        M = np.zeros((nx, nx))
        M[:c, :c] = rng.standard_normal((c, c))
        M[c:, c:] = rng.standard_normal((nx - c, nx - c))
        M[:c, c:] = rng.standard_normal((c, nx - c))
        B = np.zeros((nx, nu))
        B[:c] = rng.standard_normal((c, nu))
        Q, _ = np.linalg.qr(rng.standard_normal((nx, nx)))
        M, B = Q @ M @ Q.T, Q @ B
    return M * rng.choice([1e-3, 1.0, 1e3]), B * rng.choice([1e-3, 1.0, 1e2])


def test_random_families(staircase):
    rng = np.random.default_rng(2026)
    kinds = ("dense", "complex", "uncontrollable")
    n = 0
    for i in range(200):
        nx = int(rng.integers(2, 13))
        nu = int(rng.integers(1, min(nx, 5) + 1))
        kind = kinds[i % 3]
        if kind == "uncontrollable" and nx < 2:
            kind = "dense"
        M, B = _random_pair(rng, nx, nu, kind)
        _check(staircase, M, B)
        n += 1
    assert n == 200


def test_degenerate_pairs(staircase):
    """B = 0, nu >= nx, an already banded pair: nothing to reduce, still orthogonal and exact"""
    rng = np.random.default_rng(5)
    _check(staircase, rng.standard_normal((4, 4)), np.zeros((4, 1)))
    _check(staircase, rng.standard_normal((3, 3)), rng.standard_normal((3, 4)))
    T, Mh, Bh = _check(staircase, np.triu(rng.standard_normal((5, 5)), -1), np.eye(5)[:, :1])
    assert np.allclose(np.abs(T), np.eye(5))
