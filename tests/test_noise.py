"""Seeded process / measurement noise, CPU part: the entry points exist (declared in include/tinympc_hip.h, exported by the
built library, bound by the Python mirror, present in the Julia module); the Philox4x32-10 block function against known answers;
tinympc_host_noise — csrc/noise.h compiled for the host, the text the device kernels compile — against a numpy restatement of
the draw rule written here (Philox in Python ints, np.log / sqrt / cos / sin); and the moments of the draws.

The rule: key (seed low, seed high), counter (b low, b high, t, (which << 16) | j), j = i // 2; u1 = (((w1:w0) >> 11) + 1) 2^-53,
u2 = ((w3:w2) >> 11) 2^-53, r = sqrt(-2 ln u1), xi[2j] = r cos(2 pi u2), xi[2j+1] = r sin(2 pi u2); n = G xi row by row with one
fma per column, ascending.

Tolerance of host_noise against the restatement: |delta| <= 1e-12 max(1, ||G||_inf) — |xi| <= 8.6 by construction (u1 >= 2^-53)
and a few ulp each in log, sqrt, the argument 2 pi u2 and cos come to about 1e-14: two orders of margin over libm differences.
Every test fails without the feature: neither the symbols nor the helpers exist there."""
import ctypes
import os
import re

import numpy as np
import pytest

import tinympc_julia_amd as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = ("tinympc_set_process_noise", "tinympc_set_measurement_noise", "tinympc_set_noise_cursor", "tinympc_noise_cursor", "tinympc_noise_mode",
          "tinympc_get_noise", "tinympc_get_mpc_measured", "tinympc_host_noise", "tmpc_philox4x32_10")
GLOBAL = ("set_process_noise", "set_measurement_noise", "set_noise_cursor", "noise_cursor")
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------------
# the rule, restated
# ---------------------------------------------------------------------------------------------------------------------------
def philox(ctr, key):
    c, k = [int(v) for v in ctr], [int(v) for v in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def normals(seed, which, b, t, nx):
    xi = np.zeros(nx + 1)
    for j in range((nx + 1) // 2):
        w = philox([b & M32, (b >> 32) & M32, t, (which << 16) | j], [seed & M32, (seed >> 32) & M32])
        u1 = np.float64((((w[1] << 32) | w[0]) >> 11) + 1) * 2.0 ** -53
        u2 = np.float64(((w[3] << 32) | w[2]) >> 11) * 2.0 ** -53
        r = np.sqrt(-2.0 * np.log(u1))
        xi[2 * j], xi[2 * j + 1] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
    return xi[:nx]


def restated(seed, which, b, t, nx, G=None):
    xi = normals(seed, which, b, t, nx)
    return xi if G is None else np.asarray(G, dtype=np.float64) @ xi


# ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_python_binds():
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    for sym in HANDLE + GLOBAL:
        assert re.search(r"\bint %s\(" % sym, header), sym
    assert "A sharded solver" in header and "takes none of it" in header
    from tinympc_julia_amd import tinympc
    for sym in HANDLE + GLOBAL:
        assert sym in tinympc.SIGNATURES, sym
    for name in ("set_process_noise", "set_measurement_noise", "set_noise_cursor", "noise_cursor", "noise_mode", "get_noise", "host_noise"):
        assert hasattr(tinympc.BatchSolver, name), name
        assert callable(getattr(t, name)), name
    julia = open(os.path.join(ROOT, "tinympc-julia_amd", "julia", "TinyMPC.jl")).read()
    for name in GLOBAL:
        assert "function %s(" % name in julia, name


def test_built_library_exports_the_entry_points(hip_lib):
    raw = ctypes.CDLL(t.LIB_PATH)
    for sym in HANDLE + GLOBAL:
        assert hasattr(raw, sym), sym
        assert getattr(hip_lib, sym).restype is ctypes.c_int      # (bound by load_library)
    # without a solver the global forms fail cleanly
    hip_lib.cleanup_solver()
    assert hip_lib.set_noise_cursor(0) == -1 and hip_lib.noise_cursor() == -1
    assert b"not initialized" in hip_lib.tinympc_last_error()


@pytest.mark.parametrize("ctr, key, want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([M32] * 4, [M32] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(hip_lib, ctr, key, want):
    c, k, out = (ctypes.c_uint * 4)(*ctr), (ctypes.c_uint * 2)(*key), (ctypes.c_uint * 4)()
    assert hip_lib.tmpc_philox4x32_10(c, k, out) == 0
    assert " ".join("%08x" % v for v in out) == want
    assert " ".join("%08x" % v for v in philox(ctr, key)) == want      # (the restatement below is held to them too)


_WORST = {"abs": 0.0}


@pytest.mark.parametrize("nx", [4, 5, 12])
def test_host_noise_matches_the_restatement(hip_lib, nx):
    rng = np.random.default_rng(100 + nx)
    full = rng.standard_normal((nx, nx))
    seed = 0x9E3779B97F4A7C15
    worst = 0.0
    for G in (None, np.eye(nx), full):
        scale = 1.0 if G is None else max(1.0, np.abs(G).sum(axis=1).max())
        for which in (0, 1):
            for b in (0, 69, 2 ** 32 + 3):
                for tt in (0, 1, 2 ** 31 - 1):
                    got, want = t.host_noise(seed, which, b, tt, nx, G), restated(seed, which, b, tt, nx, G)
                    assert got.shape == (nx,) and np.isfinite(got).all()
                    err = np.abs(got - want).max()
                    worst = max(worst, err / scale)
                    assert err <= 1e-12 * scale, (nx, which, b, tt, err)
    _WORST["abs"] = max(_WORST["abs"], worst)
    print(f"host_noise vs the numpy restatement, nx = {nx}: worst |delta| / max(1, ||G||_inf) = {worst:.3e}")
    # identity is the draw itself, and diag(sigma) scales it
    sig = rng.uniform(0.5, 2.0, nx)
    assert np.array_equal(t.host_noise(seed, 0, 5, 3, nx, np.eye(nx)), t.host_noise(seed, 0, 5, 3, nx))
    assert np.array_equal(t.host_noise(seed, 0, 5, 3, nx, sig), sig * t.host_noise(seed, 0, 5, 3, nx))
    # an odd nx drops the last sine: the first nx - 1 draws are those of nx - 1 (even), pair by pair
    assert np.array_equal(t.host_noise(seed, 1, 7, 2, nx)[:nx - 1], t.host_noise(seed, 1, 7, 2, nx - 1)[:nx - 1])


def test_host_noise_refusals(hip_lib):
    for args in ((1, 2, 0, 0, 4), (1, 0, -1, 0, 4), (1, 0, 0, -1, 4)):
        with pytest.raises(t.TinyMPCError):
            t.host_noise(*args)
    with pytest.raises(t.TinyMPCError, match="expected G"):
        t.host_noise(1, 0, 0, 0, 4, np.eye(3))


def test_moments(hip_lib):
    """70 instances x 40 steps x nx = 4, seed 12345, process stream.  The restatement gave mean -0.0099, standard deviation
    1.0037, largest |draw| 4.45, largest off-diagonal correlation 0.021; asserted as conditions of the rule: |mean| < 0.1 (10
    standard errors of 11 200 draws), |std - 1| < 0.1, every off-diagonal correlation below 0.1"""
    Bn, T, nx, seed = 70, 40, 4, 12345
    xi = np.array([[t.host_noise(seed, 0, b, k, nx) for k in range(T)] for b in range(Bn)])      # (B, T, nx)
    flat = xi.reshape(-1, nx)
    corr = np.corrcoef(flat.T)
    off = np.abs(corr - np.diag(np.diag(corr))).max()
    print(f"moments: mean {xi.mean():.4f} std {xi.std():.4f} largest |draw| {np.abs(xi).max():.2f} largest off-diagonal correlation {off:.3f}")
    assert abs(xi.mean()) < 0.1 and abs(xi.std() - 1.0) < 0.1 and off < 0.1
    assert np.abs(xi).max() <= 8.6
    # the process and the measurement stream of one (b, t) differ; two seeds differ; the same seed repeats bit for bit
    meas = np.array([[t.host_noise(seed, 1, b, k, nx) for k in range(T)] for b in range(Bn)])
    assert not np.any(meas == xi)
    other = np.array([t.host_noise(seed + 1, 0, b, 0, nx) for b in range(Bn)])
    assert not np.any(other == xi[:, 0, :])
    again = np.array([[t.host_noise(seed, 0, b, k, nx) for k in range(T)] for b in range(Bn)])
    assert np.array_equal(again, xi)
    # no two (instance, step) cells share a draw
    assert len(np.unique(flat[:, 0])) == Bn * T
