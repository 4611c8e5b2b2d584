"""Per-instance families set up on the device, CPU part: the entry points exist (declared in include/tinympc_hip.h, exported by the
built library, bound by the Python mirror, present in the Julia module), and the rule the device kernel compiles — csrc/riccati.h,
run on the host through tinympc_host_family_cache — against the reference's goldens and against the parent's host code
(tinympc_host_precompute) over the very families the GPU tests use (tests/families_cases.py).

Bounds.  Against the goldens: 1e-12 norm-relative, what tests/test_capi_host.py gives host_precompute against the same files.
Against host_precompute: equal sweep counts on every instance, and values within CACHE_CAP = 1e-9 of max|host| per matrix (the
cap of the GPU test, four orders below the 1e-5 solution target the caches feed).  Measured on the build host: 0.0 for every
shape and matrix — the rule runs precompute_cache's sums in precompute_cache's order without contracting a product into the add
behind it, so on finite values the two agree to the last bit; test_rule_equals_host_code_bit_for_bit holds it to that.
Every test fails without the feature: neither the symbols nor the helpers exist there."""
import ctypes
import os
import re

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests import families_cases as fc
from tests.util import cm, golden_names, load_golden, nrel, problem_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = ("tinympc_create_families_device", "tinympc_set_families", "tinympc_get_family_cache", "tinympc_families_setup_mode",
          "tinympc_families_setup_ms")
GLOBAL = ("setup_families", "set_families", "get_family_cache", "families_setup_mode", "tinympc_host_family_cache",
          "tinympc_host_precompute_sweeps")
CACHE_CAP = 1e-9
GRID = {(nx, nu) for nx in (2, 3, 4, 6, 8, 10, 12) for nu in (1, 2, 3, 4)}
WITH_CACHE = [n for n in golden_names() if re.match(r"G[1-7]", n) and "cache" in load_golden(n)]


def test_header_declares_and_python_binds():
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    for sym in HANDLE + GLOBAL:
        assert re.search(r"\bint %s\(" % sym, header), sym
    from tinympc_julia_amd import tinympc
    for sym in HANDLE + GLOBAL:
        assert sym in tinympc.SIGNATURES, sym
    for name in ("set_families", "family_cache", "families_setup_mode"):
        assert hasattr(tinympc.BatchSolver, name), name
    assert "setup" in tinympc.BatchSolver.from_families.__code__.co_varnames
    assert callable(t.host_family_cache) and callable(t.host_precompute_sweeps)
    julia = open(os.path.join(ROOT, "tinympc-julia_amd", "julia", "TinyMPC.jl")).read()
    for name in ("setup_families", "set_families!", "family_cache", "families_setup_mode"):
        assert "function %s(" % name in julia, name
        assert name in julia.split("using LinearAlgebra")[0], name + " is not exported"
    assert "on_device::Bool=false" in julia
    csrc = os.path.join(ROOT, "tinympc-julia_amd", "csrc")
    unit = open(os.path.join(csrc, "families_setup.hip")).read()
    assert os.path.isfile(os.path.join(csrc, "riccati.h")) and "riccati_families_kernel" in unit and "fill_family_pack_kernel" in unit
    assert "fill_streamg_role" in unit      # (the pack's element map is the host fill's, not a restatement)


def test_built_library_exports_and_refuses(hip_lib):
    raw = ctypes.CDLL(t.LIB_PATH)
    for sym in HANDLE + GLOBAL:
        assert hasattr(raw, sym), sym
        assert getattr(hip_lib, sym).restype is ctypes.c_int
    hip_lib.cleanup_solver()
    assert hip_lib.families_setup_mode() == -1 and hip_lib.set_families(None, None, None, None, None) == -1
    assert b"not initialized" in hip_lib.tinympc_last_error()
    assert hip_lib.tinympc_families_setup_mode(None) == 0 and hip_lib.tinympc_set_families(None, None, None, None, None, None) == -1
    assert hip_lib.tinympc_get_family_cache(None, 0, 1, None, None, None, None, None) == -1
    with pytest.raises(t.TinyMPCError, match="nx in"):      # a shape outside the grid is refused, not computed by other code
        t.host_family_cache(np.eye(5), np.ones((5, 1)), np.eye(5), np.eye(1), 1.0)


@pytest.mark.parametrize("name", WITH_CACHE)
def test_rule_matches_reference_cache(hip_lib, name):
    """the rule against the cache the compiled reference produced, at host_precompute's tolerance against the same files"""
    g = load_golden(name)
    prob = problem_of(g)
    assert (prob.nx, prob.nu) in GRID
    c = t.host_family_cache(prob.A, prob.B, prob.Q, prob.R, prob.rho)
    for key, (r, cc) in dict(Kinf=(prob.nu, prob.nx), Pinf=(prob.nx, prob.nx), Quu_inv=(prob.nu, prob.nu), AmBKt=(prob.nx, prob.nx)).items():
        assert nrel(c[key], cm(g["cache"][key], r, cc)) <= 1e-12, key
    assert c["sweeps"] == t.host_precompute_sweeps(prob.A, prob.B, prob.Q, prob.R, prob.rho)


def test_goldens_with_a_cache_are_all_covered():
    assert len(WITH_CACHE) >= 4 and {n.split("_")[0] for n in WITH_CACHE} >= {"G1", "G6", "G7"}


def _rule(shape):
    A, Bm, Q, R, rho = fc.families(shape)
    cs = [t.host_family_cache(A[:, :, b], Bm[:, :, b], Q[:, :, b], R[:, :, b], rho[b]) for b in range(fc.FULL)]
    out = {k: np.stack([c[k] for c in cs], axis=2) for k in fc.KEYS}
    out["sweeps"] = np.array([c["sweeps"] for c in cs])
    return out


@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_rule_against_host_precompute(hip_lib, shape):
    """over the GPU test's families: the input conditions hold, every sweep count equals the host code's, values within the cap"""
    fc.check_input_conditions(shape)
    ref, got = fc.host_reference(shape), _rule(shape)
    bad = np.nonzero(got["sweeps"] != ref["sweeps"])[0]
    assert bad.size == 0, f"sweep counts differ on instances {bad[:8].tolist()}: {got['sweeps'][bad[:8]]} vs {ref['sweeps'][bad[:8]]}"
    err = fc.cache_error(got, ref)
    print(f"{shape}: rule vs host_precompute {err}, sweeps {ref['sweeps'].min()}..{ref['sweeps'].max()}")
    assert max(err.values()) <= CACHE_CAP, err


@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_rule_equals_host_code_bit_for_bit(hip_lib, shape):
    """what riccati.h claims for finite values: the same sums in the same order, no contraction — not one bit apart"""
    ref, got = fc.host_reference(shape), _rule(shape)
    for k in fc.KEYS:
        assert np.array_equal(got[k], ref[k]), k


def test_singular_instance_is_reported(hip_lib):
    A, B, Q, R = np.eye(2), np.zeros((2, 1)), np.eye(2), -2.0 * np.eye(1)      # R + 2 rho = 0 with rho = 1 and B = 0
    with pytest.raises(t.TinyMPCError, match="singular"):
        t.host_family_cache(A, B, Q, R, 1.0)
    sw = ctypes.c_int(7)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert hip_lib.tinympc_host_family_cache(dp(A), dp(B), dp(Q), dp(R), 1.0, 2, 1, None, None, None, None, ctypes.byref(sw)) == -1
    assert sw.value == -1
    with pytest.raises(t.TinyMPCError):
        t.host_precompute(A, B, Q, R, 1.0)


def test_sweep_cap_returns_what_the_host_returns(hip_lib):
    """a family that is still moving at the 1000th sweep keeps that sweep's K and P', as precompute_cache does"""
    ref = fc.host_reference((4, 1))
    b = int(np.nonzero(ref["sweeps"] == 1000)[0][0])
    A, Bm, Q, R, rho = fc.families((4, 1))
    c = t.host_family_cache(A[:, :, b], Bm[:, :, b], Q[:, :, b], R[:, :, b], rho[b])
    assert c["sweeps"] == 1000
    for k in fc.KEYS:
        assert np.array_equal(c[k], ref[k][:, :, b]), k
    # ... and a double integrator chain with a tiny input gain (a slow Riccati transient) does the same
    A2 = np.array([[1.0, 0.05], [0.0, 1.0]])
    B2 = np.array([[0.0], [1e-4]])
    c2, h2 = t.host_family_cache(A2, B2, np.eye(2), np.eye(1), 0.1), t.host_precompute(A2, B2, np.eye(2), np.eye(1), 0.1)
    assert c2["sweeps"] == t.host_precompute_sweeps(A2, B2, np.eye(2), np.eye(1), 0.1)
    for k in fc.KEYS:
        assert np.array_equal(c2[k], h2[k]), k
