"""CPU tests of the lean kernel's sparse-form routing (csrc/admm_params.h: lean_pattern_rm, lean_pattern_covers, the per-knot
costs; csrc/solver.h: lean_pick_form), reached through the library's test hooks tmpc_lean_*, which include/tinympc_hip.h does
not declare: zero / unit detection of (A, B), the coverage rule a built kernel's pattern applies to a model, and the cost
model that picks the sparse form for cartpole and the Hessenberg form for a dense pair."""
import ctypes

import numpy as np
import pytest

import tinympc_julia_amd as t

LF_PLAIN, LF_HB, LF_SPARSE = 1, 2, 3
UNIT, BBIT, ON = 16, 32, 48


@pytest.fixture(scope="module")
def hooks(hip_lib):
    lib = ctypes.CDLL(t.LIB_PATH)
    dp, u64 = ctypes.POINTER(ctypes.c_double), ctypes.c_ulonglong
    lib.tmpc_lean_pattern.restype = u64
    lib.tmpc_lean_pattern.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp]
    lib.tmpc_lean_costs.restype = ctypes.c_int
    lib.tmpc_lean_costs.argtypes = [ctypes.c_int, ctypes.c_int, u64, ctypes.POINTER(ctypes.c_int)]
    lib.tmpc_lean_covers.restype = ctypes.c_int
    lib.tmpc_lean_covers.argtypes = [u64, u64]
    lib.tmpc_lean_pick_form.restype = ctypes.c_int
    lib.tmpc_lean_pick_form.argtypes = [ctypes.c_int, ctypes.c_int, u64, u64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.tmpc_lean_builtin_pattern.restype = u64
    lib.tmpc_lean_builtin_pattern.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]

    class H:
        @staticmethod
        def pattern(A, B):
            A, B = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
            return lib.tmpc_lean_pattern(B.shape[0], B.shape[1], A.ctypes.data_as(dp), B.ctypes.data_as(dp))

        @staticmethod
        def costs(nx, nu, sp):
            out = (ctypes.c_int * 3)()
            assert lib.tmpc_lean_costs(nx, nu, sp, out) == 0
            return tuple(out)

        covers = staticmethod(lambda built, model: bool(lib.tmpc_lean_covers(built, model)))
        pick = staticmethod(lambda nx, nu, built, model, one, live, xb: lib.tmpc_lean_pick_form(nx, nu, built, model, one, live, xb))
        builtin = staticmethod(lib.tmpc_lean_builtin_pattern)
    return H


def _bits(sp, base, n):
    return [i for i in range(n) if (sp >> (base + i)) & 1]


def test_cartpole_pattern_and_units(hooks):
    p = t.problems.cartpole(20)
    sp = hooks.pattern(p.A, p.B)
    assert (sp >> ON) & 1
    assert _bits(sp, 0, 16) == [i * 4 + j for i in range(4) for j in range(4) if p.A[i, j] != 0.0]
    assert len(_bits(sp, 0, 16)) == 8
    assert _bits(sp, UNIT, 16) == [0, 5]                       # A[0][0], A[1][1]: exactly 1.0
    assert _bits(sp, BBIT, 16) == [1, 3]
    assert hooks.builtin(4, 1, 20) == sp                       # the built-in sparse kernels are cartpole's
    assert hooks.builtin(4, 1, 15) == 0 and hooks.builtin(12, 4, 20) == 0


def test_unit_must_be_exact(hooks):
    p = t.problems.cartpole(20)
    A = p.A.copy()
    A[0, 0] = 1.0000000001
    sp = hooks.pattern(A, p.B)
    assert _bits(sp, UNIT, 16) == [5]                          # still a nonzero, no longer a unit
    assert 0 in _bits(sp, 0, 16)
    A[0, 0] = -1.0
    assert _bits(hooks.pattern(A, p.B), UNIT, 16) == [5]
    assert hooks.pattern(np.eye(5), np.ones((5, 1))) == 0       # (nx above 4: no pattern)


def test_coverage_rule(hooks):
    p = t.problems.cartpole(20)
    built = hooks.pattern(p.A, p.B)
    assert hooks.covers(built, built)
    A = p.A.copy()
    A[0, 1] = 0.0                                              # one of the pattern's nonzeros removed: inside it
    assert hooks.covers(built, hooks.pattern(A, p.B))
    A = p.A.copy()
    A[3, 0] = 0.001                                            # a nonzero outside the pattern
    assert not hooks.covers(built, hooks.pattern(A, p.B))
    B = p.B.copy()
    B[0, 0] = 0.01
    assert not hooks.covers(built, hooks.pattern(p.A, B))
    A = p.A.copy()
    A[1, 1] = 1.0 + 1e-9                                       # an entry the kernel takes as 1 (never reads) is not 1
    assert not hooks.covers(built, hooks.pattern(A, p.B))
    A = p.A.copy()
    A[0, 0] = 0.0                                              # ... nor is a unit that became a zero
    assert not hooks.covers(built, hooks.pattern(A, p.B))
    A = p.A.copy()
    A[2, 2] = 1.0                                              # a new unit where the pattern has a general entry: fine
    assert hooks.covers(built, hooks.pattern(A, p.B))
    assert not hooks.covers(0, built) and not hooks.covers(built, 0)


def test_costs_and_choice(hooks):
    p = t.problems.cartpole(20)
    sp = hooks.pattern(p.A, p.B)
    assert hooks.costs(4, 1, sp) == (27, 37, 49)               # sparse, Hessenberg, plain dense fp64 per knot
    # fixed iterations, one wavefront per SIMD: sparse replaces HB; every other variant: sparse replaces the plain form
    for one, live, xb in [(1, 0, 0), (1, 1, 0), (1, 0, 1), (0, 0, 0), (0, 0, 1), (1, 1, 1)]:
        assert hooks.pick(4, 1, sp, sp, one, live, xb) == LF_SPARSE
    rng = np.random.default_rng(5)
    A, B = rng.standard_normal((4, 4)), rng.standard_normal((4, 1))
    dense = hooks.pattern(A, B)
    assert hooks.costs(4, 1, dense)[0] == 49
    assert hooks.pick(4, 1, dense, dense, 1, 0, 0) == LF_HB     # no cheaper than the band: HB keeps it
    assert hooks.pick(4, 1, dense, dense, 0, 0, 0) == LF_PLAIN
    assert hooks.pick(4, 1, sp, dense, 1, 0, 0) == LF_HB        # not covered
    A = p.A.copy()
    A[3, 0] = 0.001
    assert hooks.pick(4, 1, sp, hooks.pattern(A, p.B), 0, 1, 0) == LF_PLAIN
