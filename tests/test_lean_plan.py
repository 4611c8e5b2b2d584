"""CPU tests of the lean kernel's routing (csrc/solver.h: lean_plan, the one place that decides whether a launch runs on the
lean kernel and as which admm_lean_kernel<LIVE, UBK, ONE, XB, REFS, ST, SP, WS, MPC>), reached through the library's test
hook tmpc_lean_plan, which include/tinympc_hip.h does not declare.  Every case: 256 CUs, the cartpole model, a built-in
(4, 1, 20) entry with every kind of kernel, a cold one-shot solve of 65 536 instances with fixed iterations, zero references
and uniform input bounds — unless the case says otherwise."""
import ctypes
import itertools

import numpy as np
import pytest

import tinympc_julia_amd as t

LIVE, UBK, ONE, XB, SHARED, F64, SPARSE, WS, MPC = 1, 2, 4, 8, 16, 32, 64, 128, 256
LF_NONE, LF_PLAIN, LF_HB, LF_SPARSE = 0, 1, 2, 3
LK_ALL = 31
REF_ZERO, REF_SHARED, REF_PER_INSTANCE = 0, 1, 2
# LeanPlanIn's fields in their order (the two patterns apart)
FIELDS = ["nx", "nu", "N", "builtin", "kinds", "lean_jit", "lean_ok", "knot_bounds", "quad_G", "precision", "sw_one", "sw_dense",
          "sw_ws", "sw_loop", "slots", "iters", "mpc_steps", "cold", "save", "indexed", "adaptive_rho", "ref_mode", "loop",
          "state_bounds", "g_maybe_nonzero", "live", "stream_ext", "cus"]
BASE = dict(nx=4, nu=1, N=20, builtin=1, kinds=LK_ALL, lean_jit=0, lean_ok=1, knot_bounds=0, quad_G=1, precision=0, sw_one=0,
            sw_dense=0, sw_ws=0, sw_loop=0, slots=65536, iters=100, mpc_steps=0, cold=1, save=0, indexed=0, adaptive_rho=0,
            ref_mode=REF_ZERO, loop=0, state_bounds=0, g_maybe_nonzero=0, live=0, stream_ext=0, cus=256)
WARM = dict(cold=0, save=1)
N30 = dict(N=30, builtin=0, kinds=0, lean_jit=1)          # a shape without a built-in entry: single variants on request


@pytest.fixture(scope="module")
def plan(hip_lib):
    lib = ctypes.CDLL(t.LIB_PATH)
    u64, dp = ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_double)
    lib.tmpc_lean_plan.restype = ctypes.c_int
    lib.tmpc_lean_plan.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, u64, u64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(u64)]
    lib.tmpc_lean_pattern.restype = u64
    lib.tmpc_lean_pattern.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp]
    lib.tmpc_lean_builtin_pattern.restype = u64
    lib.tmpc_lean_builtin_pattern.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    p = t.problems.cartpole(20)
    A, B = np.ascontiguousarray(p.A, dtype=np.float64), np.ascontiguousarray(p.B, dtype=np.float64)
    model = lib.tmpc_lean_pattern(4, 1, A.ctypes.data_as(dp), B.ctypes.data_as(dp))
    built = lib.tmpc_lean_builtin_pattern(4, 1, 20)
    assert model and built == model

    def call(*parts, **kw):
        """(take, variant, form, cost_sparse, cost_dense, pattern weighed)"""
        v = dict(BASE)
        for part in parts + (kw,):
            assert set(part) <= set(FIELDS), set(part) - set(FIELDS)
            v.update(part)
        arr = (ctypes.c_int * len(FIELDS))(*[int(v[f]) for f in FIELDS])
        out, sp = (ctypes.c_int * 5)(), u64(0)
        assert lib.tmpc_lean_plan(arr, len(FIELDS), built if v["builtin"] else 0, model, out, ctypes.byref(sp)) == 0
        return bool(out[0]), out[1], out[2], out[3], out[4], sp.value
    call.model = model
    return call


TAKEN = {
    # case: (inputs, variant bits, form)
    "batch_131072": (dict(slots=131072), UBK | SPARSE, LF_SPARSE),
    "batch_65536": (dict(), UBK | ONE | SPARSE, LF_SPARSE),
    "shared_refs": (dict(ref_mode=REF_SHARED), UBK | ONE | SHARED, LF_HB),
    "batch_131072_tolerances": (dict(slots=131072, live=1), LIVE | UBK | ONE | SPARSE, LF_SPARSE),
    "batch_131072_knot_bounds": (dict(slots=131072, knot_bounds=1), 0, LF_PLAIN),
    "state_bound": (dict(state_bounds=1), UBK | ONE | XB | SPARSE, LF_SPARSE),
    "ws_forced_live": (dict(WARM, sw_ws=1, ref_mode=REF_SHARED, knot_bounds=1, g_maybe_nonzero=1), LIVE | ONE | XB | SHARED | WS, LF_PLAIN),
    "loop": (dict(WARM, sw_ws=1, sw_loop=1, loop=1, mpc_steps=10), LIVE | UBK | ONE | SPARSE | WS | MPC, LF_SPARSE),
    "precision_2": (dict(precision=2, quad_G=0, builtin=0, kinds=0, lean_jit=1), UBK | ONE | F64 | SPARSE, LF_SPARSE),
    "n30_batch_131072": (dict(N30, slots=131072), UBK | ONE | SPARSE, LF_SPARSE),      # ONE: 256 registers do not hold N = 30
    "n30_ws_fixed": (dict(N30, **WARM, sw_ws=1), UBK | ONE | SPARSE | WS, LF_SPARSE),
    "lean_dense": (dict(slots=131072, sw_dense=1), UBK, LF_PLAIN),
}
assert [TAKEN[k][1] for k in TAKEN] == [66, 70, 22, 71, 0, 78, 157, 455, 102, 70, 198, 2]

NOT_TAKEN = {
    "warm_without_lean_ws": dict(WARM),
    "n30_ws_tolerances_lds": dict(N30, **WARM, sw_ws=1, live=1),
    "index_list": dict(indexed=1),
    "per_instance_refs": dict(ref_mode=REF_PER_INSTANCE),
    "adaptive_rho": dict(adaptive_rho=1),
    "zero_iterations": dict(iters=0),
}


@pytest.mark.parametrize("case", list(TAKEN))
def test_variant_and_form(plan, case):
    kw, variant, form = TAKEN[case]
    take, v, f, cost_sparse, cost_dense, sp = plan(**kw)
    assert take and (v, f) == (variant, form), (take, v, f)
    # the two costs tmpc_lean_last_form reports: the sparse form's (cartpole's pattern: 27 fp64 instructions per knot) where a
    # pattern was weighed, and the dense form's it is weighed against — Hessenberg (37) in the 512-register fixed-iteration
    # kernels without a state bound, else plain (49)
    assert sp == plan.model and cost_sparse == 27
    assert cost_dense == (37 if (v & ONE) and not (v & (LIVE | XB)) else 49)


@pytest.mark.parametrize("case", list(NOT_TAKEN))
def test_not_taken(plan, case):
    assert plan(**NOT_TAKEN[case]) == (False, 0, LF_NONE, 0, 0, 0)


def test_entry_kinds_and_loop_requests(plan):
    """what the entry lacks is not planned: no sparse kernels — the dense form; no WS kernels — warm solves stay off the lean
    kernel; a loop request gets the loop kernel or nothing"""
    assert plan(kinds=0)[:3] == (True, UBK | ONE, LF_HB)
    assert plan(kinds=0)[3:] == (0, 37, 0)
    assert not plan(WARM, sw_ws=1, kinds=1)[0]
    assert plan(WARM, sw_ws=1, kinds=2)[:3] == (True, UBK | ONE | WS, LF_HB)
    loop = dict(WARM, sw_ws=1, sw_loop=1, loop=1, mpc_steps=10)
    assert plan(loop, kinds=LK_ALL & ~16)[:3] == (True, LIVE | UBK | ONE | WS | MPC, LF_PLAIN)   # no sparse loop kernel: the dense one
    assert not plan(loop, kinds=LK_ALL & ~(8 | 16))[0]
    assert plan(loop, kinds=LK_ALL & ~8)[1] == 455 and not plan(loop, kinds=LK_ALL & ~8, sw_dense=1)[0]
    assert not plan(loop, sw_loop=0)[0] and not plan(loop, mpc_steps=0)[0]
    assert not plan(WARM, sw_ws=1, mpc_steps=10)[0]                   # steps in one launch without the loop: the quad kernel's
    assert not plan(lean_ok=0)[0] and not plan(precision=1)[0] and not plan(WARM, sw_ws=1, quad_G=16)[0]
    assert not plan(precision=2, quad_G=0, builtin=0, kinds=0, lean_jit=1, stream_ext=1)[0]


def test_normalisations_hold_everywhere(plan):
    """over the boolean inputs of both kinds of entry: LIVE, WS and F64 imply ONE; MPC implies LIVE and WS; the WS pattern
    XB + shared references + per-knot bounds is LIVE; the built-in sparse kernels see zero references and uniform bounds"""
    flags = ["knot_bounds", "sw_one", "sw_dense", "sw_loop", "state_bounds", "g_maybe_nonzero", "live", "loop"]
    n = 0
    for entry in (dict(), dict(N30), dict(N=12, builtin=0, kinds=0, lean_jit=1)):
        for bits in itertools.product((0, 1), repeat=len(flags)):
            for slots, warm, ref in itertools.product((256, 65792), (0, 1), (REF_ZERO, REF_SHARED)):
                kw = dict(entry, **dict(zip(flags, bits)), slots=slots, ref_mode=ref, sw_ws=1, mpc_steps=5 if bits[-1] else 0)
                take, v, form, _, _, _ = plan(kw, WARM if warm else {})
                if not take:
                    assert (v, form) == (0, LF_NONE)
                    continue
                n += 1
                assert bool(v & UBK) != bool(kw["knot_bounds"]) and bool(v & SHARED) == (ref == REF_SHARED)
                assert bool(v & WS) == bool(warm) and bool(v & SPARSE) == (form == LF_SPARSE)
                if v & (LIVE | WS | F64):
                    assert v & ONE
                if v & MPC:
                    assert (v & LIVE) and (v & WS) and kw["loop"]
                if (v & WS) and (v & XB) and (v & SHARED) and not (v & UBK):
                    assert v & LIVE
                if (v & SPARSE) and "N" not in entry:
                    assert (v & UBK) and not (v & SHARED)
                if not (v & ONE):
                    assert slots > 256 * 256 and ("N" not in entry or 2 * entry["N"] * 4 + 3 * entry["N"] + 50 <= 250)
    assert n > 1000
