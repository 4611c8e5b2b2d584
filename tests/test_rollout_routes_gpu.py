"""Which route an mpc_rollout takes (csrc/solver.hip, Solver::plan_rollout), one case per route and per refusal: the loop fused
into the selected kernel (quad, mfmat), the chain of workspace-carrying launches (mfma; the lean kernel under
TINYMPC_HIP_LEAN_WS; the stream and generic kernels under TINYMPC_HIP_STREAM_MPC), the lean and the stream kernel's in-kernel
loops (TINYMPC_HIP_LEAN_LOOP, TINYMPC_HIP_STREAM_LOOP), and every refusal with its full text.

A case is read back through what the library already reports: kernel_name (the selected family), last_launch_name (the kernel
the last launch ran), tmpc_last_rollout_launches (solve-kernel launches of the last rollout enqueued: `steps` for a chain, 1 for
any in-kernel loop, -1 before any rollout) and TinyMPCError's text.  Each case asserts the triple — or the refusal's text with
the launch count left as it was — and that a second mpc_rollout on the same solver takes the same route.  Where a chain and a
loop kernel both take a case, their logs are equal bit for bit.

The expected values are those of the commit before the routes were gathered into plan_rollout — the file passed there
unchanged — so it pins the decision table, not one implementation of it.  Tiny shapes: batch 130 (two wavefronts, the second
ragged), 3 steps, 5 iterations for every instance."""
import ctypes

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.test_ref_sequence import cartpole_tracking_refs

pytestmark = pytest.mark.gpu

B, STEPS = 130, 3
# five iterations for every instance.  The lean cases ask for them with tolerances no residual reaches: the lean kernel's loop is
# its tolerance-terminated form, and so then is the chain's every launch — the two run the same sweeps
FIXED = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=5, check_termination=1)
NEVER = dict(abs_pri_tol=1e-30, abs_dua_tol=1e-30, max_iter=5, check_termination=1)
SWITCHES = ("TINYMPC_HIP_LEAN_WS", "TINYMPC_HIP_LEAN_LOOP", "TINYMPC_HIP_STREAM_MPC", "TINYMPC_HIP_STREAM_LOOP", "TINYMPC_HIP_NO_STREAM",
            "TINYMPC_HIP_GROUP", "TINYMPC_HIP_STREAM_F64", "TINYMPC_HIP_MFMA_ONESHOT_ONLY", "TINYMPC_HIP_NO_MFMAT")
ROCKET_CONE = ([0], [3], [0.25], [], [], [])          # one input cone

NO_KERNEL = "mpc_rollout: this problem shape / option set has no kernel with a fused closed loop"
NO_WORKSPACE = "mpc_rollout needs the persistent workspace (set_warm_start(1))"
SEQ_SHORT = "mpc_rollout: the reference sequence holds 2 steps, the loop asks for 3 (one reference set per step)"
SEQ_PER_INSTANCE = ("mpc_rollout: a reference sequence is shared by the batch and cannot be combined with per-instance references "
                    "(set_ref_sequence with steps = 0 drops the sequence)")

LEAN_WS, LEAN_LOOP = {"TINYMPC_HIP_LEAN_WS": "1", "TINYMPC_HIP_GROUP": "1"}, {"TINYMPC_HIP_LEAN_LOOP": "1"}
STREAM_MPC, STREAM_LOOP, NO_STREAM = {"TINYMPC_HIP_STREAM_MPC": "1"}, {"TINYMPC_HIP_STREAM_LOOP": "1"}, {"TINYMPC_HIP_NO_STREAM": "1"}


def _launches(bs):
    f = ctypes.CDLL(t.LIB_PATH).tmpc_last_rollout_launches
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p]
    return f(bs.h)


def _cartpole(N):
    return t.problems.cartpole(N, u_bound=0.5), t.problems.cartpole_x0(B, seed=7)


def _quadrotor(N):
    return t.problems.quadrotor(N, u_bound=0.5), t.problems.quadrotor_x0(B, seed=5)


def _rocket(N):
    return t.problems.rocket(N), t.problems.rocket_x0(B, seed=5)


def _sequence(steps):
    return lambda bs: bs.set_ref_sequence(*cartpole_tracking_refs(bs.N, steps))


def _per_instance(bs):
    prob = t.problems.cartpole(bs.N, u_bound=0.5)
    bs.set_x_ref(np.repeat(np.zeros_like(prob.x_min)[:, :, None] + 0.05, B, axis=2))


def _sequence_then_per_instance(bs):
    _sequence(STEPS)(bs)
    _per_instance(bs)


def _rocket_ext(bs):
    bs.set_fdyn(t.problems.rocket(bs.N).fdyn)
    bs.set_cone_constraints(*ROCKET_CONE)


# id: (problem, environment, settings, further set-up, warm start, expected (kernel_name, last_launch_name, launches) or refusal)
CASES = {
    "fused_quad": (lambda: _cartpole(10), {}, FIXED, None, True, ("quad<4,1,10,g4>", "quad<4,1,10,g4>", 1)),
    "fused_quad_cold": (lambda: _cartpole(10), {}, FIXED, None, False, NO_WORKSPACE),
    "mfma_chain": (lambda: _quadrotor(10), {}, FIXED, None, True, ("mfma<12,4,10>", "mfma<12,4,10>", STEPS)),
    "fused_mfmat": (lambda: _rocket(10), {}, FIXED, _rocket_ext, True, ("mfmat<6,3,10>", "mfmat<6,3,10>", 1)),
    "lean_chain": (lambda: _cartpole(20), LEAN_WS, NEVER, None, True, ("quad<4,1,20,g1>", "lean<4,1,20>", STEPS)),
    "lean_loop": (lambda: _cartpole(20), {**LEAN_WS, **LEAN_LOOP}, NEVER, None, True, ("quad<4,1,20,g1>", "lean<4,1,20>", 1)),
    "lean_loop_sequence_keeps_chain": (lambda: _cartpole(20), {**LEAN_WS, **LEAN_LOOP}, NEVER, _sequence(STEPS), True,
                                       ("quad<4,1,20,g1>", "lean<4,1,20>", STEPS)),
    "lean_off_per_instance_refs": (lambda: _cartpole(20), {**LEAN_WS, **LEAN_LOOP}, NEVER, _per_instance, True,
                                   ("quad<4,1,20,g1>", "quad<4,1,20,g1>", 1)),
    "stream_chain": (lambda: _cartpole(17), STREAM_MPC, FIXED, None, True, ("stream4<4,1>", "stream4<4,1>", STEPS)),
    "stream_loop": (lambda: _cartpole(17), {**STREAM_MPC, **STREAM_LOOP}, FIXED, None, True, ("stream4<4,1>", "stream4<4,1>", 1)),
    "generic_chain": (lambda: _cartpole(17), {**STREAM_MPC, **STREAM_LOOP, **NO_STREAM}, FIXED, None, True, ("generic", "generic", STEPS)),
    "stream_no_switch": (lambda: _cartpole(17), {}, FIXED, None, True, NO_KERNEL),
    "stream_loop_switch_alone": (lambda: _cartpole(17), STREAM_LOOP, FIXED, None, True, NO_KERNEL),
    "sequence_shorter_than_loop": (lambda: _cartpole(10), {}, FIXED, _sequence(STEPS - 1), True, SEQ_SHORT),
    "sequence_with_per_instance_refs": (lambda: _cartpole(10), {}, FIXED, _sequence_then_per_instance, True, SEQ_PER_INSTANCE),
}
_LOGS = {}


def _run(monkeypatch, name):
    """the case's solver through two rollouts; the first one's log is kept for the chain / loop comparisons"""
    make, env, kw, more, warm, want = CASES[name]
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob, x0 = make()
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    bs.update_settings(**kw)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if more:
        more(bs)
    bs.set_warm_start(warm)
    bs.set_x0(x0)
    assert _launches(bs) == -1
    for again in (False, True):
        if isinstance(want, str):
            with pytest.raises(t.TinyMPCError) as e:
                bs.mpc_rollout(STEPS)
            print(f"{name}: refused: {e.value}; launches {_launches(bs)}")
            assert str(e.value) == f"mpc_rollout failed ({want})", str(e.value)
            assert _launches(bs) == -1
        else:
            bs.set_x0(x0)
            log = bs.mpc_rollout(STEPS)
            got = (bs.kernel_name, bs.last_launch_name, _launches(bs))
            print(f"{name}: {got}")
            assert got == want, (got, want)
            assert np.all(log["iter"] == kw["max_iter"]) and np.abs(log["u"]).max() > 0.0
            if not again:
                _LOGS[name] = log
    bs.close()
    return _LOGS.get(name)


@pytest.mark.parametrize("name", list(CASES))
def test_route(hip_lib, monkeypatch, name):
    _run(monkeypatch, name)


@pytest.mark.parametrize("chain,loop", [("lean_chain", "lean_loop"), ("stream_chain", "stream_loop")])
def test_loop_log_is_the_chain_log(hip_lib, monkeypatch, chain, loop):
    a, c = (_LOGS.get(n) or _run(monkeypatch, n) for n in (loop, chain))
    for key in ("x", "u", "iter", "solved"):
        assert np.array_equal(a[key], c[key]), f"{loop} against {chain}: log {key}"
    assert a["status"] == c["status"]
