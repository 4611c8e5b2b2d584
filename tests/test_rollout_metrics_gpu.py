"""Per-instance closed-loop metrics folded on the device (BatchSolver.set_rollout_metrics; csrc/metrics.hip) behind every route
of mpc_rollout, against a numpy fp64 restatement of the rule (tests/test_rollout_metrics.py) applied to what get_mpc_log
returns and to the references this file installed, rounded to fp32 as the setters round — never to the device's own metrics.
(The logs themselves are held to the oracle by the existing closed-loop tests.)

Tolerances, as on the host: slots 0 and 3..10 are counts, maxima and comparisons of exactly representable values and are EXACT,
per instance and — minimum, maximum, count — in the summary; the sums (slots 1, 2 per instance; the summary's sum column) are
within 1e-12 * max(1, sum |value|): an fp64 sum of a few hundred non-negative terms is off by at most ~1e-13 relative in any
order.  The summary kernel itself is also held exactly to the device's own per-instance array (min, max, count of every slot).

Limits, so that nothing passes vacuously (asserted on the numpy side): x_lo / x_hi are per-row quantiles of a dry run's log —
the first of a fixed list of quantiles at which 10 % .. 90 % of the instances leave the set and first_viol takes at least two
distinct non-zero values; u_lo / u_hi are the solver's input bounds, with a saturated and an unsaturated step; the tolerance
cases hold both signs of the logged iteration count.

 (a) cartpole N = 20, its default fused loop (one launch), shared constant references
 (b) cartpole N = 20, a per-instance trajectory cut short (the clamp is live) from cursor 2, both noises: the chain
 (c) quadrotor N = 10 on the matrix-core chain, a reference sequence, fixed iterations
 (d) cartpole N = 17 on the generic kernel at precision 2
 (e) the lean kernel's chain and in-kernel loop; the stream kernel's chain and in-kernel loop, whose logs are bit-equal and whose
     metrics therefore are
 (f) steps = 1, 2, 3 (the fold's narrower forms); 3 + 2 steps against 5; a reset between two rollouts; run-to-run identity
 (g) enabling changes nothing else; disabling, set_precision, the refusals; the global forms with re-batching and set_gpus

Batch 70 (neither 64 nor 256 / nx divides it), 5 steps.  Every test fails without the feature: the setters do not exist there."""
import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.test_noise_loop_gpu import _diag
from tests.test_ref_sequence import quadrotor_tracking_refs
from tests.test_rollout_metrics import EXACT, NAMES, SUM_TOL, SUMS, check_slots, restated
from tests.test_stream_loop_gpu import _collect, _identical, _launches, _tol

pytestmark = pytest.mark.gpu

B, STEPS = 70, 5
SWITCHES = ("TINYMPC_HIP_STREAM_MPC", "TINYMPC_HIP_STREAM_LOOP", "TINYMPC_HIP_NO_STREAM", "TINYMPC_HIP_STREAM_F64", "TINYMPC_HIP_NO_MFMAT",
            "TINYMPC_HIP_LEAN_WS", "TINYMPC_HIP_LEAN_LOOP", "TINYMPC_HIP_GROUP", "TINYMPC_HIP_NOISE_SPLIT")
QUANTILES = (0.25, 0.15, 0.08, 0.04, 0.02, 0.01)
CURSOR = 2


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def _cartpole(N=20):
    prob = t.problems.cartpole(N, u_bound=0.5)
    return dict(prob=prob, x0=t.problems.cartpole_x0(B, seed=7), kw=_tol(8), both_signs=True)


def _fused():
    c = _cartpole()
    N = c["prob"].N
    xref = np.zeros((4, N), order="F")
    xref[0], xref[1] = np.linspace(0.05, 0.2, N), 0.01          # (knot 1 is not knot 0: the fold has to take the right one)
    uref = np.asfortranarray(np.linspace(0.02, -0.02, N - 1)[None, :])
    return dict(c, refs=(xref, uref), launches=lambda n: 1, name="quad<4,1,20")


def _trajectory():
    c = _cartpole()
    rng = np.random.default_rng(41)
    Lx, Lu = CURSOR + STEPS - 1, CURSOR + STEPS - 2              # rows c + s + 1 <= c + 5 and c + s <= c + 4: the last steps clamp
    amp, phase = rng.uniform(0.05, 0.3, B), rng.uniform(0.0, 2.0 * np.pi, B)
    wave = np.sin(0.15 * np.arange(Lx)[:, None] + phase[None, :])
    xt, ut = np.zeros((4, Lx, B), order="F"), np.zeros((1, Lu, B), order="F")
    xt[0], ut[0] = amp[None, :] * wave, 0.05 * amp[None, :] * wave[:Lu]
    return dict(c, traj=(xt, ut), gw=_diag(c["x0"]), gv=_diag(c["x0"], True, 1), launches=lambda n: n)


def _quadrotor():
    prob = t.problems.quadrotor(10)
    kw = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=10, check_termination=1)
    return dict(prob=prob, x0=t.problems.quadrotor_x0(B, seed=5), kw=kw, seq=quadrotor_tracking_refs(10, STEPS), launches=lambda n: n, name="mfma")


def _generic_p2():
    c = _cartpole(17)
    return dict(c, kw=_tol(12), precision=2, env={"TINYMPC_HIP_NO_STREAM": "1", "TINYMPC_HIP_STREAM_MPC": "1"}, launches=lambda n: n, name="generic")


def _lean(loop):
    c = _cartpole()
    env = {"TINYMPC_HIP_LEAN_WS": "1", "TINYMPC_HIP_GROUP": "1"}
    if loop:
        env["TINYMPC_HIP_LEAN_LOOP"] = "1"
    return dict(c, env=env, launches=(lambda n: 1) if loop else (lambda n: n), name="lean<4,1,20>")


def _stream(loop):
    c = _cartpole(17)
    env = {"TINYMPC_HIP_STREAM_MPC": "1"}
    if loop:
        env["TINYMPC_HIP_STREAM_LOOP"] = "1"
    return dict(c, kw=_tol(12), env=env, launches=(lambda n: 1) if loop else (lambda n: n), name="stream4<4,1>")


CASES = dict(fused=_fused, trajectory_noise=_trajectory, quadrotor_sequence=_quadrotor, generic_p2=_generic_p2, lean_chain=lambda: _lean(False),
             lean_loop=lambda: _lean(True), stream_chain=lambda: _stream(False), stream_loop=lambda: _stream(True))
_CASE_CACHE, _RUNS = {}, {}


def _case(name):
    if name not in _CASE_CACHE:
        _CASE_CACHE[name] = dict(CASES[name](), id=name)
    return _CASE_CACHE[name]


def _solver(monkeypatch, case):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in case.get("env", {}).items():
        monkeypatch.setenv(name, v)
    prob = case["prob"]
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    bs.update_settings(**case["kw"])
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(True)
    if case.get("precision"):
        bs.set_precision(case["precision"])
    if "refs" in case:
        bs.set_x_ref(case["refs"][0])
        bs.set_u_ref(case["refs"][1])
    if "seq" in case:
        bs.set_ref_sequence(*case["seq"])
    if "traj" in case:
        bs.set_ref_trajectory(*case["traj"])
        bs.set_ref_cursor(CURSOR)
    if "gw" in case:
        bs.set_process_noise(case["gw"], 0x1234_5678_9ABC_DEF1)
        bs.set_measurement_noise(case["gv"], 77)
    return bs


def _run(monkeypatch, case, parts=(STEPS,), cfg=None, reset_between=False, keep=True):
    """mpc_rollout of every part in turn on one solver; cfg: the metric configuration (None: no metrics).  Returns the logs,
    what the solver left, and — with metrics — the per-instance array and the summary after the last part"""
    key = (case["id"], tuple(parts), None if cfg is None else tuple(sorted((k, None if v is None else tuple(v)) for k, v in cfg.items())), reset_between)
    if keep and key in _RUNS:
        return _RUNS[key]
    bs = _solver(monkeypatch, case)
    if cfg is not None:
        assert bs.rollout_metrics_mode() == 0
        bs.set_rollout_metrics(True, **cfg)
        assert bs.rollout_metrics_mode() == 1
        assert not bs.get_rollout_metrics().any() and not bs.get_rollout_summary().any()      # (zeros before any rollout)
    bs.set_x0(case["x0"])
    logs = []
    for i, n in enumerate(parts):
        if i and reset_between:
            bs.reset_rollout_metrics()
        logs.append(bs.mpc_rollout(n))
        assert _launches(bs) == case["launches"](n), (_launches(bs), n)
        if "name" in case:
            assert case["name"] in bs.last_launch_name, bs.last_launch_name
    out = _collect(bs, logs[-1])
    out["logs"], out["launches"] = logs, _launches(bs)
    if cfg is not None:
        out["metrics"], out["summary"] = bs.get_rollout_metrics(), bs.get_rollout_summary()
        assert bs.get_rollout_summary(as_dict=True)["steps"]["sum"] == out["summary"][0, 0]
    bs.close()
    if keep:
        _RUNS[key] = out
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy side
# ---------------------------------------------------------------------------------------------------------------------------
def _targets(case, b, s0, n, cursor):
    """(xr, ur) of instance b for the loop steps s0 .. s0 + n - 1 of one rollout that started at reference cursor `cursor`: (n, nx), (n, nu)"""
    prob = case["prob"]
    if "refs" in case:
        return np.tile(_f32(case["refs"][0][:, 1]), (n, 1)), np.tile(_f32(case["refs"][1][:, 0]), (n, 1))
    if "seq" in case:
        xs, us = case["seq"]
        return _f32(xs[:, 1, s0:s0 + n].T), _f32(us[:, 0, s0:s0 + n].T)
    if "traj" in case:
        xt, ut = case["traj"]
        s = np.arange(s0, s0 + n)
        return (_f32(xt[:, np.minimum(cursor + s + 1, xt.shape[1] - 1), b].T), _f32(ut[:, np.minimum(cursor + s, ut.shape[1] - 1), b].T))
    return None, None


def _signed(log):
    return np.where(log["solved"] > 0, log["iter"], -log["iter"])


def _weights(case):
    return np.diag(case["prob"].Q).copy(), np.diag(case["prob"].R).copy()


def _numpy_metrics(case, logs, cfg, reset_between=False):
    """the restated rule over the logs of consecutive rollouts of one solver: (B, 11)"""
    c = dict(cfg)
    qw, rw = c.pop("qw", None), c.pop("rw", None)
    if qw is None or rw is None:                       # (null weights: the diagonal of the solver's Q / R)
        dq, dr = _weights(case)
        qw, rw = dq if qw is None else qw, dr if rw is None else rw
    out = np.zeros((B, 11))
    for b in range(B):
        acc, cursor = None, CURSOR
        for i, log in enumerate(logs):
            n = log["iter"].shape[0]
            if i and reset_between:
                acc = None
            xr, ur = _targets(case, b, 0, n, cursor)
            acc = restated(log["x"][:, :, b].T, log["u"][:, :, b].T, _signed(log)[:, b], qw, rw, xr=xr, ur=ur, acc=acc, **c)
            cursor += n
        out[b] = acc
    return out


def _limits(case, log, late=0):
    """the metric configuration of a case from a dry run's log: per-row quantiles for x, the solver's input bounds for u;
    late: some instance has to leave the set for the first time after that many steps"""
    prob = case["prob"]
    x = log["x"]
    for q in QUANTILES:
        lo, hi = np.quantile(x, q, axis=(1, 2)), np.quantile(x, 1.0 - q, axis=(1, 2))
        out = ((x > hi[:, None, None]) | (x < lo[:, None, None])).any(axis=0)          # (steps, B)
        share = out.any(axis=0).mean()
        first = np.where(out.any(axis=0), out.argmax(axis=0) + 1, 0)
        if 0.1 <= share <= 0.9 and len(set(first[first > 0])) >= 2 and (first > late).any():
            return dict(x_lo=lo, x_hi=hi, u_lo=prob.u_min[:, 0].copy(), u_hi=prob.u_max[:, 0].copy())
    raise AssertionError(f"{case['id']}: no quantile of {QUANTILES} gives a live safe set")


def _not_vacuous(case, want, logs):
    share = (want[:, 6] > 0).mean()
    firsts = set(want[:, 7][want[:, 7] > 0])
    print(f"{case['id']}: {share:.2f} of the instances leave the safe set, first_viol values {sorted(firsts)}, saturated steps {want[:, 8].sum():.0f} of "
          f"{want[:, 0].sum():.0f}, max_iter steps {want[:, 10].sum():.0f}")
    assert 0.1 <= share <= 0.9 and len(firsts) >= 2, (share, firsts)
    assert 0 < want[:, 8].sum() < want[:, 0].sum()                                       # a saturated and an unsaturated step
    if case.get("both_signs"):
        it = np.concatenate([_signed(l) for l in logs], axis=0)
        assert (it > 0).any() and (it < 0).any()
    assert (want[:, 1] > 0).all() and (want[:, 3] > 0).all()


def _summary_of(m):
    return np.stack([m.sum(axis=0), m.min(axis=0), m.max(axis=0), (m > 0).sum(axis=0).astype(np.float64)], axis=1)      # (11, 4)


def _check_summary(got, device_metrics, want_metrics, tag):
    own, want = _summary_of(device_metrics), _summary_of(want_metrics)
    # the summary kernel against the device's own array: minimum, maximum and count of every slot to the bit
    assert np.array_equal(got[:, 1:], own[:, 1:]), f"{tag}: summary min / max / count against the per-instance array"
    # ... and against the restatement: the exact slots to the bit, the two cost slots within the bound
    for k in EXACT:
        assert np.array_equal(got[k, 1:], want[k, 1:]), f"{tag}: summary of slot {k} ({NAMES[k]}): {got[k]} vs {want[k]}"
    for k in SUMS:
        assert got[k, 3] == want[k, 3] and np.all(np.abs(got[k, 1:3] - want[k, 1:3]) <= SUM_TOL * np.maximum(1.0, np.abs(want[k, 1:3]))), (tag, k)
    bound = SUM_TOL * np.maximum(1.0, np.abs(want_metrics).sum(axis=0))
    d = np.abs(got[:, 0] - want[:, 0])
    print(f"{tag}: summary sums, worst |delta| / bound = {np.max(d / bound):.3e}")
    assert np.all(d <= bound), f"{tag}: summary sums {d / bound}"


def _scored(monkeypatch, case, parts=(STEPS,), reset_between=False, extra=None):
    """a dry run for the limits (the first part list's total as one rollout), the run with metrics, the restatement"""
    dry = _run(monkeypatch, case, (STEPS,))
    cfg = dict(_limits(case, dry["logs"][0]), **(extra or {}))
    run = _run(monkeypatch, case, parts, cfg, reset_between)
    want = _numpy_metrics(case, run["logs"], cfg, reset_between)
    return dry, cfg, run, want


# ---------------------------------------------------------------------------------------------------------------------------
# (a) - (e) every route against the restatement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_route_against_the_restatement(hip_lib, monkeypatch, name):
    case = _case(name)
    dry, cfg, run, want = _scored(monkeypatch, case)
    _not_vacuous(case, want, run["logs"])
    assert np.all(run["metrics"][:, 0] == STEPS)
    check_slots(run["metrics"], want, name)
    _check_summary(run["summary"], run["metrics"], want, name)
    # enabling the metrics changed nothing else: log, last solution, status, workspace, x0, launch count
    _identical(dict(run, log=run["logs"][0]), dict(dry, log=dry["logs"][0]), name + ": with and without metrics")
    assert run["launches"] == dry["launches"]


def test_trajectory_clamp_is_live():
    case = _case("trajectory_noise")
    xt, ut = case["traj"]
    assert CURSOR + STEPS > xt.shape[1] - 1 and CURSOR + STEPS - 1 > ut.shape[1] - 1
    a, b = _targets(case, 3, 0, STEPS, CURSOR), _targets(case, 3, 0, STEPS, 0)
    assert np.array_equal(a[0][-1], a[0][-2]) and not np.array_equal(a[0], b[0])      # held beyond the end; the cursor matters


def test_stream_loop_metrics_are_the_chains(hip_lib, monkeypatch):
    """the stream kernel's in-kernel loop and its chain write bit-equal logs (tests/test_stream_loop_gpu.py), so the fold gives
    bit-equal metrics and summary; the lean loop's log is its own (compared at a tolerance there): it is held to the restatement above"""
    chain, loop = _scored(monkeypatch, _case("stream_chain")), _scored(monkeypatch, _case("stream_loop"))
    for key in ("x", "u", "iter", "solved"):
        assert np.array_equal(chain[2]["logs"][0][key], loop[2]["logs"][0][key]), key
    assert np.array_equal(chain[2]["metrics"], loop[2]["metrics"]) and np.array_equal(chain[2]["summary"], loop[2]["summary"])
    assert chain[2]["launches"] == STEPS and loop[2]["launches"] == 1


# ---------------------------------------------------------------------------------------------------------------------------
# (f) short loops, continuation, reset, identity
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("name", ["fused", "trajectory_noise"])
def test_short_loops(hip_lib, monkeypatch, name, steps):
    case = _case(name)
    cfg = _limits(case, _run(monkeypatch, case, (STEPS,))["logs"][0])
    run = _run(monkeypatch, case, (steps,), cfg)
    want = _numpy_metrics(case, run["logs"], cfg)
    assert np.all(run["metrics"][:, 0] == steps) and np.array_equal(run["metrics"][:, 3] >= run["metrics"][:, 4], np.ones(B, dtype=bool))
    check_slots(run["metrics"], want, f"{name}, {steps} steps")
    _check_summary(run["summary"], run["metrics"], want, f"{name}, {steps} steps")


@pytest.mark.parametrize("name", ["fused", "quadrotor_sequence"])
def test_two_rollouts_accumulate(hip_lib, monkeypatch, name):
    """3 then 2 steps on one solver, held to the restatement continued over the two logs (a reference sequence restarts at slice 0
    with every rollout, so its 3 + 2 steps track other targets than 5 steps would)"""
    case = _case(name)
    dry, cfg, split, want = _scored(monkeypatch, case, (3, 2))
    assert np.all(split["metrics"][:, 0] == 5)
    check_slots(split["metrics"], want, name + " 3 + 2")
    _check_summary(split["summary"], split["metrics"], want, name + " 3 + 2")


def test_three_plus_two_steps_are_five(hip_lib, monkeypatch):
    """two rollouts in a row continue the plant state, the trajectory and the noise streams (tests/test_noise_loop_gpu.py: the joined
    log is the 5-step log to the bit) — and the statistics: exact slots equal, sums within the bound, first_viol counted since the reset"""
    case = _case("trajectory_noise")
    dry = _run(monkeypatch, case, (STEPS,))
    cfg = _limits(case, dry["logs"][0], late=3)
    whole, split = _run(monkeypatch, case, (STEPS,), cfg), _run(monkeypatch, case, (3, 2), cfg)
    for k in ("x", "u", "iter", "solved"):
        assert np.array_equal(np.concatenate([l[k] for l in split["logs"]], axis=0 if k in ("iter", "solved") else 1), whole["logs"][0][k]), k
    want = _numpy_metrics(case, whole["logs"], cfg)
    assert (want[:, 7] > 3).any(), "no instance leaves the safe set for the first time in the second rollout"
    check_slots(whole["metrics"], want, "5 steps")
    check_slots(split["metrics"], want, "3 + 2 steps against the restatement of 5")
    check_slots(split["metrics"], whole["metrics"], "3 + 2 steps against 5 steps", scale=np.abs(want))
    assert np.array_equal(split["metrics"][:, 7], whole["metrics"][:, 7]) and np.all(split["metrics"][:, 0] == 5)


def test_reset_between_two_rollouts(hip_lib, monkeypatch):
    case = _case("trajectory_noise")
    cfg = _limits(case, _run(monkeypatch, case, (STEPS,))["logs"][0])
    run = _run(monkeypatch, case, (3, 2), cfg, reset_between=True)
    want = _numpy_metrics(case, run["logs"], cfg, reset_between=True)       # the second rollout alone (its targets from cursor 2 + 3)
    assert np.all(run["metrics"][:, 0] == 2) and run["metrics"][:, 7].max() <= 2
    check_slots(run["metrics"], want, "after a reset")
    _check_summary(run["summary"], run["metrics"], want, "after a reset")


def test_two_identical_runs_give_identical_bits(hip_lib, monkeypatch):
    case = _case("trajectory_noise")
    cfg = _limits(case, _run(monkeypatch, case, (STEPS,))["logs"][0])
    a, b = _run(monkeypatch, case, (STEPS,), cfg, keep=False), _run(monkeypatch, case, (STEPS,), cfg, keep=False)
    assert np.array_equal(a["metrics"], b["metrics"]) and np.array_equal(a["summary"], b["summary"])
    assert a["summary"].tobytes() == b["summary"].tobytes()


def test_own_weights(hip_lib, monkeypatch):
    """weights of the caller's instead of diag(Q), diag(R); one limit side only"""
    case = _case("fused")
    lim = _limits(case, _run(monkeypatch, case, (STEPS,))["logs"][0])
    cfg = dict(qw=np.array([3.0, 0.0, 0.5, 7.0]), rw=np.array([0.25]), x_hi=lim["x_hi"], u_lo=lim["u_lo"], x_lo=None, u_hi=None)
    run = _run(monkeypatch, case, (STEPS,), cfg)
    check_slots(run["metrics"], _numpy_metrics(case, run["logs"], cfg), "own weights")


# ---------------------------------------------------------------------------------------------------------------------------
# (g) the switch itself
# ---------------------------------------------------------------------------------------------------------------------------
def test_disable_precision_and_refusals(hip_lib, monkeypatch):
    case = _case("fused")
    cfg = _limits(case, _run(monkeypatch, case, (STEPS,))["logs"][0])
    bs = _solver(monkeypatch, case)
    for call in (bs.get_rollout_metrics, bs.get_rollout_summary, bs.reset_rollout_metrics):      # off: refused, by name
        with pytest.raises(t.TinyMPCError, match="not enabled"):
            call()
    for bad, word in ((dict(qw=[1.0, 1.0, -1.0, 1.0]), "negative"), (dict(rw=[-1.0]), "negative"), (dict(x_lo=[0.0, 0.0, 1.0, 0.0], x_hi=[1.0, 1.0, 0.5, 1.0]), "x_lo > x_hi in row 2"),
                      (dict(u_lo=[0.5], u_hi=[-0.5]), "u_lo > u_hi"), (dict(qw=[1.0, 1.0]), "expected 4 values")):
        with pytest.raises(t.TinyMPCError, match=word):
            bs.set_rollout_metrics(True, **bad)
        assert bs.rollout_metrics_mode() == 0
    bs.set_rollout_metrics(True, **cfg)
    bs.set_x0(case["x0"])
    bs.mpc_rollout(STEPS)
    m = bs.get_rollout_metrics()
    assert np.all(m[:, 0] == STEPS)
    with pytest.raises(t.TinyMPCError, match="negative"):        # a refused replacement leaves configuration and accumulators alone
        bs.set_rollout_metrics(True, qw=[-1.0, 0.0, 0.0, 0.0])
    assert bs.rollout_metrics_mode() == 1 and np.array_equal(bs.get_rollout_metrics(), m)
    bs.set_precision(1)                                           # keeps both
    assert bs.rollout_metrics_mode() == 1 and np.array_equal(bs.get_rollout_metrics(), m)
    bs.set_precision(0)
    bs.set_rollout_metrics(True, **cfg)                           # replacing zeroes the accumulators
    assert not bs.get_rollout_metrics().any()
    bs.set_rollout_metrics(False)
    assert bs.rollout_metrics_mode() == 0
    with pytest.raises(t.TinyMPCError, match="not enabled"):
        bs.get_rollout_metrics()
    bs.set_x0(case["x0"])
    bs.mpc_rollout(STEPS)                                         # ... and the loop runs as before
    assert _launches(bs) == 1
    bs.close()
    # a per-instance-family solver has no one Q and R: null weights are refused, given ones taken
    base = t.problems.cartpole(17, u_bound=0.5)
    fam = tuple(np.asfortranarray(np.repeat(m_[:, :, None], B, axis=2)) for m_ in (base.A, base.B, base.Q, base.R)) + (np.full(B, base.rho),)
    hs = t.BatchSolver.from_families(*fam, base.N)
    with pytest.raises(t.TinyMPCError, match="per-instance-family"):
        hs.set_rollout_metrics(True)
    hs.set_rollout_metrics(True, qw=np.ones(4), rw=np.ones(1))
    assert hs.rollout_metrics_mode() == 1
    hs.close()


def test_global_forms(hip_lib, monkeypatch):
    """the process-global solver: set, rollout, get, reset; re-batching drops the metrics; refused under set_gpus"""
    case = _case("fused")
    dry = _run(monkeypatch, case, (STEPS,))
    cfg = _limits(case, dry["logs"][0])
    ref = _run(monkeypatch, case, (STEPS,), cfg)
    for name in SWITCHES + ("TINYMPC_HIP_SHARD_DEVICES",):
        monkeypatch.delenv(name, raising=False)
    prob = case["prob"]
    s = t.TinyMPCSolver()
    try:
        t.setup(s, prob.A, prob.B, None, prob.Q, prob.R, prob.rho, 4, 1, prob.N, batch=B, **case["kw"])
        t.set_bound_constraints(s, prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        t.set_x_ref(s, case["refs"][0])
        t.set_u_ref(s, case["refs"][1])
        with pytest.raises(t.TinyMPCError, match="not enabled"):
            t.get_rollout_metrics(s)
        with pytest.raises(t.TinyMPCError, match="expected 4 values"):
            t.set_rollout_metrics(s, True, qw=np.ones(5))
        t.set_rollout_metrics(s, True, **cfg)
        t.set_x0(s, case["x0"])
        log = t.mpc_rollout(s, STEPS)
        for key in ("x", "u", "iter", "solved"):
            assert np.array_equal(log[key], ref["logs"][0][key]), key
        assert np.array_equal(t.get_rollout_metrics(s), ref["metrics"]) and np.array_equal(t.get_rollout_summary(s), ref["summary"])
        assert t.get_rollout_summary(s, as_dict=True)["steps"] == dict(sum=float(B * STEPS), min=float(STEPS), max=float(STEPS), count=float(B))
        t.reset_rollout_metrics(s)
        assert not t.get_rollout_metrics(s).any()
        t.set_batch_size(s, B + 3)                                # re-batching drops configuration and accumulators
        with pytest.raises(t.TinyMPCError, match="not enabled"):
            t.get_rollout_summary(s)
        t.set_rollout_metrics(s, True, **cfg)
        assert t.get_rollout_metrics(s).shape == (B + 3, 11)
        t.set_rollout_metrics(s, False)
        monkeypatch.setenv("TINYMPC_HIP_SHARD_DEVICES", "0,0")
        t.set_gpus(s, 2)
        for call, word in ((lambda: t.set_rollout_metrics(s, True, **cfg), "set_rollout_metrics"), (lambda: t.reset_rollout_metrics(s), "reset_rollout_metrics"),
                           (lambda: t.get_rollout_metrics(s), "get_rollout_metrics"), (lambda: t.get_rollout_summary(s), "get_rollout_summary")):
            with pytest.raises(t.TinyMPCError, match=word + ": not available on a sharded solver"):
                call()
    finally:
        t.cleanup()
