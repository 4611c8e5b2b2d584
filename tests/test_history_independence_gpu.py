"""Configuration history: a solver's result depends on its current configuration only, not on what it was configured for and
ran before (tests/independence_cases.py: HISTORY has the three routes, the target configuration T and the decoy).

Solver keeps about a dozen cached device images behind dirty flags — the coefficient pack, bounds, references, the plant image,
adaptive state, extension buffers, the routing key.  Per route a *used* solver is given the decoy, which differs from T in every
setter the route accepts, solves four times and rolls out once under it, is taken to T through the public API alone, reset, and
solved cold; a *fresh* solver receives T only.  Required: the same last_launch_name, np.array_equal on states, controls, iter,
solved and residuals, and after a further mpc_rollout the same log and metrics.  A second case per route: after two warm
solves, reset() followed by a solve equals the fresh solver's first warm solve, workspace included."""
import numpy as np
import pytest

from tests import independence_cases as ic
from tests.test_batch_independence_gpu import _env, _solution, make_solver

pytestmark = pytest.mark.gpu


def _route_env(monkeypatch, case):
    _env(monkeypatch, dict(env=case["env"], specialised=False))


def _install_decoy(bs, d, shared, per, case):
    """the four stages of the decoy: four solves and a rollout under it"""
    prob = shared["prob"]
    cache = bs.get_cache_terms()
    # (0) on T's own kernel: its pack, bound and reference images filled with other values, its workspace left behind
    bs.update_settings(**d["kw"])
    bs.set_bound_constraints(prob.x_min, prob.x_max, d["bounds"][2], d["bounds"][3])
    bs.set_x_ref(d["xref_same"])
    bs.set_u_ref(d["uref_same"])
    bs.set_cache_terms(1.05 * cache["Kinf"], 1.02 * cache["Pinf"], cache["Quu_inv"], 0.99 * cache["AmBKt"])
    bs.set_x0(d["x0"])
    for warm in (False, True):
        bs.set_warm_start(warm)
        bs.solve()
        assert bs.kernel_name == case["family"], f"the decoy's first solves are meant for T's own family, not {bs.kernel_name}"
    # (A) every shared setter with another value; adaptive rho, precision 1, compaction
    bs.set_bound_constraints(*d["bounds"])
    bs.set_x_ref(d["xref"])
    bs.set_u_ref(d["uref"])
    bs.set_fdyn(d["fdyn"])
    bs.set_cone_constraints(*d["cones"])
    bs.set_linear_constraints(*d["lin"])
    bs.set_adaptive_rho(True, **{k: d["adaptive"][k] for k in ("rho_min", "rho_max")}, enable_clipping=d["adaptive"]["clip"])
    bs.set_precision(1)
    bs.set_compaction(d["compaction"])
    bs.set_warm_start(True)
    bs.set_x0(d["x0"])
    bs.solve()
    first = bs.last_launch_name
    # (B) per-instance bounds (refused beside adaptive rho)
    bs.set_adaptive_rho(False)
    bs.set_instance_bounds(*d["ib"])
    assert bs.bounds_mode() == 1
    bs.solve()
    second = bs.last_launch_name
    # (C) the own-plant chain with everything it takes
    bs.set_bound_constraints(*d["bounds"])
    bs.set_compaction(0)
    bs.set_plant(*d["plant"])
    bs.set_disturbance(d["w"])
    bs.set_ref_trajectory(*d["traj"])
    bs.set_estimator(*d["est"])
    bs.set_process_noise(d["noise"]["gw"], d["noise"]["seed_w"])
    bs.set_measurement_noise(d["noise"]["gv"], d["noise"]["seed_v"])
    bs.set_rollout_metrics(True, **d["metrics"])
    log = bs.mpc_rollout(ic.STEPS)
    assert np.isfinite(log["u"]).all() and bs.get_rollout_metrics()[:, 0].min() == ic.STEPS
    print(f"HI decoy launches: {first}, {second}, rollout on {bs.last_launch_name}")
    return cache


def _to_target(bs, shared, per, kw, cache):
    """from the decoy to T, through the public API"""
    prob = shared["prob"]
    nx, nu, N = prob.nx, prob.nu, prob.N
    bs.set_plant(None, None)
    bs.set_disturbance(None)
    bs.set_ref_trajectory(None)
    bs.set_estimator(None)
    bs.set_process_noise(None)
    bs.set_measurement_noise(None)
    bs.set_rollout_metrics(False)
    bs.set_compaction(0)
    bs.set_precision(0)
    bs.set_adaptive_rho(False)
    bs.set_cache_terms(cache["Kinf"], cache["Pinf"], cache["Quu_inv"], cache["AmBKt"])
    bs.update_settings(**kw)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_fdyn(shared["fdyn"] if "fdyn" in shared else np.zeros(nx))
    if "cones" in shared:
        bs.set_cone_constraints(*shared["cones"])
    else:
        bs.set_cone_constraints([], [], [], [], [], [])
        assert bs.lib.tinympc_enable_cones(bs.h, 0, 0) == 0
    if "lin" in shared:
        bs.set_linear_constraints(*shared["lin"])
    else:
        bs.set_linear_constraints(np.zeros((0, nx)), [], np.zeros((0, nu)), [])
        bs.enable_linear(0, 0)
    if "xref" in per:
        bs.set_x_ref(per["xref"])
        bs.set_u_ref(per["uref"])
    elif "xref" in shared:
        bs.set_x_ref(shared["xref"])
        bs.set_u_ref(shared["uref"])
    else:
        bs.set_x_ref(np.zeros((nx, N)))
        bs.set_u_ref(np.zeros((nu, N - 1)))
    bs.set_rollout_metrics(True, **shared["metrics"])
    bs.reset()


def _cold_solve_and_rollout(bs, case, per, tag):
    out = {}
    bs.set_warm_start(False)
    bs.set_x0(per["x0"])
    bs.solve()
    assert bs.last_launch_name == case["kernel"], f"{tag}: the solve launched {bs.last_launch_name}"
    _solution(bs, out)
    bs.set_warm_start(True)
    log = bs.mpc_rollout(ic.STEPS)
    assert bs.last_launch_name == case["rollout_kernel"], f"{tag}: the rollout launched {bs.last_launch_name}"
    for k in ("x", "u", "iter", "solved"):
        out["log_" + k] = log[k]
    assert "xhat" not in log and "y" not in log
    out["metrics"] = bs.get_rollout_metrics()
    _solution(bs, out, "after_")
    return out


@pytest.mark.parametrize("case", ic.HISTORY, ids=lambda c: c["id"])
def test_used_solver_equals_fresh_solver(hip_lib, monkeypatch, case):
    _route_env(monkeypatch, case)
    shared, per = ic.target_of(case)
    kw = shared["kw"]["tol"]
    fresh = make_solver(shared, per, kw)
    want = _cold_solve_and_rollout(fresh, case, per, f"{case['id']} fresh")
    fresh.close()
    used = make_solver(shared, per, kw)       # (created like the fresh one; what follows is what it has been through)
    cache = _install_decoy(used, ic.decoy_of(shared, per), shared, per, case)
    _to_target(used, shared, per, kw, cache)
    assert (used.bounds_mode(), used.plant_mode(), used.estimator_mode(), used.noise_mode(), used.ref_trajectory_mode()) == (0, 0, 0, 0, 0)
    assert used.effective_precision == 0 and used.rollout_metrics_mode() == 1
    got = _cold_solve_and_rollout(used, case, per, f"{case['id']} used")
    used.close()
    it = want["iter"]
    print(f"HI {case['id']} | {case['kernel']} / {case['rollout_kernel']} | compared {len(it)} | iterations {it.min()}..{it.max()} ({len(np.unique(it))} distinct)")
    for key in want:
        assert np.array_equal(got[key], want[key]), \
            f"{case['id']}: {key} depends on the solver's history ({int(np.sum(got[key] != want[key]))} of {got[key].size} values differ)"


@pytest.mark.parametrize("case", ic.HISTORY, ids=lambda c: c["id"])
def test_reset_returns_to_the_first_warm_solve(hip_lib, monkeypatch, case):
    _route_env(monkeypatch, case)
    shared, per = ic.target_of(case)
    kw = shared["kw"]["tol"]
    x1 = np.asfortranarray(shared["prob"].A @ per["x0"])
    outs = []
    for before in ((), (per["x0"], x1)):
        bs = make_solver(shared, per, kw)
        bs.set_warm_start(True)
        for x in before:
            bs.set_x0(x)
            bs.solve()
        if before:
            bs.reset()
        bs.set_x0(per["x0"])
        bs.solve()
        out = dict(name=np.array([bs.last_launch_name]))
        _solution(bs, out)
        for k, v in bs.get_workspace().items():
            out["ws_" + k] = v
        outs.append(out)
        bs.close()
    for key in outs[0]:
        assert np.array_equal(outs[0][key], outs[1][key]), f"{case['id']}: {key} after reset() differs from a fresh solver's first warm solve"
