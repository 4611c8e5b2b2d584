"""Batch independence, bit for bit, on every kernel family: an instance's result does not depend on where it sits in the batch,
on its neighbours or on the batch size (tests/independence_cases.py has the route table, the inputs and the three arrangements;
tests/test_independence_inputs.py the conditions on the inputs, on the oracles alone).

Per route and per setting (tolerance-terminated with check_termination = 1, so that instances leave at different iterations, and
fixed iterations, which takes the UNI and fixed forms): the base batch is run once, then permuted, with its neighbours replaced by
hard and trivial instances, and truncated.  The compared instances must equal the base run with np.array_equal on states,
controls, iter, solved and the per-instance residuals; on get_workspace() after the second solve of the kept-workspace routes;
on the logs (x, u, iter, solved, estimate, outputs, measurement) and the eleven metric slots of the rollouts; on
get_adaptive_state() of the adaptive routes.  The global status and get_rollout_summary are folds over the batch and are not
compared.  Every run asserts kernel_name, last_launch_name and — lean routes — the hook tmpc_lean_last_scaled: a comparison is of
two runs of one kernel.

Oracle anchor: the tolerance-terminated base run's S instances go through parity_every_instance against orc64 at FP32_TOL (the
first solve of the kept-workspace routes; the applied control of step 0 of the rollouts, on the instances whose exit agrees), so a
kernel that is wrong the same way in every arrangement still fails.  The noise routes' first solve starts from a measurement
drawn on the device and has no anchor here (tests/test_noise_loop_gpu.py, tests/test_estimator_loop_gpu.py hold those loops to
the oracle).  Hard instances are outside what fp32 state is documented to reach: they must be finite
and solved == 0.

Each route prints "BI <route> | <setting> | <kernel> | <arrangement>: compared .. | iterations lo..hi (n distinct)" per arrangement
(profiles/independence_routes.txt holds a run's figures)."""
import ctypes
import os

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests import independence_cases as ic
from tests.util import FP32_TOL, nrel_batch, parity_every_instance

pytestmark = pytest.mark.gpu


def _scaled(bs):
    f = ctypes.CDLL(t.LIB_PATH).tmpc_lean_last_scaled
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p]
    return f(bs.h)


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    """the cache of the specialised route's kernel: TINYMPC_TEST_JIT_CACHE where the suite's other specialisation tests are given
    one, else a directory of this module's own (every run of the route after the first loads what the first compiled)"""
    return os.environ.get("TINYMPC_TEST_JIT_CACHE") or str(tmp_path_factory.mktemp("jit_cache"))


def _env(monkeypatch, route, cache=None):
    for name in ic.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in route["env"].items():
        monkeypatch.setenv(name, v)
    if route["specialised"]:      # (tests/test_mfmat_general_gpu.py's arrangement: specialisation on, with a cache)
        os.makedirs(cache, exist_ok=True)
        monkeypatch.delenv("TINYMPC_HIP_NO_JIT", raising=False)
        monkeypatch.setenv("TINYMPC_HIP_CACHE", os.path.abspath(cache))


def make_solver(shared, per, kw):
    """a solver configured with a batch's shared and per-instance inputs"""
    prob, B = shared["prob"], per["x0"].shape[-1]
    if "fam_A" in per:
        bs = t.BatchSolver.from_families(per["fam_A"], per["fam_B"], per["fam_Q"], per["fam_R"], per["fam_rho"], prob.N)
    else:
        bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    bs.update_settings(**kw)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if "ib_umin" in per:
        bs.set_instance_bounds(per["ib_xmin"], per["ib_xmax"], per["ib_umin"], per["ib_umax"])
    if "fdyn" in shared:
        bs.set_fdyn(shared["fdyn"])
    if "cones" in shared:
        bs.set_cone_constraints(*shared["cones"])
    if "lin" in shared:
        bs.set_linear_constraints(*shared["lin"])
    if "xref" in shared:
        bs.set_x_ref(shared["xref"])
        bs.set_u_ref(shared["uref"])
    if "xref" in per:
        bs.set_x_ref(per["xref"])
        bs.set_u_ref(per["uref"])
    if "adaptive" in shared:
        a = shared["adaptive"]
        bs.set_sensitivity(*a["sens"])
        bs.set_adaptive_rho(True, a["rho_min"], a["rho_max"], a["clip"])
    if shared.get("precision"):
        bs.set_precision(shared["precision"])
    if "plant_A" in per:
        bs.set_plant(per["plant_A"], per["plant_B"], per["plant_f"])
    if "w" in per:
        bs.set_disturbance(per["w"])
    if "traj_x" in per:
        bs.set_ref_trajectory(per["traj_x"], per["traj_u"])
    if "traj" in shared:
        bs.set_ref_trajectory(*shared["traj"])
    if "est_C" in per:
        bs.set_estimator(per["est_C"], per["est_L"])
    if "noise" in shared:
        n = shared["noise"]
        bs.set_process_noise(n["gw"], n["seed_w"])
        bs.set_measurement_noise(n["gv"], n["seed_v"])
    if "metrics" in shared:
        bs.set_rollout_metrics(True, **shared["metrics"])
    return bs


def _names(bs, route, tag):
    got = (bs.kernel_name, bs.last_launch_name)
    if route["specialised"]:
        assert got[0].startswith(route["family"]) and got[1].startswith(route["kernel"]), f"{tag}: routed to {got}"
    else:
        assert got == (route["family"], route["kernel"]), f"{tag}: routed to {got}, the route is {(route['family'], route['kernel'])}"
    if route["scaled"] is not None:
        assert _scaled(bs) == route["scaled"], f"{tag}: tmpc_lean_last_scaled {_scaled(bs)}"


def _solution(bs, out, prefix=""):
    sol, st = bs.get_solution(), bs.get_status()
    out[prefix + "states"], out[prefix + "controls"] = sol["states"], sol["controls"]
    out[prefix + "iter"], out[prefix + "solved"] = st["iter"], st["solved"]
    out[prefix + "residuals"] = np.ascontiguousarray(st["residuals"].T)


def run(monkeypatch, route, shared, per, setting, tag, cache=None):
    """one run of a route on a batch: every per-instance output, the instance on the last axis"""
    _env(monkeypatch, route, cache)
    bs = make_solver(shared, per, shared["kw"][setting])
    out = {}
    if route["pattern"] == "oneshot":
        bs.set_warm_start(False)
        bs.set_x0(per["x0"])
        bs.solve()
        _names(bs, route, tag)
        _solution(bs, out)
    elif route["pattern"] == "kept2":
        bs.set_warm_start(True)
        bs.set_x0(per["x0"])
        bs.solve()
        _names(bs, route, tag)
        _solution(bs, out, "first_")
        bs.set_x0(np.asfortranarray(shared["prob"].A @ per["x0"]))
        bs.solve()
        _names(bs, route, tag)
        _solution(bs, out)
        for k, v in bs.get_workspace().items():
            out["ws_" + k] = v
    else:
        bs.set_warm_start(True)
        bs.set_x0(per["x0"])
        log = bs.mpc_rollout(ic.STEPS)
        _names(bs, route, tag)
        for k in ("x", "u", "iter", "solved", "xhat", "yout", "y"):
            if k in log:
                out["log_" + k] = log[k]
        _solution(bs, out)
        if "metrics" in shared:
            out["metrics"] = np.ascontiguousarray(bs.get_rollout_metrics().T)
        if "est_C" in per:
            out["estimate"] = bs.get_estimator_state()
    if "adaptive" in shared:
        for k, v in bs.get_adaptive_state().items():
            out["adapt_" + k] = v
    bs.close()
    return out


def _anchor(route, shared, per, base, tag):
    """the base run's S instances against orc64 at FP32_TOL"""
    if "noise" in shared:
        return
    kw = shared["kw"]["tol"]
    keep = ic.kept_set(route["B"], ic.GEOMETRY[route["geom"]])
    ref = ic.oracle_on_kept(route, "tol", "orc64")
    rho = shared["adaptive"]["rho_max"] if "adaptive" in shared else (float(np.max(per["fam_rho"])) if "fam_rho" in per else shared["prob"].rho)
    if route["pattern"] == "rollout":
        it, so = base["log_iter"][0][keep], base["log_solved"][0][keep]
        agree = (it == ref["iter"]) & (so == ref["solved"])
        eu = np.abs(base["log_u"][:, 0, keep] - ref["u"][:, 0, :]).max(axis=0) / np.abs(ref["u"]).max(axis=(0, 1)).clip(1e-300)
        print(f"BI {route['id']} | anchor | step 0 control off by {eu[agree].max():.2e} on {int(agree.sum())} of {len(keep)}")
        assert agree.mean() >= 0.9, f"{tag}: {int((~agree).sum())} of {len(keep)} exits of step 0 differ from the oracle's"
        assert eu[agree].max() <= FP32_TOL, f"{tag}: step 0's control off by {eu[agree].max():.3e}"
        return
    p = "first_" if route["pattern"] == "kept2" else ""
    sol = dict(states=base[p + "states"][:, :, keep], controls=base[p + "controls"][:, :, keep])
    st = dict(iter=base[p + "iter"][keep], solved=base[p + "solved"][keep])
    same = (st["iter"] == ref["iter"]) & (st["solved"] == ref["solved"])
    ex, eu = nrel_batch(sol["states"], ref["x"])[same], nrel_batch(sol["controls"], ref["u"])[same]
    print(f"BI {route['id']} | anchor | x {ex.max():.2e} u {eu.max():.2e} same {same.mean():.3f}")
    parity_every_instance(sol, st, ref, lambda j: ic.oracle_solver(shared, per, int(keep[j]), "orc64", kw), per["x0"][:, keep], kw, rho,
                          min_same=0.9, tag=tag)


def _iterations(out, cols):
    it = out["log_iter"][:, cols] if "log_iter" in out else out["iter"][cols]
    return f"iterations {it.min()}..{it.max()} ({len(np.unique(it))} distinct)"


def check_route(monkeypatch, route, cache=None):
    shared, per = ic.base_batch(route)
    for setting in ic.SETTING_NAMES:
        tag = f"{route['id']} {setting}"
        base = run(monkeypatch, route, shared, per, setting, tag + " base", cache)
        if setting == "tol":
            _anchor(route, shared, per, base, tag + " anchor")
        for name in route["arrangements"]:
            arr, cols, base_cols, hard, trivial = ic.arrange(route, name)
            got = run(monkeypatch, route, shared, arr, setting, f"{tag} {name}", cache)
            print(f"BI {route['id']} | {setting} | {route['kernel']} | {name}: compared {len(cols)} of {arr['x0'].shape[-1]} | "
                  f"{_iterations(base, base_cols)}")
            if name == "permuted":      # (the arrangement did move the batch: un-permuting is what makes the runs equal)
                assert not np.array_equal(got["states"], base["states"])
            for key in base:
                a, b = got[key][..., cols], base[key][..., base_cols]
                if not np.array_equal(a, b):
                    moved = base_cols[np.nonzero(np.any((a != b).reshape(-1, len(cols)), axis=0))[0]]
                    raise AssertionError(f"{tag} {name}: {key} of {len(moved)} instance(s) depends on the arrangement, base instances {moved[:12]}")
            if len(hard):
                for key in ("states", "controls"):
                    assert np.isfinite(got[key][..., hard]).all(), f"{tag}: a hard instance's {key} are not finite"
                if setting == "tol":      # (the first solve: what the CPU conditions establish)
                    so = got["log_solved"][0, hard] if "log_solved" in got else got.get("first_solved", got["solved"])[hard]
                    assert not so.any(), f"{tag}: a hard instance reports solved"


@pytest.mark.parametrize("group", ic.GROUPS)
def test_result_depends_on_own_inputs_only(hip_lib, oracle_built, monkeypatch, jit_cache, group):
    if any(r["specialised"] for r in ic.routes_of(group)) and not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    for route in ic.routes_of(group):
        check_route(monkeypatch, route, jit_cache)


def _refill_run(monkeypatch, x0, tag):
    _env(monkeypatch, dict(ic.REFILL, specialised=False))
    prob = ic.refill_batch()[0]
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=x0.shape[1])
    bs.update_settings(**ic.REFILL["kw"])
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(False)
    bs.set_x0(np.asfortranarray(x0))
    bs.solve()
    assert (bs.kernel_name, bs.last_launch_name) == (ic.REFILL["family"], ic.REFILL["kernel"]), tag
    out = {}
    _solution(bs, out)
    bs.close()
    return out


def test_mfma_refill_slots(hip_lib, oracle_built, monkeypatch):
    """the refill variant, where an instance's slot depends on when its predecessors finish: permuted and with its neighbours
    replaced (tests/independence_cases.py: REFILL), S against the batch oracle"""
    prob, x0 = ic.refill_batch()
    kw, B = ic.REFILL["kw"], ic.REFILL["B"]
    base = _refill_run(monkeypatch, x0, "refill base")
    x0n, keep, hard, trivial = ic.refill_neighbours()
    ref = ic.refill_oracle_on_kept("orc64")
    from oracle import cpu_oracle

    def make(j):
        o = cpu_oracle.CpuSolver("orc64", prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
        o.update_settings(**kw)
        o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        return o
    sol = dict(states=base["states"][:, :, keep], controls=base["controls"][:, :, keep])
    st = dict(iter=base["iter"][keep], solved=base["solved"][keep])
    parity_every_instance(sol, st, ref, make, x0[:, keep], kw, prob.rho, min_same=0.9, tag="refill anchor")
    perm = ic.permutation(B, ic.GEOMETRY["mfma"])
    for name, xa, cols, base_cols in (("permuted", x0[:, perm], np.arange(B), perm), ("neighbours", x0n, keep, keep)):
        got = _refill_run(monkeypatch, xa, f"refill {name}")
        print(f"BI mfma_refill | tol | {ic.REFILL['kernel']} | {name}: compared {len(cols)} of {B} | {_iterations(base, base_cols)}")
        if name == "permuted":
            assert not np.array_equal(got["states"], base["states"])
        for key in base:
            a, b = got[key][..., cols], base[key][..., base_cols]
            if not np.array_equal(a, b):
                moved = base_cols[np.nonzero(np.any((a != b).reshape(-1, len(cols)), axis=0))[0]]
                raise AssertionError(f"refill {name}: {key} of {len(moved)} instance(s) depends on the arrangement, base instances {moved[:12]}")
        if name == "neighbours":
            assert np.isfinite(got["states"][..., hard]).all() and np.isfinite(got["controls"][..., hard]).all()
            assert not got["solved"][hard].any(), "a hard instance reports solved"
