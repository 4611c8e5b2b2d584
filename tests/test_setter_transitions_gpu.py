"""Every single setter on a used solver, held to a fresh solver, bit for bit (tests/transition_cases.py has the routes, the
transitions and the inputs; tests/test_transition_inputs.py the conditions that keep this file from passing vacuously).

Solver keeps about a dozen cached device images behind dirty flags.  A setter that forgets to invalidate one makes the next
solve run the OLD problem without an error — and tests/test_history_independence_gpu.py cannot see it: its way back from the
decoy calls set_bound_constraints, set_fdyn and set_cache_terms on every route, each of which sets packs_dirty and bumps the
routing generation on behalf of every other setter in the sequence.  Here a transition is exactly ONE public call between two
solves, on eleven routes that cache differently, in both directions.

Used solver: created at A, x0 set once, solved (the launch name asserted: the route's own at its base configuration, the fresh
solver's of the same configuration elsewhere), the one call, reset() where A' keeps its workspace (reset clears the workspace and
touches neither packs_dirty nor the routing key), solved.  Fresh solver: created at A', the same x0, solved.  Required: the same
kernel_name and last_launch_name; np.array_equal on states, controls, iter, solved and residuals; on get_workspace() where the
workspace is kept; on get_adaptive_state() where adaptive rho is on.  No comparison has a tolerance.

Oracle anchor of the fresh solver (so that two solvers wrong in the same way fail too), with the suite's own bars and no new one:
effective precision 0 parity_every_instance at FP32_TOL; precision 2 exact iteration counts and solved flags, 1e-6 on x, u and the
residuals (tests/test_jit.py); precision 1 parity_every_instance at tests/util.py::precision1_limit; adaptive rho at effective
precision 0 tests/test_gpu_parity.py's: rho within 1e-5 relative, adapted Kinf / Pinf within FP32_TOL, on the instances whose exit
agrees.  Adaptive rho at precision 1 or 2 has no bar in the suite: compared with the fresh solver, printed, not anchored.

What it found.  Before Solver::set_cones, set_linear, tinympc_enable_cones, tinympc_enable_linear and the precision-2 branch of
select_kernel set packs_dirty, four cases failed, all on route 8 (precision 2, specialisation on):
test_one_setter_on_a_used_solver[p2_lean-rows], [p2_lean-cone], [p2_lean-rows_off] and [p2_lean-cones_off].  lean_jit is decided in
upload_packs, so the used solver kept launching lean<4,1,20;f64>, which has no rows and no cones, after it had received them (all
293 instances differed from the fresh solver's generic<f64>), and stayed on generic<f64> after it had lost them.

A refusal (transition_cases.REFUSALS) is asserted by a word of its message, and the next solve must equal the one before the call.

Each direction prints "ST <route> | <transition> | <fwd|rev> | <launch at A> -> <launch at A'> | compared .. | iterations lo..hi (n
distinct) | oracle A vs A' share .." (profiles/transition_routes.txt holds a run's figures)."""
import numpy as np
import pytest

import tinympc_julia_amd as t
from tests import transition_cases as tc
from tests.test_batch_independence_gpu import _env, _solution, make_solver
from tests.test_jit import jit_on  # noqa: F401  (the fixture of the routes that exist only with specialisation on)
from tests.util import FP32_TOL, nrel_batch, parity_every_instance, precision1_limit

pytestmark = pytest.mark.gpu


def _route_env(request, monkeypatch, route):
    _env(monkeypatch, dict(env=route["env"], specialised=False))
    if route["jit"]:
        request.getfixturevalue("jit_on")


def configure(cfg, per):
    """a solver at a configuration: make_solver for what it knows, then the rest in a fixed order, the settings' flags last"""
    sh = dict(prob=cfg["prob"])
    for k in ("fdyn", "cones", "lin"):
        if cfg[k] is not None:
            sh[k] = cfg[k]
    if cfg["precision"]:
        sh["precision"] = cfg["precision"]
    pi = dict(x0=per["x0"])
    if cfg["ib"] is not None:
        pi.update(zip(("ib_xmin", "ib_xmax", "ib_umin", "ib_umax"), cfg["ib"]))
    bs = make_solver(sh, pi, cfg["kw"])
    if cfg["il"] is not None:
        bs.set_instance_linear(*cfg["il"])
    if cfg["lin_on"] is not None:
        bs.enable_linear(*cfg["lin_on"])
    if cfg["cones_on"] is not None:
        assert bs.lib.tinympc_enable_cones(bs.h, int(cfg["cones_on"][0]), int(cfg["cones_on"][1])) == 0
    if cfg["xref"] is not None:
        bs.set_x_ref(cfg["xref"])
    if cfg["uref"] is not None:
        bs.set_u_ref(cfg["uref"])
    if cfg["cache"] is not None:
        c = cfg["cache"]
        bs.set_cache_terms(c["Kinf"], c["Pinf"], c["Quu_inv"], c["AmBKt"])
    if cfg["adaptive"] is not None:      # (no set_sensitivity: the tables are the library's own, as after the one call of the used solver)
        a = cfg["adaptive"]
        bs.set_adaptive_rho(True, a["rho_min"], a["rho_max"], a["clip"])
    if cfg["strict"]:
        bs.set_strict_precision(True)
    if cfg["compaction"]:
        bs.set_compaction(cfg["compaction"])
    bs.set_warm_start(cfg["warm"])
    bs.update_settings(**cfg["kw"])
    return bs


def _outputs(bs, cfg):
    out = dict(names=np.array([bs.kernel_name, bs.last_launch_name]), effective_precision=np.array([bs.effective_precision]))
    _solution(bs, out)
    if cfg["warm"]:
        for k, v in bs.get_workspace().items():
            out["ws_" + k] = v
    if cfg["adaptive"] is not None:
        for k, v in bs.get_adaptive_state().items():
            out["adapt_" + k] = v
    return out


_fresh = {}


def fresh(route, tr, side):
    """the fresh solver's first solve under A or A', run and anchored once per configuration"""
    key = tc.label(route, tr, side)
    if key not in _fresh:
        cfg = tc.configs(route, tr)[0 if side == "A" else 1]
        _, per = tc.base_cfg(route)
        bs = configure(cfg, per)
        bs.set_x0(per["x0"])
        bs.solve()
        out = _outputs(bs, cfg)
        bs.close()
        _anchor(route, tr, side, cfg, per, out, key)
        _fresh[key] = out
    return _fresh[key]


def _anchor(route, tr, side, cfg, per, out, tag):
    cols = tc.cols_of(route)
    ref = tc.oracle_of(route, tr, side)
    kw, ep = cfg["kw"], int(out["effective_precision"][0])
    sol = dict(states=out["states"][:, :, cols], controls=out["controls"][:, :, cols])
    st = dict(iter=out["iter"][cols], solved=out["solved"][cols])
    same = (st["iter"] == ref["iter"]) & (st["solved"] == ref["solved"])
    ex, eu = nrel_batch(sol["states"], ref["x"]), nrel_batch(sol["controls"], ref["u"])
    worst = max(ex[same].max(), eu[same].max()) if same.any() else float("nan")
    print(f"ST anchor {tag} | precision {ep} | {out['names'][1]} | same exit {same.mean():.3f} | x, u off by {worst:.2e} where it agrees")
    adaptive = cfg["adaptive"] is not None
    if adaptive and ep != 0:
        return
    make = lambda j: tc.oracle_solver(cfg, per, int(cols[j]))
    rho = cfg["adaptive"]["rho_max"] if adaptive else cfg["prob"].rho
    x0 = per["x0"][:, cols]
    if ep == 2:
        assert np.array_equal(st["iter"], ref["iter"]) and np.array_equal(st["solved"], ref["solved"]), f"{tag}: exits differ from orc64's at precision 2"
        assert ex.max() <= 1e-6 and eu.max() <= 1e-6, f"{tag}: x, u off by {ex.max():.2e}, {eu.max():.2e} at precision 2"
        res = out["residuals"][:, cols].T
        assert np.abs(res - ref["res"]).max() <= 1e-6 * max(1.0, np.abs(ref["res"]).max()), f"{tag}: residuals at precision 2"
    elif ep == 1:
        limit, e32, agree = precision1_limit(tc.oracle_of(route, tr, side, "orc32"), ref)
        print(f"ST anchor {tag} | e32 {e32:.2e} limit {limit:.2e} oracles agree on {agree:.3f}")
        parity_every_instance(sol, st, ref, make, x0, kw, rho, tol=limit, min_same=0.9, tag=tag)
    else:
        parity_every_instance(sol, st, ref, make, x0, kw, rho, min_same=0.9, tag=tag)
        if adaptive and same.any():
            ad_rho, K, P = out["adapt_rho"][cols], out["adapt_Kinf"][:, :, cols], out["adapt_Pinf"][:, :, cols]
            er = (np.abs(ad_rho - ref["rho"]) / ref["rho"])[same].max()
            ek, ep_ = nrel_batch(K, ref["Kinf"])[same].max(), nrel_batch(P, ref["Pinf"])[same].max()
            print(f"ST anchor {tag} | rho within {er:.2e}, Kinf {ek:.2e}, Pinf {ep_:.2e}; rho moved on {np.mean(np.abs(ref['rho'] - cfg['prob'].rho) > 1e-3):.2f}")
            assert er <= 1e-5 and ek <= FP32_TOL and ep_ <= FP32_TOL, f"{tag}: adapted state off by {er:.2e}, {ek:.2e}, {ep_:.2e}"


def _differences(got, want, tag):
    bad = []
    for key in want:
        if not np.array_equal(got[key], want[key]):
            if key == "names":
                bad.append(f"launched {tuple(got[key])}, the fresh solver {tuple(want[key])}")
            else:
                d = np.asarray(got[key] != want[key])
                per_instance = np.any(d.reshape(-1, d.shape[-1]), axis=0) if d.ndim else d
                bad.append(f"{key} of {int(np.sum(per_instance))} instance(s)")
    assert not bad, f"{tag}: the used solver differs from the fresh one: " + "; ".join(bad)


def check_direction(route, tr, direction):
    a_side, b_side = ("A", "B") if direction == "fwd" else ("B", "A")
    key = tr["fwd"] if direction == "fwd" else tr["rev"]
    A, Bc = (tc.configs(route, tr)[i] for i in ((0, 1) if direction == "fwd" else (1, 0)))
    _, per = tc.base_cfg(route)
    tag = f"{route['id']} {tr['id']} {direction}"
    want_a, want_b = fresh(route, tr, a_side), fresh(route, tr, b_side)
    if tc.label(route, tr, a_side).endswith("/base"):
        assert tuple(want_a["names"]) == (route["family"], route["kernel"]), f"{tag}: the base configuration ran {tuple(want_a['names'])}"
    used = configure(A, per)
    used.set_x0(per["x0"])
    used.solve()
    first = _outputs(used, A)
    assert np.array_equal(first["names"], want_a["names"]), f"{tag}: the first solve ran {tuple(first['names'])}, a fresh solver of A {tuple(want_a['names'])}"
    refusal = tc.REFUSALS.get((route["id"], tr["id"], direction))
    try:
        tc.one_call(used, key, Bc, route)
        refused = None
    except t.TinyMPCError as e:
        refused = str(e)
    if refusal is not None or refused is not None:
        assert refusal is not None and refused is not None and refusal in refused, f"{tag}: refusal {refused!r}, the table has {refusal!r}"
        if A["warm"]:
            used.reset()
        used.solve()
        _differences(_outputs(used, A), first, tag + " (refused)")
        used.close()
        print(f"ST {route['id']} | {tr['id']} | {direction} | {first['names'][1]} | refused: {refusal}")
        return
    if Bc["warm"]:
        used.reset()
    used.solve()
    got = _outputs(used, Bc)
    used.close()
    it = want_b["iter"]
    share = tc.changed_share(tc.oracle_of(route, tr, "A"), tc.oracle_of(route, tr, "B"))
    print(f"ST {route['id']} | {tr['id']} | {direction} | {want_a['names'][1]} -> {want_b['names'][1]} | compared {len(it)} | "
          f"iterations {it.min()}..{it.max()} ({len(np.unique(it))} distinct) | oracle A vs A' share {share:.3f}")
    _differences(got, want_b, tag)


@pytest.mark.parametrize("rid,xid", tc.CASES, ids=[f"{r}-{x}" for r, x in tc.CASES])
def test_one_setter_on_a_used_solver(hip_lib, oracle_built, request, monkeypatch, rid, xid):
    route, tr = tc.route_by_id(rid), tc.transition_by_id(xid)
    _route_env(request, monkeypatch, route)
    failures = []
    for direction in ("fwd", "rev"):
        try:
            check_direction(route, tr, direction)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    if tr["kind"] == "neutral":
        a, b = fresh(route, tr, "A"), fresh(route, tr, "B")
        want = tc.LAUNCH_AT.get((rid, xid))
        if want is not None:
            assert b["names"][1] == want and a["names"][1] != want, f"{rid} {xid}: launches {a['names'][1]} -> {b['names'][1]}, the table has {want}"


def test_set_batch_size_on_the_process_global_surface(hip_lib, oracle_built, monkeypatch):
    """group 14, route 1: the drop-in surface's one solver re-batched up and down between two solves equals a solver set up
    at that size (set_batch_size drops references and per-instance inputs and resets the workspace; bounds and settings stay)"""
    route = tc.route_by_id("lean")
    _env(monkeypatch, dict(env=route["env"], specialised=False))
    cfg, per = tc.base_cfg(route)
    prob, kw = cfg["prob"], cfg["kw"]
    ref = tc.oracle_of(route, tc.transition_by_id("tolerances"), "A")

    def setup(B):
        s = t.TinyMPCSolver()
        t.setup(s, prob.A, prob.B, np.zeros(prob.nx), prob.Q, prob.R, prob.rho, prob.nx, prob.nu, prob.N, batch=B, abs_pri_tol=kw["abs_pri_tol"],
                abs_dua_tol=kw["abs_dua_tol"], max_iter=kw["max_iter"], check_termination=kw["check_termination"])
        t.set_bound_constraints(s, prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        t.set_warm_start(s, False)
        return s

    def solve(s, B):
        t.set_x0(s, np.asfortranarray(per["x0"][:, :B]))
        t.solve(s)
        sol, st = t.get_solution(s), t.get_status(s)
        assert t.kernel_name() == route["family"], t.kernel_name()
        return dict(states=sol["states"], controls=sol["controls"], iter=st["iter"], solved=st["solved"], residuals=st["residuals"])

    sizes = (70, 293)
    try:
        want = {}
        for B in sizes:
            want[B] = solve(setup(B), B)
            t.cleanup()
            sub = {k: v[..., :B] if k in ("x", "u") else v[:B] for k, v in ref.items()}
            parity_every_instance(want[B], want[B], sub, lambda j: tc.oracle_solver(cfg, per, int(j)), per["x0"][:, :B], kw, prob.rho, min_same=0.9,
                                  tag=f"global surface, batch {B}")
        for first, second in (sizes, sizes[::-1]):
            s = setup(first)
            before = solve(s, first)
            _differences(before, want[first], f"global surface, batch {first}")
            t.set_batch_size(s, second)
            got = solve(s, second)
            t.cleanup()
            print(f"ST lean | set_batch_size | {first} -> {second} | {route['family']} | compared {second} | iterations {got['iter'].min()}..{got['iter'].max()}")
            _differences(got, want[second], f"set_batch_size {first} -> {second}")
    finally:
        t.cleanup()
