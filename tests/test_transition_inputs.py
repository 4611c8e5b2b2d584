"""Conditions on the inputs of the setter-transition tests (tests/transition_cases.py), on the CPU oracle alone: what
tests/test_setter_transitions_gpu.py runs the solvers on cannot pass vacuously.

Per route and solution-changing transition (groups 1-9 and 12): on at least half of the instances orc64 at A' differs from orc64
at A by more than 1e-3, norm-relative, in x or u — 100 x FP32_TOL.  A setter whose effect the used solver loses then moves the
result a hundred times further than the parity tolerance.  Both numbers are conditions on the inputs, not measurements: the rows,
cones, bounds and references of transition_cases.data_of were chosen until the oracle alone meets them.
Per route: the instances leave at more than three distinct iteration counts under the base configuration (tolerance-terminated,
a check every iteration, max_iter <= 60).
Each case prints "TI <route> | <transition> | share .. | iterations A lo..hi, A' lo..hi" (profiles/transition_routes.txt)."""
import numpy as np
import pytest

from tests import transition_cases as tc

CHANGING = [(r, x) for r, x in tc.CASES if tc.transition_by_id(x)["kind"] == "change"]


def test_tables_are_complete():
    ids = [r["id"] for r in tc.ROUTES]
    assert len(ids) == len(set(ids)) == 11 and [r["n"] for r in tc.ROUTES] == list(range(1, 12))
    assert len({x["id"] for x in tc.TRANSITIONS}) == len(tc.TRANSITIONS)
    assert {x["group"] for x in tc.TRANSITIONS} == set(range(1, 14))        # (14: the process-global surface, a GPU test of its own)
    for r in tc.ROUTES:
        cfg, per = tc.base_cfg(r)
        kw = cfg["kw"]
        assert kw["abs_pri_tol"] > 0 and kw["abs_dua_tol"] > 0 and kw["check_termination"] == 1 and kw["max_iter"] <= 60
        assert per["x0"].shape[1] == r["B"] and all(name in tc.ic.SWITCHES for name in r["env"])
        assert np.array_equal(per["x0"], per["x0"].astype(np.float32).astype(np.float64))      # (what the device holds)
        took = {x["group"] for x in tc.TRANSITIONS if tc.applies(r, x)}
        assert took == (set(range(5, 14)) if r["id"] == "p0_lean_jit" else set(range(1, 14))), (r["id"], took)
    for x in tc.TRANSITIONS:
        assert x["kind"] == ("neutral" if x["group"] in (10, 11, 13) else "change")
        for r in tc.ROUTES:
            if tc.applies(r, x):
                a, b = tc.configs(r, x)
                assert set(a) == set(b) and [k for k in a if a[k] is not b[k]] == [k for k in a if k in x["delta"]], (r["id"], x["id"])
    for (rid, xid) in list(tc.LAUNCH_AT) + [k[:2] for k in tc.REFUSALS]:
        assert (rid, xid) in tc.CASES


@pytest.mark.parametrize("route", tc.ROUTES, ids=lambda r: r["id"])
def test_base_iteration_counts_spread(oracle_built, route):
    r = tc.oracle_of(route, tc.transition_by_id("tolerances"), "A")
    counts = np.unique(r["iter"])
    print(f"TI {route['id']} | base | {len(r['iter'])} instances | iterations {counts.min()}..{counts.max()} ({len(counts)} distinct), solved {r['solved'].mean():.2f}")
    assert len(counts) > 3, counts
    assert np.isfinite(r["x"]).all() and np.isfinite(r["u"]).all()


@pytest.mark.parametrize("rid,xid", CHANGING, ids=[f"{r}-{x}" for r, x in CHANGING])
def test_transition_changes_the_solution(oracle_built, rid, xid):
    route, tr = tc.route_by_id(rid), tc.transition_by_id(xid)
    ra, rb = tc.oracle_of(route, tr, "A"), tc.oracle_of(route, tr, "B")
    share = tc.changed_share(ra, rb)
    print(f"TI {rid} | {xid} | share {share:.3f} of {len(ra['iter'])} | iterations A {ra['iter'].min()}..{ra['iter'].max()}, "
          f"A' {rb['iter'].min()}..{rb['iter'].max()} ({len(np.unique(rb['iter']))} distinct)")
    assert np.isfinite(rb["x"]).all() and np.isfinite(rb["u"]).all()
    assert share >= tc.MIN_SHARE, f"{rid} {xid}: A' differs from A on {share:.3f} of the instances only"
