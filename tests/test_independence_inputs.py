"""Conditions on the inputs of the batch-independence tests (tests/independence_cases.py), on the CPU oracles alone: what
tests/test_batch_independence_gpu.py runs the kernels on does exercise what it is meant to.

Per route, on orc64 and the tolerance-terminated setting (the first, cold solve of every instance):
  - S, the instances that stay in place when the neighbours are replaced, leaves at more than three distinct iteration counts;
  - every hard instance runs to max_iter unsolved with |u| on its bound somewhere;
  - every trivial instance stops at the first check — where zero solves the zero-state problem; on the routes with non-zero
    shared references or an affine term (first_check = False) nothing is asked of its exit;
  - orc32 takes orc64's exit on at least 0.9 of S: the oracle anchor leaves out at most a tenth of S.
Per geometry: the permutation moves an instance across and within every unit and into and out of every ragged tail, S contains
the whole tail, and the truncated size is no multiple of any unit and at most B - 17."""
import numpy as np
import pytest

from tests import independence_cases as ic


def _input_key(route):
    return (route["inputs"][0], tuple(sorted(route["inputs"][1].items())), route["B"], route["geom"], route["hard"], route["first_check"])


# routes that share inputs, geometry and factors share the conditions: one case per distinct key
DISTINCT = list({_input_key(r): r for r in reversed(ic.ROUTES)}.values())[::-1]


def test_route_table_is_complete():
    ids = [r["id"] for r in ic.ROUTES]
    assert len(ids) == len(set(ids))
    for r in ic.ROUTES:
        assert r["geom"] in ic.GEOMETRY and r["inputs"][0] in ic.BUILDERS and r["pattern"] in ("oneshot", "kept2", "rollout")
        assert set(r["arrangements"]) <= set(ic.ARRANGEMENTS) and r["kernel"] and r["family"]
        assert all(name in ic.SWITCHES for name in r["env"]), r["env"]
        noisy = "noise" in ic.base_batch(r)[0]
        assert ("permuted" in r["arrangements"]) != noisy, r["id"]      # noise is keyed by (seed, b, t): no permutation there
    kernels = {r["kernel"].split("<")[0] for r in ic.ROUTES}
    assert {"lean", "quad", "mfma", "mfmat", "mfmar", "mfmac", "stream4", "generic"} <= kernels


@pytest.mark.parametrize("geom", sorted(ic.GEOMETRY))
def test_arrangements_cross_every_boundary(geom):
    units = ic.GEOMETRY[geom]
    sizes = {r["B"] for r in ic.ROUTES if r["geom"] == geom}
    assert sizes
    for B in sizes:
        assert any(B % u for u in units), "the batch is ragged in no unit"
        perm = ic.permutation(B, units)
        assert sorted(perm) == list(range(B)) and ic.crosses(perm, units)
        assert not ic.crosses(np.arange(B), units)                     # (the condition does reject: the identity)
        for u in units:                                                 # ... and a permutation that stays within one unit u
            if u > 1 and u < B:
                inside = np.arange(B)
                inside[:u] = np.roll(inside[:u], 1)
                assert not ic.crosses(inside, units), u
        keep = ic.kept_set(B, units)
        tl = ic.tails(B, units)
        assert set(range(tl[max(tl)], B)) <= set(keep) and set(range(0, B, 3)) <= set(keep)
        others = np.setdiff1d(np.arange(B), keep)
        assert len(others) >= 8                                         # hard and trivial neighbours, several of each
        Bp = ic.truncated_size(B, units)
        assert 0 < Bp <= B - 17 and all(Bp % u for u in units if u > 1)
        for u in units:                                                 # B' cuts through a unit that the base batch fills
            if u > 1 and u < B:
                assert Bp // u < B // u or Bp % u != B % u


@pytest.mark.parametrize("route", DISTINCT, ids=lambda r: r["id"])
def test_inputs_of_a_route(oracle_built, route):
    shared, per = ic.base_batch(route)
    kw = shared["kw"]["tol"]
    units = ic.GEOMETRY[route["geom"]]
    keep = ic.kept_set(route["B"], units)
    r64, r32 = ic.oracle_on_kept(route, "tol", "orc64"), ic.oracle_on_kept(route, "tol", "orc32")
    counts = np.unique(r64["iter"])
    same = float(np.mean((r64["iter"] == r32["iter"]) & (r64["solved"] == r32["solved"])))
    arr, _, _, hard, trivial = ic.arrange(route, "neighbours")
    rh = ic.oracle_first_solve(shared, arr, "orc64", kw, hard)
    rt = ic.oracle_first_solve(shared, arr, "orc64", kw, trivial)
    print(f"BI inputs {route['id']}: S {len(keep)} of {route['B']}, iterations {counts.min()}..{counts.max()} ({len(counts)} distinct), "
          f"solved {r64['solved'].mean():.2f}, orc32 agrees on {same:.3f}; hard {len(hard)}: iter {np.unique(rh['iter'])} solved {rh['solved'].sum()}; "
          f"trivial {len(trivial)}: iter {np.unique(rt['iter'])}")
    assert len(counts) > 3, counts
    assert same >= 0.9, same
    assert np.all(rh["iter"] == kw["max_iter"]) and not rh["solved"].any(), (rh["iter"], rh["solved"])
    assert np.isfinite(rh["x"]).all() and np.isfinite(rh["u"]).all()
    for j, b in enumerate(hard):
        assert ic.input_bound_active(shared, arr, int(b), rh["u"][:, :, j]), f"hard instance {b}: the input bound is not active"
    assert np.isfinite(rt["x"]).all() and np.isfinite(rt["u"]).all()
    if route["first_check"]:
        assert np.all(rt["iter"] == 1) and rt["solved"].all(), (rt["iter"], rt["solved"])


def test_inputs_of_the_refill_route(oracle_built):
    """the same conditions on the batch oracle, at the refill test's size; the launch refills only from two rounds of resident
    workgroups on a batch that is a multiple of 64 (tests/test_mfma_variants_gpu.py: 32 768 instances at N = 30)"""
    kw, B = ic.REFILL["kw"], ic.REFILL["B"]
    units = ic.GEOMETRY["mfma"]
    assert B % 64 == 0 and B >= 32768 and ic.crosses(ic.permutation(B, units), units)
    x0n, keep, hard, trivial = ic.refill_neighbours()
    r64, r32 = ic.refill_oracle_on_kept("orc64"), ic.refill_oracle_on_kept("orc32")
    counts = np.unique(r64["iter"])
    same = float(np.mean((r64["iter"] == r32["iter"]) & (r64["solved"] == r32["solved"])))
    rh, rt = ic.refill_oracle(x0n[:, hard]), ic.refill_oracle(x0n[:, trivial])
    print(f"BI inputs mfma_refill: S {len(keep)} of {B}, iterations {counts.min()}..{counts.max()} ({len(counts)} distinct), "
          f"solved {r64['solved'].mean():.2f}, orc32 agrees on {same:.3f}; hard {len(hard)}: iter {np.unique(rh['iter'])} solved {rh['solved'].sum()}; "
          f"trivial {len(trivial)}: iter {np.unique(rt['iter'])}")
    assert len(counts) > 3 and same >= 0.9
    assert np.all(rh["iter"] == kw["max_iter"]) and not rh["solved"].any() and np.isfinite(rh["x"]).all()
    assert np.all(np.abs(rh["u"]).max(axis=(0, 1)) >= 0.5 - 1e-9)
    assert np.all(rt["iter"] == kw["check_termination"]) and rt["solved"].all()
