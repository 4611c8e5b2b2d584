"""The input conditions of the workspace hand-over tests (tests/test_workspace_handover_gpu.py), on the oracles alone: what keeps
that file from passing vacuously.  tests/handover_cases.py has the tours; every figure asserted here is printed first
(profiles/handover_routes.txt holds a run's).

 * the tours visit what they claim: every ordered pair of their families, the quad kernel with 1, 2 and 4 lanes, a chunked solve out
   of the lean route, the lift at a step of the lean / the matrix-core kernel;
 * the warm start matters: at every step k >= 1 orc64 from the kept workspace differs from orc64 cold-started at the same x0 by
   more than 1e-3 on at least half of the instances — a family that ignored the workspace would fail;
 * every array matters: for each of d, y, g, v, z, zeroing that one array in the oracle before some step changes that step's solution
   by more than 1e-3 on at least a tenth of the instances.  g on the tours with a state bound: at a step before the lift, and on
   the quadrotor tour AT the lift (the step whose launch carries g on the host flag's word alone).  On the cartpole tour the lifted
   bound is on the cart's position, whose weight of 10 against rho = 1 makes a solve forget a stale g within four iterations
   (contraction 1 / 11 an iteration): there the condition at the lift is that the dual the bound left is there to be carried —
   above 1e-2 on at least a tenth of the instances — and the GPU file holds g itself to the oracle's after that step.
   v and z cannot meet the condition as worded and are held to what they can do: they are the PREVIOUS slack, read by the dual
   residual alone (admm.cpp:93-97), so no iterate depends on them; zeroing one moves a solution only by moving an exit, and only the
   exit at the first check, after which both are overwritten.  Asserted: zeroing v (z) changes no more instances than
   leave at the first check, and on the cartpole tours, a quarter of whose instances start nearly settled, it changes at least
   0.03 of the batch — at every step of the cartpole tour (measured 0.04 to 0.10), at some step of the precision-2 one (0.01 to
   0.04); a tenth was not reached at any scale tried.  The GPU file compares v and z themselves at every step;
 * both exits occur: in the tolerance-terminated tours the solved share of every step lies in [0.1, 0.9];
 * the replay cap: orc32 leaves orc64's exit on at most 0.05 of the instances per step (the GPU file allows 0.1), and with
   orc64's exits imposed stays within FP32_TOL of it — on the cartpole, rocket, precision-2 and adaptive tours.  On the quadrotor at
   N = 30 the all-fp32 loop does not: 4e-6 to 1.9e-5 over the tour's steps, and 1e-5 to 9e-5 at every other input tried (the input
   bound from 0.05 to 0.5, the state bound on or off, 5 to 40 iterations a solve) — why no kernel runs that shape with fp32
   recurrences by default.  A decided exception: the figure is held to 3e-5, the exits to the cap; the
   kernels, with fp64 recurrences, hold FP32_TOL there with a factor of ten;
 * cones and rows bind: on the rocket tour at least a tenth of the instances touch a cone at every step and, from the step that
   adds them, a row;
 * the derived workspace limits are what handover_cases.derived_limits says: max(lean limit, 4 x orc32's worst distance)."""
import numpy as np
import pytest

from tests import handover_cases as hc
from tests.util import FP32_TOL, nrel_batch

E32_TOURS = ("cartpole", "rocket", "p2", "adaptive")
# a decided exception: the all-fp32 loop of the (12,4,30) shape does not come within FP32_TOL of orc64 at any
# input tried; on this tour it is 4e-6 .. 1.9e-5 off.  Held to three times FP32_TOL so that it cannot drift
QUADROTOR_E32_CEILING = 3e-5
FIRST_CHECK_TOURS = ("cartpole", "p2")
FIRST_CHECK_SHARE = 0.03        # v, z: the first-check leavers zeroing one of them moves — cartpole at every step, p2 at some step
G_TOURS = ("cartpole", "quadrotor")


def test_tours_visit_what_they_claim(hip_lib):
    for id in hc.TOURS:
        tour = hc.tour_of(id)
        fam = [s["kernel"].split("<")[0] for s in tour["steps"]]
        assert set(fam) == set(tour["families"]), (id, fam)
        if id != "rocket":
            want = {(a, b) for a in tour["families"] for b in tour["families"] if a != b}
            assert hc._pairs(tour["steps"]) == want, (id, want - hc._pairs(tour["steps"]))
            assert len(tour["steps"]) == (7 if id == "p2" else len(want) + 1)      # (p2: three solves each way)
        for a, b in zip(tour["steps"][:-1], tour["steps"][1:]):
            assert a["kernel"] != b["kernel"], (id, a["kernel"])
            assert (a["env"] != b["env"]) != bool([c for c in b["calls"] if c[0] != "lift"]), (id, b["change"])     # ONE thing moves the route
    rocket = hc.tour_of("rocket")["steps"]
    assert hc._pairs(rocket[:7]) == {(a, b) for a in ("mfmat", "stream4", "generic") for b in ("mfmat", "stream4", "generic") if a != b}
    assert ("rows",) in rocket[7]["calls"] and [s["kernel"] for s in rocket[7:]] == ["stream4<6,3>", "generic", "stream4<6,3>"]
    cart = hc.tour_of("cartpole")["steps"]
    assert {"quad<4,1,20,g1>", "quad<4,1,20,g2>", "quad<4,1,20,g4>"} <= {s["kernel"] for s in cart}
    assert cart[-1]["calls"] == (("compaction", 5),) and cart[-2]["kernel"] == "lean<4,1,20>" and cart[-1]["env"] == cart[-2]["env"]
    assert cart[hc.tour_of("cartpole")["lift"]]["kernel"] == "lean<4,1,20>"
    quad = hc.tour_of("quadrotor")
    assert quad["steps"][quad["lift"]]["kernel"] == "mfma<12,4,30>" and quad["steps"][quad["lift"] - 1]["kernel"] != "mfma<12,4,30>"
    p2 = [s["kernel"] for s in hc.tour_of("p2")["steps"]]
    assert p2 == ["generic<f64>", "stream4<4,1;f64>"] * 3 + ["generic<f64>"]


@pytest.mark.parametrize("id", hc.TOURS)
def test_the_warm_start_matters(hip_lib, oracle_built, id):
    tour = hc.tour_of(id)
    shares = [hc.warm_share(tour, k) for k in range(1, len(tour["steps"]))]
    print(f"HO {id}: share of instances whose warm solve differs from the cold one by more than {hc.CHANGE:g}, steps 1..: " + " ".join(f"{s:.2f}" for s in shares))
    assert min(shares) >= 0.5, (id, shares)


@pytest.mark.parametrize("id", hc.TOURS)
def test_every_array_matters(hip_lib, oracle_built, id):
    tour = hc.tour_of(id)
    n = len(tour["steps"])
    keys = [k for k in hc.WS_KEYS if k != "g" or id in G_TOURS]
    for key in keys:
        shares = [hc.zeroed_share(tour, k, key) for k in range(1, n)]
        print(f"HO {id}: share of instances that zeroing {key} before a step changes by more than {hc.CHANGE:g}, steps 1..: " + " ".join(f"{s:.2f}" for s in shares))
        if key == "g":
            lift = tour["lift"]
            assert max(shares[:lift - 1]) >= 0.1, (id, key, shares)
            left = np.abs(hc.oracle_tour(tour)[lift - 1]["ws"]["g"]).max(axis=(0, 1))
            print(f"HO {id}: the state dual the lifted bound leaves is above 1e-2 on {np.mean(left > 1e-2):.2f} of the instances (largest {left.max():.2e})")
            assert np.mean(left > 1e-2) >= 0.1, (id, np.mean(left > 1e-2))
            if id == "quadrotor":
                assert shares[lift - 1] >= 0.1, (id, "g at the lift", shares[lift - 1])
        elif key in ("v", "z"):
            first = [float(np.mean((a["iter"] == 1) & (a["solved"] == 1))) for a in hc.oracle_tour(tour)[1:]]
            print(f"HO {id}: instances that leave at the first check, steps 1..: " + " ".join(f"{s:.2f}" for s in first))
            assert all(a <= b + 1e-12 for a, b in zip(shares, first)), (id, key, shares, first)
            if id in FIRST_CHECK_TOURS:
                assert (min(shares) if id == "cartpole" else max(shares)) >= FIRST_CHECK_SHARE, (id, key, shares)
        else:
            assert max(shares) >= 0.1, (id, key, shares)


@pytest.mark.parametrize("id", hc.TOURS)
def test_exits_and_replay_cap(hip_lib, oracle_built, id):
    tour = hc.tour_of(id)
    r64, r32 = hc.oracle_tour(tour), hc.oracle_tour(tour, "orc32")
    solved = [float(a["solved"].mean()) for a in r64]
    differ = [float(b["replayed"].mean()) for b in r32]
    e32 = [max(float(nrel_batch(b["x"], a["x"]).max()), float(nrel_batch(b["u"], a["u"]).max())) for a, b in zip(r64, r32)]
    its = [f"{a['iter'].min()}..{a['iter'].max()}" for a in r64]
    print(f"HO {id}: solved share per step " + " ".join(f"{s:.2f}" for s in solved))
    print(f"HO {id}: iterations per step " + " ".join(its))
    print(f"HO {id}: orc32 leaves orc64's exit on " + " ".join(f"{s:.3f}" for s in differ))
    print(f"HO {id}: orc32 from orc64, exits imposed " + " ".join(f"{e:.1e}" for e in e32))
    print(f"HO {id}: an input at its bound on " + " ".join(f"{hc.input_bound_share(tour, a):.2f}" for a in r64))
    if tour["terminated"]:
        assert min(solved) >= 0.1 and max(solved) <= 0.9, (id, solved)
    else:
        assert all(np.all(a["iter"] == tour["kw"]["max_iter"]) and not a["solved"].any() for a in r64)
    assert max(differ) <= hc.ORACLE_CAP < hc.REPLAY_CAP, (id, differ)
    if id in E32_TOURS:
        assert max(e32) <= FP32_TOL, (id, e32)
    else:
        assert id == "quadrotor" and max(e32) <= QUADROTOR_E32_CEILING, (id, e32)
    if "adaptive" in tour:
        moved = [float(np.mean(np.abs(a["rho"] - tour["prob"].rho) > 0.05)) for a in r64]
        drho = [float((np.abs(b["rho"] - a["rho"]) / a["rho"]).max()) for a, b in zip(r64, r32)]
        print(f"HO {id}: rho has left the family's on " + " ".join(f"{m:.2f}" for m in moved) + "; orc32's rho within " + " ".join(f"{d:.1e}" for d in drho))
        assert min(moved) >= 0.5 and max(drho) <= 1e-5, (id, moved, drho)
    if tour["lift"] is not None:
        xb = [hc.state_bound_share(tour, a) for a in r64[:tour["lift"]]]
        print(f"HO {id}: a bounded state at its bound, steps before the lift, on " + " ".join(f"{s:.2f}" for s in xb))
        assert min(xb) >= 0.1, (id, xb)


def test_cones_and_rows_bind(hip_lib, oracle_built):
    tour = hc.tour_of("rocket")
    run = hc.oracle_tour(tour)
    cones = [hc.cone_share(tour, a) for a in run]
    first = next(i for i, s in enumerate(tour["steps"]) if ("rows",) in s["calls"])
    rows = [hc.row_share(tour, a) for a in run[first:]]
    print("HO rocket: a cone touched on " + " ".join(f"{s:.2f}" for s in cones) + f"; a row, from step {first} on, on " + " ".join(f"{s:.2f}" for s in rows))
    print("HO rocket: rows " + "; ".join(np.array2string(a, precision=4).replace("\n", "") for a in hc.rows_of(tour)))
    assert min(cones) >= 0.1 and min(rows) >= 0.1, (cones, rows)


@pytest.mark.parametrize("id", hc.TOURS)
def test_derived_limits(hip_lib, oracle_built, id):
    tour = hc.tour_of(id)
    lim = hc.derived_limits(tour)
    print(f"HO {id}: derived workspace limits " + ", ".join(f"{k} {v[0]:.2e} (orc32 within {v[1]:.2e})" for k, v in lim.items()))
    for key, (limit, e32) in lim.items():
        assert limit == max(hc.lean_limit(key), hc.FACTOR * e32) and np.isfinite(limit)
    for (tid, family), keys in hc.DERIVED.items():
        assert tid in hc.TOURS and family in hc.tour_of(tid)["families"] and set(keys) <= set(hc.WS_KEYS)
