"""The conditions on the inputs of tests/test_precision1_gpu.py, asserted on the two CPU oracles alone (no GPU).

The precision-1 kernels are held to limit_case = max(FP32_TOL, 4 * e32_case), e32_case being orc32's own distance from orc64
(tests/util.py: precision1_limit).  A bar taken from the reference model can hide a failure: where orc32 itself is far off the bar
is wide, where the two oracles stop at different iterations few instances are compared, and where no bound binds or every
instance leaves by the same exit the projections and the per-lane guard are not exercised.  So, per case of
tests/precision1_cases.py — the very inputs the GPU file runs:
  * e32_case <= 2e-4 (no limit above 8e-4),
  * orc32 and orc64 agree on (iter, solved) for >= 0.9 of the instances,
  * per quad entry, one tolerance-terminated case at least has an oracle solved share within [0.1, 0.9]: both exits in one
    wavefront,
  * with state bounds on, >= 0.2 of the instances have a state at a bound in orc64's solution (a knot after the first),
  * >= 0.1 of the instances have an input at its bound (in the linear-row case, whose box is out of reach on purpose: at a row).
"""
import numpy as np
import pytest

from tests import precision1_cases as pc

E32_CAP = 2e-4
MIN_SAME = 0.9


def _check_pair(tag, e32, same):
    print(f"{tag}: e32 {e32:.2e} agreement {same:.2f}")
    assert e32 <= E32_CAP, f"{tag}: orc32 is {e32:.2e} from orc64"
    assert same >= MIN_SAME, f"{tag}: the oracles agree on the exit of {same:.2f} of the instances only"


@pytest.mark.parametrize("entry", pc.QUAD_ENTRIES, ids=pc.entry_id)
def test_quad_entry_cases(oracle_built, entry):
    nx, nu, N, G = entry
    B = pc.BATCH[G]
    mixed = []
    for xb in pc.XB:
        for refs in pc.REFS:
            for setting in pc.SETTINGS:
                case = pc.quad_case(nx, nu, N, B, xb, refs, setting)
                r64, r32, limit, e32, same = pc.oracle_pair(case)
                _check_pair(case["tag"], e32, same)
                assert limit <= 4 * E32_CAP
                ub = pc.input_bound_share(case, r64)
                assert ub >= 0.1, f"{case['tag']}: an input at its bound on {ub:.2f} of the instances only"
                if xb:
                    sb = pc.state_bound_share(case, r64)
                    assert sb >= 0.2, f"{case['tag']}: a state at its bound on {sb:.2f} of the instances only"
                if setting == "tol":
                    mixed.append(float(r64["solved"].mean()))
                    assert np.all(r64["iter"][r64["solved"] == 0] == case["kw"]["max_iter"])
                else:
                    assert not r64["solved"].any() and np.all(r64["iter"] == case["kw"]["max_iter"])
    assert any(0.1 <= m <= 0.9 for m in mixed), f"{pc.entry_id(entry)}: solved shares {mixed}: no case with both exits"


def test_state_bounds_are_per_knot_and_span_two_lane_roles(oracle_built):
    """what the recipe promises of the bounded rows: finite on rows 0 .. nx/2 - 1 only, the upper bound 10 % higher from knot
    N/2 on; for nx = 12 (three rows per lane in the four-lanes-per-instance kernel) rows 0 .. 5 are lanes 0 and 1"""
    for nx, nu, N in ((4, 1, 20), (12, 4, 30), (6, 3, 10)):
        p = pc.quad_case(nx, nu, N, 70, True, "zero", "fixed")["prob"]
        fin = np.abs(p.x_max) < 1e17
        assert fin[:nx // 2].all() and not fin[nx // 2:].any() and np.array_equal(fin, np.abs(p.x_min) < 1e17)
        assert np.allclose(p.x_max[:nx // 2, N // 2:], 1.1 * p.x_max[:nx // 2, :1]) and np.allclose(p.x_max[:nx // 2, :N // 2], p.x_max[:nx // 2, :1])
        assert np.array_equal(p.x_min[:, :1] * np.ones((1, N)), p.x_min)
        off = pc.quad_case(nx, nu, N, 70, False, "zero", "fixed")["prob"]
        assert np.all(off.x_min == -1e17) and np.all(off.x_max == 1e17) and np.all(np.abs(off.u_max) < 1e17)


@pytest.mark.parametrize("entry", pc.CONTINUED, ids=pc.entry_id)
def test_continued_solve_cases(oracle_built, entry):
    nx, nu, N, G = entry
    case = pc.quad_case(nx, nu, N, pc.BATCH[G], True, "shared", "fixed", max_iter=20)
    x1, r64, limit, e32, same = pc.continued_pair(case)
    _check_pair(case["tag"] + " second solve", e32, same)
    assert pc.input_bound_share(case, r64) >= 0.1 and pc.state_bound_share(case, r64) >= 0.2
    assert np.abs(x1 - case["x0"]).max() > 1e-3                     # (the second solve starts elsewhere)


@pytest.mark.parametrize("entry", pc.CLOSED_LOOP, ids=pc.entry_id)
def test_closed_loop_cases(oracle_built, entry):
    nx, nu, N, G = entry
    case = pc.quad_case(nx, nu, N, pc.BATCH[G], False, "zero", "fixed", max_iter=10)
    r64, limit, e32, same = pc.closed_loop_pair(case, pc.LOOP_STEPS)
    _check_pair(case["tag"] + " closed loop", e32, same)
    hit = np.abs(np.abs(r64["u"]) - 0.5).min(axis=(0, 1)) <= 1e-12   # the applied control of some step sits at the box
    assert hit.mean() >= 0.1, hit.mean()


@pytest.mark.parametrize("name", sorted(pc.STREAM_CASES))
def test_stream_and_generic_cases(oracle_built, name):
    case = pc.STREAM_CASES[name]()
    r64, r32, limit, e32, same = (pc.loop_pair if "make" in case else pc.oracle_pair)(case)
    _check_pair(case["tag"], e32, same)
    if "lin" in case:        # the rows bind where the box cannot
        Ax, bx, Au, bu = case["lin"]
        at_row = (np.einsum("ij,jkb->ikb", Au, r64["u"]) >= bu[:, None, None] - 1e-9).any(axis=(0, 1))
        assert at_row.mean() >= 0.1, at_row.mean()
    elif name.startswith("rocket_cones"):
        # the input cone binds: |u_xy| reaches mu u_z at some knot — to the solve's tolerance, the solution being the box
        # set's slack, which the cone set's slack meets at convergence only
        u = r64["u"]
        on_cone = (np.hypot(u[0], u[1]) >= 0.999 * 0.25 * u[2]).any(axis=0)
        assert on_cone.mean() >= 0.1, on_cone.mean()
    else:
        ub = pc.input_bound_share(case, r64)
        assert ub >= 0.1, f"{case['tag']}: an input at its bound on {ub:.2f} of the instances only"


@pytest.mark.parametrize("N", [20, 17])
def test_adaptive_rho_cases(hip_lib, oracle_built, N):
    """part e stands only where the reference model carries it: orc32 reproduces orc64's adapted rho on every instance (to
    1e-5 relative, the bar of the adaptive tests of the fp64-recurrence kernels), rho does move, both exits occur and the
    solution error stays under the cap.  (The sensitivities come from the library's host-only finite differences.)"""
    case = pc.adaptive_case(N)
    r64, limit, e32, same, rho_limit, drho = pc.adaptive_pair(case)
    _check_pair(case["tag"], e32, same)
    print(f"{case['tag']}: rho {r64['rho'].min():.3f} .. {r64['rho'].max():.3f}, orc32 within {drho:.2e}")
    assert same == 1.0 and drho <= 1e-5
    assert (np.abs(r64["rho"] - case["prob"].rho) > 0.05).mean() >= 0.5
    assert 0.1 <= r64["solved"].mean() <= 0.9
    assert pc.input_bound_share(case, r64) >= 0.1
