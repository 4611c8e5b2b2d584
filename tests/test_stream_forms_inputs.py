"""The conditions on the inputs of tests/test_stream_forms_gpu.py, asserted on the two CPU oracles alone (no GPU).

The stream and the generic kernel are held to FP32_TOL against orc64 in every form.  A comparison with a reference can hide a
failure: where the fp32 loop itself is far off, the bar is not the kernel's to meet; where the two oracles stop at different
iterations, few instances are compared; where no set acts or every instance leaves by the same exit, the projections and the
per-lane guard are not exercised.  So, per shape and arm of tests/stream_forms_cases.py — the very inputs the GPU file runs —
and as caps, the seeds and the recipes having been chosen until the oracles meet them (stream_forms_cases.conditions):
  * orc32's worst nrel_batch from orc64 <= FP32_TOL: orc32 rounds everything the fp32-state kernels round, and the recurrences
    besides; where it holds the bar the kernels have no excuse (for the arms that run at precision 1 too this is well inside
    test_precision1_inputs.py's cap of 2e-4),
  * orc32 and orc64 agree on (iter, solved) for >= 0.9 of the instances,
  * per shape, one tolerance-terminated arm at least has an orc64 solved share within [0.1, 0.9]: both exits in one wavefront,
  * in every arm >= 0.1 of the instances have an input at a bound, on the input cone's surface or at an input row,
  * in every arm >= 0.2 of the instances have a state at its bound at a knot after the first,
  * adaptive arms: rho leaves the family's value by > 0.05 on >= half the instances, and orc32 reproduces orc64's rho to 1e-5,
  * per-instance families: the 70 families hold >= 8 distinct Riccati sweep counts.
Each arm prints "<case> <arm>: e32 .. agreement .. solved .. binding .. state .." before anything is asserted."""
import numpy as np
import pytest

from tests import stream_forms_cases as sc


@pytest.mark.parametrize("shape", sc.GRID, ids=sc.shape_id)
def test_stream_grid_cases(hip_lib, oracle_built, shape):
    case = sc.stream_case(*shape)
    missed = sc.conditions(case, sc.STREAM_ARMS)
    assert not missed, "\n".join(missed)


def test_stream_grid_layout():
    """what the recipe promises of the 25 cases: neighbouring shapes differ in the horizon, every horizon lies in 5 .. 9, the state
    cone covers rows RX - 1 and RX, the input cone rows 0 and 1 (RU = 1 on the whole grid), the bounds are per knot, every x0 is
    inside its box, and the rows' coefficients lie on the 2^-10 grid"""
    hs = [sc.horizon(*s) for s in sc.GRID]
    assert all(5 <= h <= 9 for h in hs) and all(a != b for a, b in zip(hs, hs[1:])) and sc.horizon(4, 1) not in (2, 5, 10, 15, 20, 30)
    for nx, nu in sc.GRID:
        cu, cx = sc.cone_layout(nx, nu)
        rx = (nx + 3) // 4
        rows = set(range(cx[0][0], cx[0][0] + cx[1][0]))
        assert {rx - 1, rx} <= rows and max(rows) < nx and len(rows) == (3 if nx >= 3 else 2)
        assert (len(cu[0]) == 0) == (nu == 1)
        if nu > 1:
            assert cu[0] == [0] and cu[1] == [min(3, nu)]


@pytest.mark.parametrize("shape", [(2, 1), (6, 3), (10, 4)], ids=sc.shape_id)
def test_stream_case_inputs_are_what_they_say(oracle_built, shape):
    case = sc.stream_case(*shape)
    p, x0 = case["prob"], case["x0"]
    assert np.all(x0 > p.x_min[:, :1]) and np.all(x0 < p.x_max[:, :1])
    assert np.any(p.x_max[:, -1] != p.x_max[:, 0]) and np.any(p.x_min[:, -1] != p.x_min[:, 0])
    Ax, bx, Au, bu = sc.shared_rows(case)
    assert Ax.shape == (2, case["nx"]) and Au.shape == (2, case["nu"])
    assert np.array_equal(Ax * 1024.0, np.round(Ax * 1024.0)) and np.array_equal(Au * 1024.0, np.round(Au * 1024.0))
    assert np.all(Ax @ x0 < bx[:, None])                               # every x0 satisfies the state rows


@pytest.mark.parametrize("shape", sc.GENERIC_SHAPES, ids=sc.shape_id)
def test_generic_cases(hip_lib, oracle_built, shape):
    case = sc.generic_case(*shape)
    missed = sc.conditions(case, sc.generic_arms(case))
    assert not missed, "\n".join(missed)


def test_long_horizon_cases(oracle_built):
    """Part 3's inputs: 10 fixed iterations, input bounds only, five instances; orc32 within FP32_TOL of orc64 at every horizon that
    is solved on the stream kernel, and an input at its bound in every instance"""
    from tests.util import FP32_TOL
    for N in sc.long_horizons()["solved"]:
        case = sc.long_case(N)
        r64, r32, limit, e32, same = sc.long_pair(case)
        ub = sc.pc.input_bound_share(case, r64)
        print(f"{case['tag']}: e32 {e32:.2e} agreement {same:.2f} binding {ub:.2f}")
        assert e32 <= FP32_TOL and same == 1.0 and ub >= 0.1
