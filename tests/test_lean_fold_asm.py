"""The folded backward sweep of the headline kernel in the compiler's own assembly (csrc/admm_lean.hip.h: FOLD).

The unit is built exactly as tests/test_lean_scaled_asm.py builds its own: admm_lean_kernel<4,1,20, LIVE=false, UBK=true,
ONE=true, XB=false, zero references, fp32 state, cartpole's scaled pattern> — what bench.py's default launches.  With one input
C = -rho Quu_inv is a scalar that the costate's scale takes in: d_k = fma(B^_1, pv_1, fma(c, r~, pv_3)) replaces t = r~ + pv_3,
fma(B^_1, pv_1, t), d = C t — one fp64 instruction fewer at each of the 19 knots that form a d.  The scaled kernel's bounds
(tests/test_lean_scaled_asm.py: 544 vector instructions; profiles/r21_cartpole_isa_census.json: 454 of them fp64) move down by
19 each; the packed slack / dual update, the absence of spills and the status fold's 7 swaps stay.  The tolerance-terminated
unit of the same pattern, which shares the sweeps and must agree with it bit for bit, compiles without a spill."""
import os

import pytest

from tests.test_lean_pk_asm import _hot_loop, _ops, _valu
from tests.test_lean_scaled_asm import HIPCC, N, _unit

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def test_folded_headline_loop(tmp_path):
    body, spills = _unit(tmp_path, "fold", "false")
    loop, ops = _hot_loop(body), _ops(body)
    pk, valu = sum(o == "v_pk_add_f32" for o in loop), _valu(loop)
    f64 = sum(o.startswith(("v_fma_f64", "v_fmac_f64", "v_add_f64", "v_mul_f64")) for o in loop)
    swaps = sum(o.startswith("global_atomic_swap") for o in ops)
    print(f"folded: {valu} VALU in the loop ({f64} fp64, {pk} v_pk_add_f32), spills {spills}, {swaps} global_atomic_swap")
    assert valu <= 544 - (N - 1)
    assert f64 <= 454 - (N - 1)
    assert pk >= 27
    assert spills == [0] and not any(o.startswith("scratch_") for o in ops)
    assert swaps == 7


def test_folded_live_unit_does_not_spill(tmp_path):
    body, spills = _unit(tmp_path, "fold_live", "true")
    assert spills == [0] and not any(o.startswith("scratch_") for o in _ops(body))
