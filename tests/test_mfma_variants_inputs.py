"""The conditions on the inputs of tests/test_mfma_variants_gpu.py, asserted on the two CPU oracles alone (no GPU).

A comparison against the oracle says little where the inputs leave the code under test idle: an adaptive solve whose rho
stays at the family's value runs the plain arithmetic, a batch that leaves by one exit exercises neither the per-instance
capture nor the idle lanes, a state bound that never binds leaves the dual at zero, and an instance whose exit is a coin toss
on the reference model itself cannot be held to equal iteration counts.  So, per case of tests/mfma_cases.py — the very
inputs the GPU file runs — in both flavours (adaptive, plain) and both calling patterns (one-shot pair, kept-workspace pair):
  * adaptive: rho leaves the family's value by more than 1e-3 in at least half the instances, after each solve; where the
    case clamps rho to [1, 6] the clamp binds in at least one instance (rho ends a solve on it); the unclipped and the
    non-symmetric cases are where the table says,
  * tolerance-terminated: both exits occur in the batch, in at least one of the two solves,
  * with XB on: |g|max > 1e-3 (the bound binds) and, per instance, |g|max / |x|max <= 170 — the condition under which
    tests/test_gpu_parity.py::test_matrix_core_kernel_vs_oracle's rule max(1e-5, 2^-24 |g|max / |x|max) stays at 1e-5,
  * orc32 takes orc64's (iter, solved) in both solves on >= 0.9 of the instances: the termination decisions are not marginal
    on the reference model, so at most a few instances need a replay on the GPU side.
"""
import numpy as np
import pytest

from tests import mfma_cases as mc


def test_the_table_reaches_every_variant():
    """30 cases x 2 flavours x 2 patterns = the 120 (N, REFS, XB, WS, ADP) kernels, each once; every horizon and every
    reference mode sees both settings; per horizon one unclipped case and one clamped to [1, 6]; one shared-reference and one
    per-instance-reference case with the non-symmetric table"""
    assert len(mc.CASES) == 30 and len(set(mc.CASES)) == 30
    variants = {(N, refs, xb, pattern, adaptive) for N, refs, xb in mc.CASES for pattern in mc.PATTERNS for adaptive in (False, True)}
    assert len(variants) == 120
    for N in mc.HORIZONS:
        assert {mc.setting_of(N, r, x) for r in mc.REFS for x in mc.XB} == {"tol", "fixed"}
        cs = [mc.case(N, r, x) for r in mc.REFS for x in mc.XB]
        assert sum(c["adaptive"] == mc.NOCLIP_ADAPTIVE for c in cs) == 1 and sum(c["adaptive"] == mc.TIGHT_ADAPTIVE for c in cs) == 1
    for r in mc.REFS:
        assert {mc.setting_of(N, r, x) for N in mc.HORIZONS for x in mc.XB} == {"tol", "fixed"}
    assert sorted(k[1] for k in mc.NONSYMMETRIC) == ["per_instance", "shared"]
    dP = mc.case(*mc.NONSYMMETRIC[0])["sens"][1]
    assert np.abs(dP - dP.T).max() > 0.01 * np.abs(dP).max()
    dP = mc.case(10, "zero", False)["sens"][1]
    assert np.abs(dP - dP.T).max() <= 1e-12 * np.abs(dP).max()


@pytest.mark.parametrize("key", mc.CASES, ids=mc.case_id)
def test_case_conditions(oracle_built, key):
    c = mc.case(*key)
    prob = c["prob"]
    assert c["x0"].shape == (12, mc.B)
    assert (np.abs(prob.x_max).min() < 1e17) == c["xb"] and np.abs(prob.u_max).max() < 1e17
    for adaptive in (True, False):
        for pattern in mc.PATTERNS:
            tag = f"{c['tag']} {'adaptive' if adaptive else 'plain'} {pattern}"
            x1, r64, r32 = mc.oracle_pair(c, adaptive, pattern)
            assert np.abs(x1 - c["x0"]).max() > 1e-3                      # (the second solve starts elsewhere)
            agree = np.ones(mc.B, dtype=bool)
            for k in range(2):
                agree &= (r64[k]["iter"] == r32[k]["iter"]) & (r64[k]["solved"] == r32[k]["solved"])
            rho = np.stack([r["rho"] for r in r64])
            solved = [float(r["solved"].mean()) for r in r64]
            gmax = max(float(np.abs(r["g"]).max()) for r in r64)
            ratio = max(float((np.abs(r["g"]).max(axis=(0, 1)) / np.abs(r["x"]).max(axis=(0, 1))).max()) for r in r64)
            print(f"{tag}: rho {rho.min():.3f} .. {rho.max():.3f}, solved {solved[0]:.2f} / {solved[1]:.2f}, |g|max {gmax:.2f}, "
                  f"|g|/|x| {ratio:.1f}, orc32 agrees on {agree.mean():.3f}")
            assert agree.mean() >= 0.9, f"{tag}: orc32 takes orc64's exits on {agree.mean():.3f} of the instances only"
            if adaptive:
                moved = (np.abs(rho - prob.rho) > 1e-3).mean(axis=1)
                assert moved.min() >= 0.5, f"{tag}: rho moves in {moved} of the instances"
                a = c["adaptive"]
                if a == mc.TIGHT_ADAPTIVE:
                    assert ((rho == a["rho_min"]) | (rho == a["rho_max"])).any(), f"{tag}: the clamp [1, 6] never binds"
                if a["clip"]:
                    assert rho.min() >= a["rho_min"] and rho.max() <= a["rho_max"]
            else:
                assert np.all(rho == prob.rho)
            if c["setting"] == "tol":
                assert any(0.0 < s < 1.0 for s in solved), f"{tag}: solved shares {solved}: one exit only"
                for r in r64:
                    assert np.all(r["iter"][r["solved"] == 0] == c["kw"]["max_iter"])
            else:
                for r in r64:
                    assert not r["solved"].any() and np.all(r["iter"] == c["kw"]["max_iter"])
            if c["xb"]:
                assert gmax > 1e-3, f"{tag}: the state bound never binds"
                assert ratio <= 170.0, f"{tag}: |g|max / |x|max = {ratio:.1f}"
            else:
                assert gmax == 0.0
