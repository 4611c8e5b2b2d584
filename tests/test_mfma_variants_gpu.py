"""Every horizon and variant of the matrix-core family (admm_mfma_kernel, mfma_entry.hip.h) against the fp64 restatement.

tests/mfma_cases.py lays out 30 cases (N x reference mode x XB) whose two flavours (adaptive rho, plain) and two calling
patterns (one-shot pair, kept-workspace pair) launch each of the 120 plain and adaptive kernels of the five built-in horizons;
tests/test_mfma_variants_inputs.py establishes on the oracles alone that these inputs exercise what they are meant to, and
tests/test_oracle.py (L3) that the restatement's adaptive path is the compiled reference's with references, state bounds and a
non-symmetric table.  Here the kernels run them:

  bars, per instance and solve: (iter, solved) equal the oracle's; x and u within FP32_TOL (norm-relative); rho within 1e-5
  relative; the adapted Kinf / Pinf within FP32_TOL; after the second kept-workspace solve the workspace d, v, z within 1e-5
  and the duals y, g within 2e-5 of their own norm (tests/test_gpu_parity.py::test_matrix_core_workspace_variant_vs_oracle's
  bars); g == 0 with XB off.  These are the bars test_adaptive_rho_vs_reference_golden holds this family to.

  An instance whose (iter, solved) differs from the oracle's in either solve is not dropped: its whole two-solve sequence is
  replayed on a fresh oracle with the GPU's decision imposed where the oracle's own differs (CpuSolver.set_forced_exit), it
  must meet the same bars against the replay, and the decision must have been marginal (tests/util.py:
  parity_every_instance's condition).  At most 5 % of a case's instances may need that; none in a fixed-iteration case.

Each solve prints its measured figures as a line starting with "MV " before anything is asserted
(profiles/r14_mfma_variants_parity.txt holds them)."""
import numpy as np
import pytest

import tinympc_julia_amd as t
from tests import mfma_cases as mc
from tests.util import FP32_TOL, _ratio, nrel, nrel_batch, parity_every_instance

pytestmark = pytest.mark.gpu

MAX_REPLAYED = 0.05


def _run_gpu(c, adaptive, pattern, x1):
    """the two solves of a case on the library: per solve dict(sol, st, ad, ws, status)"""
    prob, N = c["prob"], c["N"]
    name = f"mfma<12,4,{N}>"
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=mc.B)
    bs.update_settings(**c["kw"])
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if c["xref"] is not None:
        bs.set_x_ref(c["xref"])
        bs.set_u_ref(c["uref"])
    if adaptive:
        a = c["adaptive"]
        bs.set_sensitivity(*c["sens"])
        bs.set_adaptive_rho(True, a["rho_min"], a["rho_max"], a["clip"])
    if pattern == "oneshot":
        bs.set_warm_start(False)
    out = []
    for x in (c["x0"], x1):
        bs.set_x0(np.asfortranarray(x))
        status = bs.solve()
        assert bs.kernel_name == name and bs.last_launch_name == name, (bs.kernel_name, bs.last_launch_name, name)
        out.append(dict(sol=bs.get_solution(), st=bs.get_status(), ad=bs.get_adaptive_state(), status=status,
                        ws=bs.get_workspace() if pattern == "kept" else None))
    bs.close()
    return out


def _margin(c, tag, nat, imposed, it_g, so_g):
    """parity_every_instance's condition on a decision that differs: at the iteration where the two part the ORACLE's
    residual-to-tolerance ratio is within band of 1.  nat: the oracle's own solve, imposed: the same solve with the GPU's
    decision forced."""
    kw = c["kw"]
    pt, dt, ct = kw["abs_pri_tol"], kw["abs_dua_tol"], max(1, kw["check_termination"])
    assert pt > 0 and dt > 0, f"{tag}: iteration counts differ in a fixed-iteration solve"
    assert abs(it_g - nat["iter"]) <= ct, f"{tag}: stops at {it_g} vs {nat['iter']}"
    assert (imposed["iter"], imposed["solved"]) == (it_g, so_g)
    scale = max(1.0, np.abs(imposed["x"]).max(), np.abs(imposed["u"]).max())
    band = 2.0 * FP32_TOL * max(1.0, c["prob"].rho, imposed["rho"]) * scale / min(pt, dt)
    if it_g < nat["iter"] or (it_g == nat["iter"] and so_g == 1):    # the GPU saw convergence where the oracle did not
        ratio = _ratio(imposed["res"], pt, dt)
        assert 1.0 <= ratio <= 1.0 + band, f"{tag}: left early at ratio {ratio:.4f} (band {band:.3g})"
    else:                                                            # the oracle converged where the GPU went on
        ratio = _ratio(nat["res"], pt, dt)
        assert 1.0 - band <= ratio < 1.0, f"{tag}: went on at ratio {ratio:.4f} (band {band:.3g})"


def _replay(c, adaptive, pattern, b, x1, dec_g, tag):
    """instance b's two solves on fresh oracles with the GPU's decisions imposed wherever the oracle's own differ"""
    forced = [0, 0]
    seq = None
    for k in range(2):
        seq = mc.run_sequence(c, "orc64", b, adaptive, pattern, x1=x1, forced=tuple(forced))
        nat = seq[k]                                      # the oracle's own decision, given the GPU's before
        if (nat["iter"], nat["solved"]) != dec_g[k]:
            forced[k] = dec_g[k][0] if dec_g[k][1] else -1
            seq = mc.run_sequence(c, "orc64", b, adaptive, pattern, x1=x1, forced=tuple(forced))
            _margin(c, f"{tag} instance {b} solve {k}", nat, seq[k], *dec_g[k])
    assert [(s["iter"], s["solved"]) for s in seq] == dec_g
    return seq


def _compare_pair(c, adaptive, pattern, gpu, x1, r64, tag):
    """the per-instance loop with replay: measures everything, prints it, then asserts"""
    fixed = c["setting"] == "fixed"
    keys = ["x", "u"] + (["rho", "Kinf", "Pinf"] if adaptive else []) + (list(mc.STATE) if pattern == "kept" else [])
    err = {(k, key): np.zeros(mc.B) for k in range(2) for key in keys}
    replayed = []
    for b in range(mc.B):
        dec_g = [(int(g["st"]["iter"][b]), int(g["st"]["solved"][b])) for g in gpu]
        dec_o = [(int(r["iter"][b]), int(r["solved"][b])) for r in r64]
        if dec_g == dec_o:
            ref = [{key: (r[key][..., b] if key != "rho" else r[key][b]) for key in keys} for r in r64]
        else:
            assert not fixed, f"{tag}: instance {b} stops at {dec_g}, the oracle at {dec_o}, in a fixed-iteration case"
            replayed.append(b)
            ref = _replay(c, adaptive, pattern, b, x1[:, b], dec_g, tag)
        for k, g in enumerate(gpu):
            err[k, "x"][b] = nrel(g["sol"]["states"][:, :, b], ref[k]["x"])
            err[k, "u"][b] = nrel(g["sol"]["controls"][:, :, b], ref[k]["u"])
            if adaptive:
                err[k, "rho"][b] = abs(g["ad"]["rho"][b] - ref[k]["rho"]) / ref[k]["rho"]
                err[k, "Kinf"][b] = nrel(g["ad"]["Kinf"][:, :, b], ref[k]["Kinf"])
                err[k, "Pinf"][b] = nrel(g["ad"]["Pinf"][:, :, b], ref[k]["Pinf"])
            if pattern == "kept":
                for key in mc.STATE:
                    scale = max(np.abs(ref[k][key]).max(), 1e-2)
                    err[k, key][b] = np.abs(g["ws"][key][:, :, b] - ref[k][key]).max() / scale
    for k in range(2):
        print(f"MV {tag} solve {k}: " + " ".join(f"{key} {err[k, key].max():.2e}" for key in keys) +
              f" | equal exits {1.0 - len(replayed) / mc.B:.3f} replayed {len(replayed)}")
    assert len(replayed) <= MAX_REPLAYED * mc.B, f"{tag}: {len(replayed)} of {mc.B} instances needed a replay"
    for k, g in enumerate(gpu):
        assert g["status"] == int(np.any(g["st"]["solved"] == 0))
        for key in keys:
            if key in ("y", "g"):
                lim = 2e-5
            elif key == "rho":
                lim = 1e-5
            else:
                lim = FP32_TOL
            if pattern == "kept" and key in mc.STATE and k == 0:
                continue                                  # (the workspace is compared after the second solve)
            w = int(np.argmax(err[k, key]))
            assert err[k, key][w] <= lim, f"{tag} solve {k}: {key} of instance {w} off by {err[k, key][w]:.3e} (limit {lim:.0e})"
    if pattern == "kept" and not c["xb"]:
        assert np.abs(gpu[1]["ws"]["g"]).max() == 0.0
    return len(replayed)


@pytest.mark.parametrize("key", mc.CASES, ids=mc.case_id)
def test_adaptive_variants_vs_oracle(hip_lib, oracle_built, key):
    """the 60 ADP kernels: admm_mfma_kernel<12, 4, N, REFS, XB, WS, false, true>, one-shot pair (WS = false) and
    kept-workspace pair (WS = true) per case; the second solve of either enters with rho_b != rho_family, so that the
    instance's correction dK is non-zero from its first iteration"""
    c = mc.case(*key)
    for pattern in mc.PATTERNS:
        x1, r64, _ = mc.oracle_pair(c, True, pattern)
        gpu = _run_gpu(c, True, pattern, x1)
        _compare_pair(c, True, pattern, gpu, x1, r64, f"{c['tag']} {c['setting']} adaptive {pattern}")
        assert np.abs(gpu[0]["ad"]["rho"] - c["prob"].rho).max() > 1e-3


@pytest.mark.parametrize("key", mc.CASES, ids=mc.case_id)
def test_plain_variants_vs_oracle(hip_lib, oracle_built, key):
    """the 60 plain kernels: admm_mfma_kernel<12, 4, N, REFS, XB, WS>, mfma<12,4,15> and REF_PER_INSTANCE with WS among them.
    The one-shot solves are independent cold solves: parity_every_instance; the kept-workspace pair: the per-instance loop
    with replay"""
    c = mc.case(*key)
    prob = c["prob"]
    x1, r64, _ = mc.oracle_pair(c, False, "oneshot")
    gpu = _run_gpu(c, False, "oneshot", x1)
    for k, (g, r) in enumerate(zip(gpu, r64)):
        tag = f"{c['tag']} {c['setting']} plain oneshot solve {k}"
        same = (g["st"]["iter"] == r["iter"]) & (g["st"]["solved"] == r["solved"])
        ex, eu = nrel_batch(g["sol"]["states"], r["x"])[same], nrel_batch(g["sol"]["controls"], r["u"])[same]
        print(f"MV {tag}: x {ex.max():.2e} u {eu.max():.2e} | equal exits {same.mean():.3f} replayed {int((~same).sum())}")
        ref = dict(x=r["x"], u=r["u"], iter=r["iter"], solved=r["solved"], res=r["res"])
        parity_every_instance(g["sol"], g["st"], ref, lambda b: mc.make_solver(c, "orc64", b, False), r["x0"], c["kw"], prob.rho,
                              min_same=1.0 - MAX_REPLAYED, tag=tag)
        assert g["status"] == int(np.any(g["st"]["solved"] == 0))
        assert np.all(g["ad"]["rho"] == prob.rho)
    x1, r64, _ = mc.oracle_pair(c, False, "kept")
    gpu = _run_gpu(c, False, "kept", x1)
    _compare_pair(c, False, "kept", gpu, x1, r64, f"{c['tag']} {c['setting']} plain kept")


@pytest.mark.parametrize("N", mc.HORIZONS)
def test_adaptive_result_is_not_the_plain_one(hip_lib, oracle_built, monkeypatch, N):
    """the switch and the kernel were both exercised: the adaptive and the plain solutions of a case differ in bits, and
    the stream kernel's adaptive variant (TINYMPC_HIP_NO_MFMA_ADP) agrees with the matrix-core one within 2e-6 on the
    instances with equal iteration counts"""
    c = mc.case(N, "zero", True)
    x1, _, _ = mc.oracle_pair(c, True, "kept")
    adp = _run_gpu(c, True, "kept", x1)
    pln = _run_gpu(c, False, "kept", x1)
    for a, p in zip(adp, pln):
        assert not np.array_equal(a["sol"]["states"], p["sol"]["states"])
        assert not np.array_equal(a["sol"]["controls"], p["sol"]["controls"])
    monkeypatch.setenv("TINYMPC_HIP_NO_MFMA_ADP", "1")
    prob = c["prob"]
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=mc.B)
    bs.update_settings(**c["kw"])
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_sensitivity(*c["sens"])
    a = c["adaptive"]
    bs.set_adaptive_rho(True, a["rho_min"], a["rho_max"], a["clip"])
    same = np.ones(mc.B, dtype=bool)
    for k, x in enumerate((c["x0"], x1)):
        bs.set_x0(np.asfortranarray(x))
        bs.solve()
        assert bs.kernel_name == "stream4<12,4>" and bs.last_launch_name == "stream4<12,4>", bs.last_launch_name
        sol, st = bs.get_solution(), bs.get_status()
        same &= (st["iter"] == adp[k]["st"]["iter"]) & (st["solved"] == adp[k]["st"]["solved"])
        ex = nrel_batch(sol["states"], adp[k]["sol"]["states"])[same].max()
        eu = nrel_batch(sol["controls"], adp[k]["sol"]["controls"])[same].max()
        print(f"MV {c['tag']} stream4 vs mfma adaptive solve {k}: x {ex:.2e} u {eu:.2e} | equal iterations {same.mean():.3f}")
        assert ex <= 2e-6 and eu <= 2e-6
    assert same.mean() >= 0.9                             # (the comparison is of the batch, not of a few instances)
    bs.close()


# The refill variant (admm_mfma_kernel<..., WS = false, RF = true>) at the other horizons.  launch_mfma_refill refills only from
# two rounds of resident workgroups on: tiles >= 2 x workgroups per CU x 256 CUs, the batch a multiple of 64.  Workgroups
# per CU by mfma_blocks_per_cu (admm_mfma.hip.h): 2 where 3 N + 3 (N - 1) <= 120 without a state bound — N = 10, 15, 20 —
# else 1; the launcher asks the runtime for the kernel's real occupancy, which is 2 for <12,4,10, REF_ZERO, XB> too (250
# registers).  So, per N and for both cases:
#   N = 10, 15, 20:  2 x 2 x 256 = 1024 tiles = 65 536 instances (zero references; taken for the state-bound case as well)
#   N = 25:          2 x 1 x 256 =  512 tiles = 32 768 instances at least: 40 960, the existing N = 30 test's batch
REFILL_BATCH = {10: 65536, 15: 65536, 20: 65536, 25: 40960}


@pytest.mark.parametrize("case", ["zero_refs_ct10", "state_bounds_ct20"])
@pytest.mark.parametrize("N", sorted(REFILL_BATCH))
def test_mfma_refill_is_the_same_solve_at_the_other_horizons(hip_lib, monkeypatch, N, case):
    """tests/test_gpu_parity.py::test_mfma_refill_is_the_same_solve's zero-reference and state-bound cases at N = 10, 15, 20,
    25: bit for bit the plain launch (TINYMPC_HIP_NO_REFILL)"""
    prob = t.problems.quadrotor(N, u_bound=0.5)
    B = REFILL_BATCH[N]
    rng = np.random.default_rng(5)
    x0 = t.problems.quadrotor_x0(B, seed=9)
    x0[:, rng.integers(0, B, B // 3)] *= 0.1               # a third of the instances are easy: slots turn over at different rates
    ct = {"zero_refs_ct10": 10, "state_bounds_ct20": 20}[case]
    kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=ct)
    outs = []
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("TINYMPC_HIP_NO_REFILL", env)
        bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
        bs.update_settings(**kw)
        if case == "state_bounds_ct20":
            xmin, xmax = prob.x_min.copy(), prob.x_max.copy()
            xmin[:3], xmax[:3] = -0.25, 0.25                  # finite state bounds: the state dual is carried (XB)
            bs.set_bound_constraints(xmin, xmax, prob.u_min, prob.u_max)
        else:
            bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        bs.set_warm_start(False)
        bs.set_x0(x0)
        status = bs.solve()
        assert bs.kernel_name == f"mfma<12,4,{N}>" and bs.last_launch_name == f"mfma<12,4,{N}>"
        outs.append((status, bs.get_solution(), bs.get_status()))
        bs.close()
    (s1, sol1, st1), (s2, sol2, st2) = outs
    assert s1 == s2
    for k in ("iter", "solved", "residuals"):
        assert np.array_equal(st1[k], st2[k]), k
    assert np.array_equal(sol1["states"], sol2["states"]) and np.array_equal(sol1["controls"], sol2["controls"])
    assert len(np.unique(st1["iter"])) > 3 and np.all(st1["iter"] % ct == 0)
