"""Precision 1 (tinympc_set_precision(s, 1): fp32 recurrences) against the oracles, on every kernel that has a float form:
the lanes-per-instance kernels (admm_quad_kernel<..., RT = float, ...>, all 18 built-in entries), the run-time-horizon stream
kernel (admm_streamg_kernel<NX, NU, G, float, EXT, HET, OS>) and the generic kernel (admm_generic_kernel<float, float>).

The float kernels are not the double ones with another type: the coefficient pack is rounded to float on the host, the
register / LDS placement of the coefficients and the LDS size follow sizeof(RT), and the FOLD form exists for doubles only.

The bar.  FP32_TOL is documented as not met at precision 1 (include/tinympc_hip.h), so the bar comes from the reference model,
per case, on the CPU (tests/util.py: precision1_limit): e32_case = orc32's worst distance from orc64 (orc32: the same loop in
fp32 with the fp64-computed cache), limit_case = max(FP32_TOL, 4 * e32_case).  The kernel is compared with orc64 through
parity_every_instance at that limit, marginal termination decisions replayed with set_forced_exit.  The factor 4: orc32 is one
realisation of fp32 rounding, the kernel (summation order, FMA contraction, float-rounded coefficients) another; their
worst-of-a-batch errors differ by a small factor, a structural fault (a wrong LDS offset, a row of the wrong lane role, a bound
at the wrong knot) moves the result by orders of magnitude.  tests/test_precision1_inputs.py asserts, on the oracles alone and on
these very inputs (tests/precision1_cases.py), that no limit exceeds 8e-4, that the oracles agree on the exit of >= 0.9 of the
instances, that bounds bind and that both exits occur.

Every solve asserts the kernel that ran, effective_precision == 1, and a result that differs in bits from the same solver's
precision-0 result on the same inputs: a silent fall-back to the fp64-recurrence kernels cannot pass.

Each comparison prints a line "P1 <kernel> | <case> | <form> | e32 .. x .. u .. ratio .. same .." before it asserts
(profiles/r13_precision1_parity.txt is a run's output)."""
import numpy as np
import pytest

import tinympc_julia_amd as t
from tests import precision1_cases as pc
from tests.util import nrel_batch, parity_every_instance

pytestmark = pytest.mark.gpu


def _configure(bs, case):
    prob = case["prob"]
    bs.update_settings(**case["kw"])
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if case["xref"] is not None and "fam" not in case:
        bs.set_x_ref(case["xref"])
        bs.set_u_ref(case["uref"])


def _solver(case):
    prob = case["prob"]
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=case["x0"].shape[1])
    _configure(bs, case)
    return bs


def _set_form(bs, form):
    """one-shot: cold start, nothing kept (the OS / UNI loop forms where the kernel has them); kept: the workspace-carrying
    kernel started cold"""
    if form == "one_shot":
        bs.set_warm_start(False)
    else:
        bs.set_warm_start(True)
        bs.reset()


def _is_precision1(bs, name, base):
    """the three assertions of every precision-1 solve; base: the precision-0 solution of the same solver and inputs"""
    assert bs.kernel_name == name and bs.last_launch_name == name, (bs.kernel_name, bs.last_launch_name, name)
    assert bs.effective_precision == 1
    sol = bs.get_solution()
    assert not (np.array_equal(sol["states"], base["states"]) and np.array_equal(sol["controls"], base["controls"])), \
        f"{name}: bit-identical to the precision-0 result"
    return sol


def _record(name, tag, form, e32, limit, sol_x, sol_u, ref, agree):
    """the kernel's worst error against orc64 over the instances whose exit agrees (the others are replayed by
    parity_every_instance), printed before anything is asserted"""
    ex = nrel_batch(sol_x, ref["x"])[agree].max() if agree.any() else float("nan")
    eu = nrel_batch(sol_u, ref["u"])[agree].max() if agree.any() else float("nan")
    ratio = max(ex, eu) / e32 if e32 > 0 else float("inf")
    print(f"P1 {name} | {tag} | {form} | e32 {e32:.2e} limit {limit:.2e} x {ex:.2e} u {eu:.2e} ratio {ratio:.2f} same {agree.mean():.3f}")


def _compare(bs, name, case, form, base, pair, make):
    r64, r32, limit, e32, same32 = pair
    sol = _is_precision1(bs, name, base)
    st = bs.get_status()
    agree = (st["iter"] == r64["iter"]) & (st["solved"] == r64["solved"])
    _record(name, case["tag"], form, e32, limit, sol["states"], sol["controls"], r64, agree)
    x3 = case["xref"] if case["xref"] is not None and np.ndim(case["xref"]) == 3 else None
    u3 = case["uref"] if x3 is not None else None
    rho = float(np.max(case["fam"][4])) if "fam" in case else case["prob"].rho
    parity_every_instance(sol, st, r64, make, case["x0"], case["kw"], rho, xref=x3, uref=u3, tol=limit, min_same=0.9,
                          tag=f"{name} {case['tag']} {form}")


# ---- (a) every built-in quad entry ----
@pytest.mark.parametrize("entry", pc.QUAD_ENTRIES, ids=pc.entry_id)
def test_quad_entry_float_recurrences(hip_lib, oracle_built, monkeypatch, entry):
    """24 solves per entry: state bounds off / on (template flag XB) x reference mode (REF_ZERO, REF_SHARED, REF_PER_INSTANCE)
    x fixed iterations / tolerance-terminated x one-shot / workspace-carrying, on two workgroups with a part-filled last
    wavefront and quad row.  TINYMPC_HIP_GROUP forces the entry and keeps the matrix-core routes away.  Where the shape has
    the cheaper loop forms (LOOPV), the switches that take them away one by one: all three forms of the float kernel run."""
    nx, nu, N, G = entry
    B = pc.BATCH[G]
    monkeypatch.setenv("TINYMPC_HIP_GROUP", str(G))
    name = f"quad<{nx},{nu},{N},g{G}>"
    for xb in pc.XB:
        for refs in pc.REFS:
            for setting in pc.SETTINGS:
                case = pc.quad_case(nx, nu, N, B, xb, refs, setting)
                pair = pc.oracle_pair(case)
                bs = _solver(case)                          # (a fresh solver: REF_ZERO is a solver that never saw references)
                bs.set_x0(case["x0"])
                bs.set_warm_start(False)
                bs.solve()
                assert bs.kernel_name == name and bs.effective_precision == 0
                base = bs.get_solution()
                bs.set_precision(1)
                for form in ("one_shot", "kept"):
                    _set_form(bs, form)
                    bs.solve()
                    _compare(bs, name, case, form, base, pair, pc.make_oracle(case))
                if entry in pc.LOOPV and (xb, refs, setting) == (True, "shared", "fixed"):
                    bs.set_warm_start(False)
                    for off in (("TINYMPC_HIP_NO_UNI",), ("TINYMPC_HIP_NO_OS",), ("TINYMPC_HIP_NO_UNI", "TINYMPC_HIP_NO_OS")):
                        for sw in off:
                            monkeypatch.setenv(sw, "1")
                        bs.reload_switches()
                        bs.solve()
                        _compare(bs, name, case, "one_shot " + "+".join(s[12:] for s in off), base, pair, pc.make_oracle(case))
                        for sw in off:
                            monkeypatch.delenv(sw)
                    bs.reload_switches()
                bs.close()


# ---- (b) continued solve from a kept workspace ----
@pytest.mark.parametrize("entry", pc.CONTINUED, ids=pc.entry_id)
def test_continued_solve_from_a_kept_workspace(hip_lib, oracle_built, monkeypatch, entry):
    """solve from x0, then from A x0 + B u0 (the oracle's u0) without a reset: the second solve against persistent per-instance
    oracles that did the same two solves (tests/test_stream_f64_gpu.py::test_workspace_kept_closed_loop's pattern).  State
    bounds on, shared references, 20 iterations each."""
    nx, nu, N, G = entry
    monkeypatch.setenv("TINYMPC_HIP_GROUP", str(G))
    name = f"quad<{nx},{nu},{N},g{G}>"
    case = pc.quad_case(nx, nu, N, pc.BATCH[G], True, "shared", "fixed", max_iter=20)
    x1, r64, limit, e32, same = pc.continued_pair(case)
    out = {}
    for precision in (0, 1):
        bs = _solver(case)
        bs.set_warm_start(True)
        bs.set_precision(precision)
        for x in (case["x0"], x1):
            bs.set_x0(x)
            bs.solve()
        assert bs.kernel_name == name and bs.last_launch_name == name and bs.effective_precision == precision
        out[precision] = (bs.get_solution(), bs.get_status())
        bs.close()
    sol, st = out[1]
    assert not (np.array_equal(sol["states"], out[0][0]["states"]) and np.array_equal(sol["controls"], out[0][0]["controls"]))
    agree = (st["iter"] == r64["iter"]) & (st["solved"] == r64["solved"])
    _record(name, case["tag"], "second solve, workspace kept", e32, limit, sol["states"], sol["controls"], r64, agree)
    second = dict(case, x0=x1)
    parity_every_instance(sol, st, r64, pc.make_oracle(case), second["x0"], case["kw"], case["prob"].rho, tol=limit, min_same=0.9,
                          tag=f"{name} continued")


# ---- (c) fused closed loop ----
@pytest.mark.parametrize("entry", pc.CLOSED_LOOP, ids=pc.entry_id)
def test_fused_closed_loop(hip_lib, oracle_built, monkeypatch, entry):
    """mpc_rollout(5), 10 iterations per step, against the host-stepped oracle loop of
    tests/test_gpu_parity.py::test_fused_mpc_rollout_batch_vs_oracle: applied controls and plant states"""
    nx, nu, N, G = entry
    monkeypatch.setenv("TINYMPC_HIP_GROUP", str(G))
    name = f"quad<{nx},{nu},{N},g{G}>"
    case = pc.quad_case(nx, nu, N, pc.BATCH[G], False, "zero", "fixed", max_iter=10)
    r64, limit, e32, same = pc.closed_loop_pair(case, pc.LOOP_STEPS)
    logs = {}
    for precision in (0, 1):
        bs = _solver(case)
        bs.set_precision(precision)
        bs.set_x0(case["x0"])
        logs[precision] = bs.mpc_rollout(pc.LOOP_STEPS)
        assert bs.kernel_name == name and bs.last_launch_name == name and bs.effective_precision == precision
        bs.close()
    log = logs[1]
    assert not (np.array_equal(log["u"], logs[0]["u"]) and np.array_equal(log["x"], logs[0]["x"]))
    _record(name, case["tag"], f"mpc_rollout({pc.LOOP_STEPS})", e32, limit, log["x"], log["u"], r64, np.ones(log["u"].shape[2], dtype=bool))
    assert np.all(log["iter"] == 10) and not log["solved"].any()
    eu, ex = nrel_batch(log["u"], r64["u"]), nrel_batch(log["x"], r64["x"])
    assert eu.max() <= limit, f"applied controls: worst {eu.max():.3e} (instance {eu.argmax()}, limit {limit:.1e})"
    assert ex.max() <= limit, f"plant states: worst {ex.max():.3e} (instance {ex.argmax()}, limit {limit:.1e})"


# ---- (d) stream and generic kernels ----
STREAM = [("cartpole17_zero", "stream4<4,1>"), ("cartpole17_shared", "stream4<4,1>"), ("cartpole17_per_instance", "stream4<4,1>"),
          ("quadrotor7_zero", "stream4<12,4>"), ("quadrotor7_shared", "stream4<12,4>"), ("quadrotor7_per_instance", "stream4<12,4>"),
          ("rocket_cones12", "stream4<6,3>"), ("linear9", "stream4<4,1>"), ("families17", "stream4<4,1>"),
          ("random_3_2_3", "stream4<3,2>"), ("random_5_2_9", "generic"), ("cartpole17_shared", "generic")]


@pytest.mark.parametrize("case_name,kernel", STREAM, ids=[f"{c}-{k.split('<')[0]}" for c, k in STREAM])
def test_stream_and_generic_float_recurrences(hip_lib, oracle_built, monkeypatch, case_name, kernel):
    """the stream kernel box-only in all three reference modes on (4,1) and (12,4), with the affine term and one cone per side
    (EXT = 1), with linear rows (EXT = 2), as a per-instance family (HET) and at N = 3; the generic kernel on (5,2) and, with the
    stream kernel switched off, on the cartpole.  One-shot (OS) and workspace-carrying, batch 70: two stream workgroups."""
    monkeypatch.setenv("TINYMPC_HIP_NO_QUAD", "1")
    monkeypatch.setenv("TINYMPC_HIP_NO_MFMAT", "1")
    if kernel == "generic" and case_name.startswith("cartpole"):
        monkeypatch.setenv("TINYMPC_HIP_NO_STREAM", "1")
    case = pc.STREAM_CASES[case_name]()
    looped = "make" in case
    pair = (pc.loop_pair if looped else pc.oracle_pair)(case)
    make = case["make"]("orc64") if looped else pc.make_oracle(case)
    prob = case["prob"]
    if "fam" in case:
        bs = t.BatchSolver.from_families(*case["fam"], prob.N)
        _configure(bs, case)
    else:
        bs = _solver(case)
    if case_name.startswith("rocket_cones"):
        bs.set_fdyn(prob.fdyn)
        bs.set_cone_constraints(*pc.ROCKET_CONES)
    if "lin" in case:
        bs.set_linear_constraints(*case["lin"])
    bs.set_strict_precision(True)                 # (where the shape has a matrix-core kernel, precision 1 would stay on it)
    bs.set_x0(case["x0"])
    _set_form(bs, "kept")                         # (a precision-0 one-shot solve with cones would go to the matrix cores)
    bs.solve()
    assert bs.kernel_name == kernel and bs.last_launch_name == kernel and bs.effective_precision == 0
    base = bs.get_solution()
    bs.set_precision(1)
    for form in ("one_shot", "kept"):
        _set_form(bs, form)
        bs.solve()
        _compare(bs, kernel, case, form, base, pair, make)
    bs.close()


# ---- (e) adaptive rho ----
@pytest.mark.parametrize("N,kernel", [(20, "quad<4,1,20,g4>"), (17, "stream4<4,1>")])
def test_adaptive_rho_float_recurrences(hip_lib, oracle_built, monkeypatch, N, kernel):
    """the ADP float kernels: launch_quad_adp<S, float, ...> of the four-lanes-per-instance cartpole entry and the stream
    kernel's ADP form, against oracles given the library's own sensitivities: solution at the case's limit, the adapted rho of
    every instance whose exit agrees at the same rule's limit on rho"""
    if kernel.startswith("quad"):
        monkeypatch.setenv("TINYMPC_HIP_GROUP", "4")
    else:
        monkeypatch.setenv("TINYMPC_HIP_NO_QUAD", "1")
    case = pc.adaptive_case(N)
    r64, limit, e32, same, rho_limit, drho = pc.adaptive_pair(case)
    bs = _solver(case)
    bs.set_sensitivity(*case["sens"])
    bs.set_adaptive_rho(True, pc.ADAPTIVE["rho_min"], pc.ADAPTIVE["rho_max"], pc.ADAPTIVE["clip"])
    bs.set_warm_start(False)
    bs.set_x0(case["x0"])
    bs.solve()
    assert bs.kernel_name == kernel and bs.effective_precision == 0
    base = bs.get_solution()
    bs.set_precision(1)
    for form in ("one_shot", "kept"):
        _set_form(bs, form)
        bs.reset()                              # (the adapted rho outlives a solve; reset returns every instance to the family's)
        bs.solve()
        sol = _is_precision1(bs, kernel, base)
        st, ad = bs.get_status(), bs.get_adaptive_state()
        agree = (st["iter"] == r64["iter"]) & (st["solved"] == r64["solved"])
        _record(kernel, case["tag"], form, e32, limit, sol["states"], sol["controls"], r64, agree)
        er = (np.abs(ad["rho"] - r64["rho"]) / r64["rho"])[agree].max()
        print(f"P1 {kernel} | {case['tag']} | {form} | rho within {er:.2e} (orc32 {drho:.2e}, limit {rho_limit:.1e})")
        parity_every_instance(sol, st, r64, case["make"]("orc64"), case["x0"], case["kw"], pc.ADAPTIVE["rho_max"], tol=limit,
                              min_same=0.9, tag=f"{kernel} {case['tag']} {form}")
        assert er <= rho_limit, f"{kernel} {form}: adapted rho off by {er:.2e}"
        assert np.abs(ad["rho"] - case["prob"].rho).max() > 0.05
    bs.close()
