"""Every form of the two run-time-shape kernels against the oracle: admm_streamg_kernel<NX, NU, 4, ...> on all 25 shapes of its
grid, admm_generic_kernel at the edges of its shape range, and the stream kernel's LDS image around 48 KiB, 64 KiB and the
150 KiB routing limit.  The inputs are tests/stream_forms_cases.py's; tests/test_stream_forms_inputs.py holds them, on the CPU
oracles alone, to the conditions under which the bars below mean something.

Part 1.  launch_streamg (csrc/streamg_entry.hip.h) picks one of 28 templates per shape.  Every arm runs kept-workspace
(set_warm_start(True) + reset(): OS = false) and then one-shot (set_warm_start(False): OS = true):

  arm       precision  RT      EXT  HET  ADP   template admm_streamg_kernel<NX, NU, 4, ...>          setup
  plain     0          double  0    no   no    <double, 0, false, OS>
  ext1      0          double  1    no   no    <double, 1, false, OS>                               affine term, cones
  ext2      0          double  2    no   no    <double, 2, false, OS>                               ext1 + linear rows
  het       0          double  0    yes  no    <double, 0, true, OS>                                host, and device
  het_ext2  0          double  2    yes  no    <double, 2, true, OS>                                device (fill kernel)
  adp       0          double  0    no   yes   <double, 0, false, OS, true>
  plain     1          float   0    no   no    <float, 0, false, OS>
  ext2      1          float   2    no   no    <float, 2, false, OS>
  het_ext2  1          float   2    yes  no    <float, 2, true, OS>                                 device (fill kernel, float)
  adp       1          float   0    no   yes   <float, 0, false, OS, true>

20 of the 28 per shape; the other eight are <double, 1, true, OS>, <float, 1, *, OS>, <float, 0, true, OS> — the EXT = 1 and
plain rows of a pack whose EXT = 2 form runs here (EXT only removes code: EXT = 2 holds the cone and the row passes, EXT = 1
the cone pass alone).  kernel_name and last_launch_name are the bare "stream4<nx,nu>" for this whole family, so the form that
ran follows from the configuration (precision, extensions, families, warm start, adaptive rho) by launch_streamg's own
dispatch, which this table restates; effective_precision tells RT, families_setup_mode the fill route.

Bars, none new: parity_every_instance at FP32_TOL with min_same = 0.9 at precision 0 (adaptive arms: the oracle adapts too, the
imposed-exit replay included, and on the instances whose exit agrees rho within 1e-5 relative, the adapted Kinf and Pinf within
FP32_TOL); precision1_limit(orc32, orc64) at precision 1 (rho: adaptive_pair's rule); the host and the device route of the
per-instance families within 2e-6 of each other; one-shot and kept-workspace solves from a cold workspace stop at the same
iterations; precision 2: 1e-6 and the oracle's exact (iter, solved), the oracle fed the same fp32 inputs.

Part 2.  The generic kernel: (1,1), (5,5), (13,1), (16,5) with LIN_MAX_ROWS state rows, (64,1), (33,32), (64,32) at N = 4,
(5,2) and — with the stream kernel switched off — (4,1) at N = 2.  Arms: plain and ext2 at precision 0, plain at precision 1
and 2, per-instance bounds and per-instance rows at precision 0 and 2, adaptive rho plain and with the affine term and the
state cone (the oracle runs that combination: oracle/tinympc_oracle_body.inc adapt_rho carries the affine term in its primal
residual).  No arm is left out: t.host_sensitivity takes 2.1 s at (64,1) and 0.12 s at (64,32) on the CPU.  At 64 states a
solve of 70 instances costs the generic kernel 7 ms an iteration, so those two cases stop at 25 iterations (the others at 50).
A shape over the limit, (65,1) and (4,33), is refused by name when the solver is created — the routes are asked there — so
nothing is launched and no solver exists to set precision 2 on: select_kernel's precision-2 twin of the message cannot be
reached through the API.

Every comparison prints a line "SF <kernel> | <case> <arm> | p<precision> <form> | iter lo..hi | same .. | x .. u .. bar .."
(adaptive: "| rho ..") before it asserts; profiles/stream_forms_routes.txt is a run's output."""
import numpy as np
import pytest

import tinympc_julia_amd as t
from tests import stream_forms_cases as sc
from tests.util import FP32_TOL, nrel_batch, parity_every_instance

pytestmark = pytest.mark.gpu

TIGHT = 1e-6        # tests/test_precision2_gpu.py
SWITCHES = ("TINYMPC_HIP_NO_QUAD", "TINYMPC_HIP_NO_MFMAT", "TINYMPC_HIP_NO_MFMAC", "TINYMPC_HIP_NO_MFMAR")


def _solver(case, a, setup="host"):
    prob = case["prob"]
    if a["het"]:
        bs = t.BatchSolver.from_families(*case["fam"], prob.N, setup=setup)
    else:
        bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=case["x0"].shape[1])
    bs.update_settings(**case["kw"])
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if a["ib"] is not None:
        bs.set_instance_bounds(*a["ib"])
    if a["refs"]:
        bs.set_x_ref(case["xref"])
        bs.set_u_ref(case["uref"])
    if a["ext"]:
        cu, cx = a["cones"]
        bs.set_fdyn(case["fdyn"])
        if len(cu[0]) or len(cx[0]):
            bs.set_cone_constraints(cu[0], cu[1], cu[2], cx[0], cx[1], cx[2])
    if a["rows"] is not None:
        bs.set_linear_constraints(*a["rows"])
    if a["il"] is not None:
        bs.set_instance_linear(*a["il"])
    if a["adaptive"]:
        bs.set_sensitivity(*a["sens"])
        bs.set_adaptive_rho(True, sc.ADAPTIVE["rho_min"], sc.ADAPTIVE["rho_max"], sc.ADAPTIVE["clip"])
    bs.set_x0(case["x0"])
    return bs


def _both_forms(bs, case, a, pair, kernel, precision, base=None):
    """the arm kept-workspace and one-shot, both from a cold workspace, at the solver's precision: each against orc64 at the
    precision's bar; returns the one-shot solution"""
    r64, r32, limit, e32, same32 = pair
    make = a["make"]("orc64")
    iters, sol = {}, None
    for form in ("kept", "one_shot"):
        bs.set_warm_start(form == "kept")
        bs.reset()                               # (a cold workspace; the adapted rho returns to the family's)
        bs.solve()
        assert bs.kernel_name == kernel and bs.last_launch_name == kernel, (a["tag"], form, bs.kernel_name, bs.last_launch_name, kernel)
        assert bs.effective_precision == precision
        sol, st = bs.get_solution(), bs.get_status()
        agree = (st["iter"] == r64["iter"]) & (st["solved"] == r64["solved"])
        ex = nrel_batch(sol["states"], r64["x"])[agree].max() if agree.any() else float("nan")
        eu = nrel_batch(sol["controls"], r64["u"])[agree].max() if agree.any() else float("nan")
        bar = {0: FP32_TOL, 1: limit, 2: TIGHT}[precision]
        line = (f"SF {kernel} | {a['tag']} | p{precision} {form} | iter {st['iter'].min()}..{st['iter'].max()} | same {agree.mean():.3f} | "
                f"x {ex:.2e} u {eu:.2e} bar {bar:.1e}")
        if a["adaptive"]:
            ad = bs.get_adaptive_state()
            er = (np.abs(ad["rho"] - r64["rho"]) / r64["rho"])[agree].max()
            ek = nrel_batch(ad["Kinf"], r64["Kinf"])[agree].max()
            ep = nrel_batch(ad["Pinf"], r64["Pinf"])[agree].max()
            rbar = 1e-5 if precision == 0 else sc.rho_limit(r64, r32)[0]
            line += f" | rho {er:.2e} bar {rbar:.1e} Kinf {ek:.2e} Pinf {ep:.2e}"
        print(line)
        if base is not None:
            assert not (np.array_equal(sol["states"], base["states"]) and np.array_equal(sol["controls"], base["controls"])), \
                f"{a['tag']} p{precision} {form}: bit-identical to the precision-0 result"
        if precision == 2:
            assert np.array_equal(st["iter"], r64["iter"]) and np.array_equal(st["solved"], r64["solved"]), f"{a['tag']} p2 {form}"
            assert ex <= TIGHT and eu <= TIGHT, f"{a['tag']} p2 {form}: x {ex:.3e} u {eu:.3e}"
        else:
            parity_every_instance(sol, st, r64, make, case["x0"], case["kw"], a["rho"], tol=bar, min_same=0.9,
                                  tag=f"{kernel} {a['tag']} p{precision} {form}")
        if a["adaptive"]:
            assert er <= rbar, f"{a['tag']} p{precision} {form}: adapted rho off by {er:.2e}"
            if precision == 0:
                assert ek <= FP32_TOL and ep <= FP32_TOL, f"{a['tag']} {form}: adapted Kinf {ek:.2e} Pinf {ep:.2e}"
        iters[form] = st["iter"].copy()
    assert np.array_equal(iters["kept"], iters["one_shot"]), f"{a['tag']} p{precision}: one-shot and kept-workspace solves stop apart"
    return sol, st


# ---- Part 1: the stream grid ----
@pytest.mark.parametrize("shape", sc.GRID, ids=sc.shape_id)
def test_stream_forms(hip_lib, oracle_built, monkeypatch, shape):
    for s in SWITCHES:
        monkeypatch.setenv(s, "1")
    nx, nu = shape
    kernel = f"stream4<{nx},{nu}>"
    case = sc.stream_case(nx, nu)
    routes = {}
    for name, setups in (("plain", ("host",)), ("ext1", ("host",)), ("ext2", ("host",)), ("het", ("host", "device")),
                         ("het_ext2", ("device",)), ("adp", ("host",))):
        a, pair = sc.arm(case, name), (sc.arm_pair(case, name) if name in sc.FLOAT_ARMS else (sc.arm_ref(case, name),) + (None,) * 4)
        for setup in setups:
            bs = _solver(case, a, setup)
            if a["het"]:
                assert bs.families_setup_mode == (2 if setup == "device" else 1)
            base, st = _both_forms(bs, case, a, pair, kernel, 0)
            if name == "het":
                routes[setup] = (base, st)
            if name in sc.FLOAT_ARMS:
                bs.set_strict_precision(True)
                bs.set_precision(1)
                _both_forms(bs, case, a, pair, kernel, 1, base=base)
            bs.close()
    (sh, th), (sd, td) = routes["host"], routes["device"]
    both = (th["iter"] == td["iter"]) & (th["solved"] == td["solved"])
    ex, eu = nrel_batch(sd["states"], sh["states"])[both].max(), nrel_batch(sd["controls"], sh["controls"])[both].max()
    print(f"SF {kernel} | {case['tag']} het | host against device route | same {both.mean():.3f} | x {ex:.2e} u {eu:.2e} bar 2.0e-06")
    assert both.mean() >= 0.9 and ex <= 2e-6 and eu <= 2e-6


# ---- Part 2: the generic kernel at the edges of its shape range ----
@pytest.mark.parametrize("shape", sc.GENERIC_SHAPES, ids=sc.shape_id)
def test_generic_forms(hip_lib, oracle_built, monkeypatch, shape):
    for s in SWITCHES:
        monkeypatch.setenv(s, "1")
    if shape[:2] in sc.GRID:
        monkeypatch.setenv("TINYMPC_HIP_NO_STREAM", "1")
    case = sc.generic_case(*shape)
    for name in sc.generic_arms(case):
        # (orc32, for the precision-1 bar, only where precision 1 runs: the oracle side is what a 64-state test costs)
        a, pair = sc.arm(case, name), (sc.arm_pair(case, name) if name == "plain" else (sc.arm_ref(case, name),) + (None,) * 4)
        tail = {"ib": "ib", "il": "il"}.get(name)
        bs = _solver(case, a)
        base, _ = _both_forms(bs, case, a, pair, f"generic<{tail}>" if tail else "generic", 0)
        if name == "plain":
            bs.set_strict_precision(True)
            bs.set_precision(1)
            _both_forms(bs, case, a, pair, "generic", 1, base=base)
        if name in ("plain", "ib", "il"):
            bs.set_precision(2)
            _both_forms(bs, case, a, pair, f"generic<f64;{tail}>" if tail else "generic<f64>", 2)
        bs.close()


@pytest.mark.parametrize("shape", [(65, 1), (4, 33)], ids=sc.shape_id)
def test_generic_shape_limit_is_refused_by_name(hip_lib, shape):
    """a shape over GEN_MAX_NX = 64 / GEN_MAX_NU = 32 has no kernel.  The routes are asked when the solver is created
    (alloc_batch -> select_kernel), so creation itself is refused, with the limit in the message, and nothing can be launched:
    no solver exists to set precision 2 on or to solve with — select_kernel's precision-2 twin of the message is reached
    only through the same door.  Both constructors are held to it."""
    from tests.test_gpu_parity import _random_problem
    nx, nu = shape
    prob = _random_problem(np.random.default_rng(nx + nu), nx, nu, 4, bounded=True)
    with pytest.raises(t.TinyMPCError, match=r"generic kernel limits \(nx <= 64, nu <= 32\)"):
        t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=3)
    fam = tuple(np.repeat(m[:, :, None], 3, axis=2) for m in (prob.A, prob.B, prob.Q, prob.R)) + (np.full(3, prob.rho),)
    with pytest.raises(t.TinyMPCError, match="limits|stream-kernel instantiation"):
        t.BatchSolver.from_families(*fam, prob.N)


# ---- Part 3: long horizons on the stream kernel ----
def test_stream_long_horizons(hip_lib, oracle_built, monkeypatch):
    """(12,4): streamg_lds_bytes is 6 976 + 128 N bytes at precision 0 (CP = 216 doubles for each of four roles, 128 B of bounds a
    knot, 64 B of diagonals).  N = 330 is the first horizon past 48 KiB — from there launch_streamg raises the kernel's dynamic
    LDS limit —, N = 458 the first past 64 KiB, N = 1145 the last that route_stream lets through (150 KiB); N = 1146 is the
    generic kernel's.  Five instances, 10 fixed iterations, input bounds only; kept-workspace and one-shot."""
    for s in SWITCHES:
        monkeypatch.setenv(s, "1")
    hz = sc.long_horizons()
    assert hz == dict(solved=[330, 458, 1145], generic=1146)
    assert sc.stream_lds_bytes(12, 4, 329) <= 48 * 1024 < sc.stream_lds_bytes(12, 4, 330) == 6976 + 128 * 330
    for N in hz["solved"] + [hz["generic"]]:
        case = sc.long_case(N)
        prob = case["prob"]
        r64 = sc.long_pair(case)[0]
        kernel = "generic" if N == hz["generic"] else "stream4<12,4>"
        bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=5)
        bs.update_settings(**case["kw"])
        bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        bs.set_x0(case["x0"])
        for form in ("kept", "one_shot"):
            bs.set_warm_start(form == "kept")
            bs.reset()
            bs.solve()
            assert bs.kernel_name == kernel and bs.last_launch_name == kernel, (N, form, bs.kernel_name, bs.last_launch_name)
            sol, st = bs.get_solution(), bs.get_status()
            ex, eu = nrel_batch(sol["states"], r64["x"]).max(), nrel_batch(sol["controls"], r64["u"]).max()
            print(f"SF {kernel} | {case['tag']} | p0 {form} | iter {st['iter'].min()}..{st['iter'].max()} | x {ex:.2e} u {eu:.2e} bar {FP32_TOL:.1e}")
            parity_every_instance(sol, st, r64, sc.pc.make_oracle(case), case["x0"], case["kw"], prob.rho, tol=FP32_TOL,
                                  min_same=1.0, tag=f"{kernel} N={N} {form}")
        bs.close()
