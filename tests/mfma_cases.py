"""Inputs of the matrix-core family's variant tests: one place, used by the CPU-only conditions
(tests/test_mfma_variants_inputs.py, the two oracles alone) and by the GPU comparison (tests/test_mfma_variants_gpu.py), so
that what the conditions establish is what the kernels are run on.  Its model is tests/precision1_cases.py.

Per built-in horizon (12, 4, N), N in {10, 15, 20, 25, 30}, mfma_entry.hip.h instantiates 12 plain kernels
admm_mfma_kernel<12, 4, N, REFS, XB, WS>, 12 adaptive-rho ones <..., RF = false, ADP = true> and 4 refill ones.  launch_mfma
decides the variant from the solve:

    reference mode of the case      REFS   zero: no reference set (REF_ZERO) / shared: 2-D references (REF_SHARED) /
                                           per_instance: 3-D references (REF_PER_INSTANCE)
    XB of the case                  XB     a finite state bound is enabled (rows 0-2 at +-0.31)
    calling pattern                 WS     "oneshot": set_warm_start(False), cold start, workspace not kept -> WS = false
                                           "kept": the default, workspace read and kept              -> WS = true
    flavour                         ADP    set_adaptive_rho(True) -> the ADP kernels, else the plain ones

so the 30 cases below (N x reference mode x XB), each in both flavours and both calling patterns, launch each of the
5 x (12 + 12) = 120 plain and adaptive kernels once by construction; the GPU file asserts the family's name per solve.  (A
one-shot plain solve could take the refill kernel instead of <..., WS = false>: never at 87 instances, a batch that is no
multiple of 64 and far below two rounds of resident workgroups.)

A case is a dict(N, refs, xb, setting, prob, x0, xref, uref, kw, adaptive, sens, tag).  Both calling patterns are two solves
per instance, the second from the plant's next state x1 = A x0 + B u0 with orc64's own u0 of the first solve (one x1 for both
oracles and the kernel):
    "oneshot"  two cold solves; the adapted (rho, Kinf, Pinf) persist (a cold start leaves the adaptive state alone:
               Solver::ensure_extension_buffers refills it only when adapt_dirty).  On the oracle: d, y, g, v, z zeroed with
               set_state between the solves.
    "kept"     two consecutive solves of one solver, nothing touched in between.
Oracle results are cached per (case, flavour, pattern) and handed out read-only."""
import numpy as np

import tinympc_julia_amd as t
from tests.util import cm, load_golden

HORIZONS = (10, 15, 20, 25, 30)
REFS = ("zero", "shared", "per_instance")
XB = (False, True)
PATTERNS = ("oneshot", "kept")
# one full workgroup (64 instances), one full tile of 16 and a ragged tile of 7: inactive instances inside a tile, inactive
# tiles inside a workgroup — where the reduce-scatter over an instance's four lanes and `P.adapt + b` could read past the batch
B = 87
X_BOUND = 0.31          # rows 0-2, every knot: tests/test_gpu_parity.py::test_matrix_core_workspace_variant_vs_oracle's bound
TOL = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=40, check_termination=1)
# 25 iterations: the loop index passes 5, 10, 15, 20 (admm.cpp:147 adapts on i > 0, i % 5 == 0 before the index is bumped)
FIXED = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=25, check_termination=1)
DEFAULT_ADAPTIVE = dict(rho_min=0.1, rho_max=10.0, clip=True)
TIGHT_ADAPTIVE = dict(rho_min=1.0, rho_max=6.0, clip=True)
NOCLIP_ADAPTIVE = dict(rho_min=0.1, rho_max=10.0, clip=False)
# per horizon: the (reference mode, XB) cell that runs unclipped, and the one clamped to [1, 6] (chosen on the oracle so that
# the clamp binds: tests/test_mfma_variants_inputs.py asserts it per case)
NOCLIP = {10: ("zero", True), 15: ("shared", False), 20: ("per_instance", True), 25: ("zero", False), 30: ("shared", True)}
TIGHT = {10: ("per_instance", False), 15: ("zero", True), 20: ("zero", False), 25: ("zero", True), 30: ("per_instance", False)}
# the two cases that run with the non-symmetric dPinf/drho of tests/golden/L3_live_reference_adaptive_refs_bounds.json: the
# only input that tells Pinf' x from Pinf x in the terminal norm rows and in the reference term
NONSYMMETRIC = [(15, "shared", False), (10, "per_instance", True)]
SEED = {N: 4 for N in HORIZONS}
# seed of a case's reference draw: 9000 + 10 N + index of the mode, but for (25, shared) — with that draw (9251) the batch's
# residuals sit on the tolerance for many iterations and orc32 takes orc64's exits on 0.897 of the instances only in the
# adaptive one-shot pair (the condition of tests/test_mfma_variants_inputs.py is 0.9); with draw 2: 1.0
REF_SEED = {(25, "shared"): 2}


def case_id(c):
    return f"N{c[0]}_{c[1]}_xb{int(c[2])}"


CASES = [(N, refs, xb) for N in HORIZONS for refs in REFS for xb in XB]


def setting_of(N, refs, xb):
    """tolerance-terminated or fixed, alternating over the table so that every horizon and every reference mode sees both"""
    return "tol" if (HORIZONS.index(N) + REFS.index(refs) + int(xb)) % 2 == 0 else "fixed"


def tables(nonsymmetric=False):
    """(dKinf/drho, dPinf/drho): the compiled reference's built-in quadrotor tables as G9a stores them; the non-symmetric
    dPinf/drho as L3 stores it"""
    g = load_golden("G9a_quadrotor_adaptive_fixed100")
    dK, dP = cm(g["dKinf_drho"], 4, 12), cm(g["dPinf_drho"], 12, 12)
    if nonsymmetric:
        run = [r for r in load_golden("L3_live_reference_adaptive_refs_bounds")["runs"] if r["label"].endswith("nonsymmetric")][0]
        dP = cm(run["dPinf_drho"], 12, 12)
    return dK, dP


_cases = {}


def case(N, refs, xb):
    key = (N, refs, xb)
    if key in _cases:
        return _cases[key]
    prob = t.problems.quadrotor(N)
    x0 = t.problems.quadrotor_x0(B, seed=SEED[N])
    prob.x_min, prob.x_max = np.full((12, N), -1e17), np.full((12, N), 1e17)
    if xb:
        prob.x_min[:3, :], prob.x_max[:3, :] = -X_BOUND, X_BOUND
    rng = np.random.default_rng(REF_SEED.get((N, refs), 9000 + 10 * N + REFS.index(refs)))
    xref = uref = None
    if refs == "shared":
        xref, uref = 0.05 * rng.standard_normal((12, N)), 0.02 * rng.standard_normal((4, N - 1))
    elif refs == "per_instance":
        xref, uref = 0.05 * rng.standard_normal((12, N, B)), 0.02 * rng.standard_normal((4, N - 1, B))
    if xref is not None:
        xref, uref = np.asfortranarray(xref), np.asfortranarray(uref)
    setting = setting_of(N, refs, xb)
    adaptive = NOCLIP_ADAPTIVE if NOCLIP[N] == (refs, xb) else (TIGHT_ADAPTIVE if TIGHT[N] == (refs, xb) else DEFAULT_ADAPTIVE)
    c = dict(N=N, refs=refs, xb=xb, setting=setting, prob=prob, x0=x0, xref=xref, uref=uref,
             kw=dict(TOL if setting == "tol" else FIXED), adaptive=adaptive, sens=tables(key in NONSYMMETRIC),
             nonsymmetric=key in NONSYMMETRIC, tag=case_id(key))
    _cases[key] = c
    return c


def make_solver(c, kind, b, adaptive):
    """a cold, fully configured CpuSolver of instance b"""
    from oracle import cpu_oracle
    prob, xref, uref = c["prob"], c["xref"], c["uref"]
    o = cpu_oracle.CpuSolver(kind, prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
    o.update_settings(**c["kw"])
    o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if xref is not None:
        o.set_x_ref(xref if xref.ndim == 2 else xref[:, :, b])
        o.set_u_ref(uref if uref.ndim == 2 else uref[:, :, b])
    if adaptive:
        a = c["adaptive"]
        o.set_sensitivity(*c["sens"])
        o.set_adaptive_rho(1, a["rho_min"], a["rho_max"], a["clip"])
    return o


STATE = ("d", "y", "g", "v", "z")


def run_sequence(c, kind, b, adaptive, pattern, x1=None, forced=(0, 0)):
    """the two solves of instance b on a fresh oracle.  x1: the second solve's initial state (None: A x0 + B u0 of this run).
    forced: per solve, CpuSolver.set_forced_exit's argument (0: the oracle's own decision).  Returns the two solves' dicts:
    get_solution() + get_adapted() + the workspace after the solve (d, y, g, v, z) + x0."""
    prob = c["prob"]
    o = make_solver(c, kind, b, adaptive)
    x, out = c["x0"][:, b], []
    for k in range(2):
        o.set_x0(x)
        o.set_forced_exit(forced[k])
        o.solve()
        r = o.get_solution()
        r.update(o.get_adapted())
        r.update(o.get_state())
        r["x0"] = np.array(x)
        out.append(r)
        if k == 0:
            x = prob.A @ x + prob.B @ r["u"][:, 0] if x1 is None else x1
            if pattern == "oneshot":
                o.set_state(*[np.zeros_like(r[key]) for key in STATE])
    o.close()
    return out


def _stack(seqs, k):
    """solve k of every instance's sequence as batch arrays (instance axis last)"""
    keys = ("x", "u", "res", "Kinf", "Pinf", "x0") + STATE
    out = {key: np.stack([s[k][key] for s in seqs], axis=-1) for key in keys}
    out["res"] = np.ascontiguousarray(out["res"].T)                      # (B, 4) like get_status()'s
    for key in ("iter", "solved"):
        out[key] = np.array([s[k][key] for s in seqs], dtype=np.int32)
    out["rho"] = np.array([s[k]["rho"] for s in seqs])
    for a in out.values():
        a.setflags(write=False)
    return out


_pairs = {}


def oracle_pair(c, adaptive, pattern):
    """(x1 (12, B), orc64's two solves, orc32's two solves), each solve a dict of batch arrays; computed once"""
    key = (c["tag"], bool(adaptive), pattern)
    if key not in _pairs:
        s64 = [run_sequence(c, "orc64", b, adaptive, pattern) for b in range(B)]
        x1 = np.asfortranarray(np.stack([s[1]["x0"] for s in s64], axis=-1))
        x1.setflags(write=False)
        s32 = [run_sequence(c, "orc32", b, adaptive, pattern, x1=x1[:, b]) for b in range(B)]
        _pairs[key] = (x1, [_stack(s64, 0), _stack(s64, 1)], [_stack(s32, 0), _stack(s32, 1)])
    return _pairs[key]
