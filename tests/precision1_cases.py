"""Inputs of the precision-1 parity tests: one place, used by the CPU-only conditions (tests/test_precision1_inputs.py, the two
oracles alone) and by the GPU comparison (tests/test_precision1_gpu.py), so that what the conditions establish is what the
kernels are run on.

A case is a dict(prob, x0, xref, uref, kw, tag): the family with its bounds, the batch's initial states, references (None, shared
2-D or per-instance 3-D) and the solver settings.  Oracle results are cached per case and handed out read-only."""
import os

import numpy as np

import tinympc_julia_amd as t
from tests.util import precision1_limit

# find_quad_kernel's table (csrc/kernels.hip): (nx, nu, N, lanes per instance)
QUAD_ENTRIES = [(4, 1, 20, 4), (4, 1, 20, 2), (4, 1, 20, 1), (4, 1, 10, 4), (4, 1, 10, 2), (4, 1, 10, 1),
                (4, 1, 5, 4), (4, 1, 5, 1), (4, 1, 15, 4), (4, 1, 15, 1), (4, 1, 30, 4), (4, 1, 30, 1), (4, 1, 2, 4),
                (12, 4, 30, 4), (12, 4, 20, 4), (6, 3, 10, 4), (6, 3, 10, 2), (6, 3, 50, 4)]
# one workgroup (256 / G instances) plus a ragged tail: two workgroups, a part-filled last wavefront and quad row
BATCH = {4: 70, 2: 131, 1: 259}
# entries whose kernel has the run-time loop forms (LOOPV: plain, UNI, OS)
LOOPV = [(4, 1, 20, 1), (4, 1, 10, 1), (4, 1, 5, 1), (4, 1, 15, 1), (4, 1, 30, 1), (6, 3, 50, 4)]
# part b (continued solve from a kept workspace), part c (fused closed loop)
CONTINUED = [(4, 1, 20, 4), (4, 1, 20, 1), (12, 4, 20, 4), (6, 3, 10, 2)]
CLOSED_LOOP = [(4, 1, 20, 4), (4, 1, 10, 2)]
LOOP_STEPS = 5
XB = (False, True)
REFS = ("zero", "shared", "per_instance")
SETTINGS = ("fixed", "tol")
# the rocket's input box as a share of the unconstrained solve's max |u|, and its tolerance by horizon: chosen on the CPU
# oracles so that the box binds and both exits occur within max_iter = 60 (its initial states spread by 5 % only, so the
# instances of a case stop within a few iterations of each other: N = 10 mixes exits with references, N = 50 without).
# tests/test_precision1_inputs.py asserts both conditions
ROCKET_U_SHARE = 0.3
ROCKET_TOL = {10: 5e-4, 50: 8e-3}

NTHREADS = max(1, min(16, len(os.sched_getaffinity(0))))


def entry_id(e):
    return f"{e[0]}_{e[1]}_{e[2]}_g{e[3]}"


def family(nx, N):
    """(problem with the input box only, x0 generator) of a shape's family"""
    if nx == 4:
        return t.problems.cartpole(N, u_bound=0.5), t.problems.cartpole_x0
    if nx == 12:
        return t.problems.quadrotor(N), t.problems.quadrotor_x0
    p = t.problems.rocket(N)
    return p, t.problems.rocket_x0


def settings(nx, N, setting, max_iter=None):
    if setting == "fixed":
        return dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=max_iter or 40, check_termination=1)
    tol = ROCKET_TOL[N] if nx == 6 else 1e-3
    return dict(abs_pri_tol=tol, abs_dua_tol=tol, max_iter=max_iter or 60, check_termination=1)


def references(nx, nu, N, B, mode, seed):
    """the family's own references (rocket: rocket_refs; else zero) plus seeded noise, 0.1 on x and 0.05 on u"""
    if mode == "zero":
        return None, None
    rng = np.random.default_rng(seed)
    xr0, ur0 = t.problems.rocket_refs(N) if nx == 6 else (np.zeros((nx, N)), np.zeros((nu, N - 1)))
    if mode == "shared":
        return (np.asfortranarray(xr0 + 0.1 * rng.standard_normal((nx, N))),
                np.asfortranarray(ur0 + 0.05 * rng.standard_normal((nu, N - 1))))
    return (np.asfortranarray(xr0[:, :, None] + 0.1 * rng.standard_normal((nx, N, B))),
            np.asfortranarray(ur0[:, :, None] + 0.05 * rng.standard_normal((nu, N - 1, B))))


def state_bounds(prob, x0, on):
    """off: +-1e17 everywhere.  on: rows 0 .. nx/2 - 1 at +-0.8 max_b |x0[row, b]|, the upper bound 10 % higher from knot N/2 on
    (per-knot bounds; for nx = 12 the six rows span two lane roles of the four-lanes-per-instance kernel)"""
    nx, N = prob.nx, prob.N
    prob.x_min, prob.x_max = np.full((nx, N), -1e17), np.full((nx, N), 1e17)
    if on:
        lim = 0.8 * np.abs(x0).max(axis=1)
        for r in range(nx // 2):
            prob.x_min[r, :], prob.x_max[r, :] = -lim[r], lim[r]
            prob.x_max[r, N // 2:] = 1.1 * lim[r]


_cases = {}


def quad_case(nx, nu, N, B, xb, refs, setting, max_iter=None):
    key = (nx, nu, N, B, xb, refs, setting, max_iter)
    if key in _cases:
        return _cases[key]
    prob, gen = family(nx, N)
    x0 = gen(B, seed=100 + N)
    xref, uref = references(nx, nu, N, B, refs, seed=7000 + 10 * N + REFS.index(refs))
    state_bounds(prob, x0, xb)
    kw = settings(nx, N, setting, max_iter)
    if nx == 6:
        # the rocket's own box (-10 .. 105) never binds on these inputs: a box at a share of what the solve without any
        # bound asks for, around the input reference's level (uref[2] = 10 for the tracking modes)
        from oracle import cpu_oracle
        free = t.problems.rocket(N)
        free.x_min, free.x_max = np.full((6, N), -1e17), np.full((6, N), 1e17)
        free.u_min, free.u_max = np.full((3, N - 1), -1e17), np.full((3, N - 1), 1e17)
        r = cpu_oracle.solve_batch("orc64", free, x0, xref=xref, uref=uref, nthreads=NTHREADS, **settings(6, N, "fixed"))
        lim = ROCKET_U_SHARE * np.abs(r["u"]).max()
        prob.u_min, prob.u_max = np.full((3, N - 1), -lim), np.full((3, N - 1), lim)
    case = dict(prob=prob, x0=x0, xref=xref, uref=uref, kw=kw,
                tag=f"({nx},{nu},{N}) B={B} xb={int(xb)} refs={refs} {setting}")
    _cases[key] = case
    return case


_oracles = {}


def _freeze(r):
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def oracle_pair(case):
    """(orc64 result, orc32 result, limit_case, e32_case, agreement share) of a box-constrained case, computed once"""
    from oracle import cpu_oracle
    key = case["tag"]
    if key not in _oracles:
        kw = dict(xref=case["xref"], uref=case["uref"], nthreads=NTHREADS, **case["kw"])
        r64 = _freeze(cpu_oracle.solve_batch("orc64", case["prob"], case["x0"], **kw))
        r32 = _freeze(cpu_oracle.solve_batch("orc32", case["prob"], case["x0"], **kw))
        limit, e32, same = precision1_limit(r32, r64)
        _oracles[key] = (r64, r32, limit, e32, same)
    return _oracles[key]


def make_oracle(case, kind="orc64"):
    """factory of cold, configured CpuSolvers of a box-constrained case (shared references applied here)"""
    from oracle import cpu_oracle
    prob, xref, uref = case["prob"], case["xref"], case["uref"]

    def make(b=None):
        o = cpu_oracle.CpuSolver(kind, prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
        o.update_settings(**case["kw"])
        o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        if xref is not None and np.ndim(xref) == 2:
            o.set_x_ref(xref)
            o.set_u_ref(uref)
        return o
    return make


def state_bound_share(case, r64):
    """share of the instances with a state at (or past) a finite bound at some knot after the first in orc64's solution: the
    projection of the state slack is active there.  Knot 0 is x0 itself and does not count."""
    prob = case["prob"]
    scale = np.abs(r64["x"]).max(axis=(1, 2), keepdims=True)
    x = r64["x"][:, 1:, :]
    hit = (x >= prob.x_max[:, 1:, None] - 1e-9 * scale) | (x <= prob.x_min[:, 1:, None] + 1e-9 * scale)
    return float(hit.any(axis=(0, 1)).mean())


def input_bound_share(case, r64):
    prob = case["prob"]
    scale = np.abs(r64["u"]).max()
    u = r64["u"]
    hit = (u >= prob.u_max[:, :, None] - 1e-9 * scale) | (u <= prob.u_min[:, :, None] + 1e-9 * scale)
    return float(hit.any(axis=(0, 1)).mean())


# ---- the stream and generic kernels' cases (part d): configurations the oracle takes one solver per instance for ----
ROCKET_CONES = ([0], [3], [0.25], [0], [3], [0.5])


def _loop(make, x0, xref=None, uref=None):
    """every instance on its own CpuSolver: dict like solve_batch's"""
    nxs, B = x0.shape
    out = None
    for b in range(B):
        o = make(b)
        if xref is not None and np.ndim(xref) == 3:
            o.set_x_ref(xref[:, :, b])
            o.set_u_ref(uref[:, :, b])
        o.set_x0(x0[:, b])
        o.solve()
        r = o.get_solution()
        if out is None:
            out = dict(x=np.zeros(r["x"].shape + (B,)), u=np.zeros(r["u"].shape + (B,)), iter=np.zeros(B, dtype=np.int32),
                       solved=np.zeros(B, dtype=np.int32), res=np.zeros((B, 4)))
        out["x"][:, :, b], out["u"][:, :, b] = r["x"], r["u"]
        out["iter"][b], out["solved"][b], out["res"][b] = r["iter"], r["solved"], r["res"]
        o.close()
    return out


def loop_pair(case):
    """oracle_pair for a case with its own solver factory case["make"](kind) (extensions, per-instance families)"""
    key = case["tag"]
    if key not in _oracles:
        r64 = _freeze(_loop(case["make"]("orc64"), case["x0"], case["xref"], case["uref"]))
        r32 = _freeze(_loop(case["make"]("orc32"), case["x0"], case["xref"], case["uref"]))
        limit, e32, same = precision1_limit(r32, r64)
        _oracles[key] = (r64, r32, limit, e32, same)
    return _oracles[key]


def _random_family(nx, nu, N, seed):
    rng = np.random.default_rng(seed)
    A = np.eye(nx) + 0.1 * rng.standard_normal((nx, nx))
    Bm = rng.standard_normal((nx, nu))
    qd = np.array([5.0, 2.0, 1.0, 3.0, 0.5])[:nx]
    prob = t.problems.Problem("rand", A, Bm, np.diag(qd), np.diag([1.0, 2.0][:nu]), 2.0, N)
    prob.x_min, prob.x_max = np.full((nx, N), -2.0), np.full((nx, N), 2.0)
    prob.u_min, prob.u_max = np.full((nu, N - 1), -0.3), np.full((nu, N - 1), 0.3)
    return prob, rng


STREAM_B = 70


def random_case(nx, nu, N):
    """a random family outside the built-in shapes: (3,2) on the stream kernel at the shortest horizon it is asked for here,
    (5,2) on the generic kernel"""
    key = ("rand", nx, nu, N)
    if key not in _cases:
        prob, rng = _random_family(nx, nu, N, seed=300 + 10 * nx + nu)
        x0 = np.asfortranarray(rng.uniform(-1, 1, (nx, STREAM_B)))
        _cases[key] = dict(prob=prob, x0=x0, xref=None, uref=None, kw=settings(nx, N, "tol"),
                           tag=f"random ({nx},{nu},{N}) B={STREAM_B}")
    return _cases[key]


def rocket_cone_case(N=12):
    """the affine term and one cone per side: tests/test_gpu_parity.py::test_rocket_fdyn_cones_vs_oracle's configuration"""
    from oracle import cpu_oracle
    key = ("rocket_cones", N)
    if key not in _cases:
        prob = t.problems.rocket(N)
        x0 = t.problems.rocket_x0(STREAM_B, seed=2)
        xr, ur = t.problems.rocket_refs(N)
        kw = dict(abs_pri_tol=2e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1)

        def make(kind):
            def mk(b=None):
                o = cpu_oracle.CpuSolver(kind, prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
                o.update_settings(**kw)
                o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
                o.set_fdyn(prob.fdyn)
                o.set_cone_constraints(*ROCKET_CONES)
                o.set_x_ref(xr)
                o.set_u_ref(ur)
                return o
            return mk
        _cases[key] = dict(prob=prob, x0=x0, xref=xr, uref=ur, kw=kw, make=make, tag=f"rocket fdyn + cones N={N}")
    return _cases[key]


def linear_rows_case(N=9):
    """linear rows on the cartpole: tests/test_gpu_parity.py::test_linear_constraints_vs_oracle's configuration (the input box
    at 5 is out of reach on purpose: the rows |u| <= 0.8 are what binds)"""
    from oracle import cpu_oracle
    key = ("lin", N)
    if key not in _cases:
        prob = t.problems.cartpole(N, u_bound=5.0)
        x0 = t.problems.cartpole_x0(STREAM_B, seed=6)
        lin = (np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0]]), np.array([0.6, 0.12]), np.array([[1.0], [-1.0]]),
               np.array([0.8, 0.8]))
        kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=120, check_termination=1)

        def make(kind):
            def mk(b=None):
                o = cpu_oracle.CpuSolver(kind, prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
                o.update_settings(**kw)
                o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
                o.set_linear_constraints(*lin)
                return o
            return mk
        _cases[key] = dict(prob=prob, x0=x0, xref=None, uref=None, kw=kw, make=make, lin=lin, tag=f"cartpole linear rows N={N}")
    return _cases[key]


def families_case(N=17):
    """one family per instance, perturbed cartpoles: tests/test_gpu_parity.py::test_per_instance_families_vs_oracle's draw"""
    from oracle import cpu_oracle
    key = ("het", N)
    if key not in _cases:
        rng = np.random.default_rng(41)
        B = STREAM_B
        base = t.problems.cartpole(N, u_bound=0.5)
        A = np.repeat(base.A[:, :, None], B, axis=2) * (1.0 + 0.02 * rng.standard_normal((4, 4, B)))
        Bm = np.repeat(base.B[:, :, None], B, axis=2) * (1.0 + 0.05 * rng.standard_normal((4, 1, B)))
        Q, R = np.zeros((4, 4, B)), np.zeros((1, 1, B))
        for b in range(B):
            Q[:, :, b] = np.diag(np.array([10.0, 1.0, 10.0, 1.0]) * rng.uniform(0.5, 2.0, 4))
            R[:, :, b] = rng.uniform(0.5, 2.0)
        rho = rng.uniform(0.5, 3.0, B)
        x0 = t.problems.cartpole_x0(B, seed=5)
        kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1)

        def make(kind):
            def mk(b):
                o = cpu_oracle.CpuSolver(kind, A[:, :, b], Bm[:, :, b], Q[:, :, b], R[:, :, b], float(rho[b]), N)
                o.update_settings(**kw)
                o.set_bound_constraints(base.x_min, base.x_max, base.u_min, base.u_max)
                return o
            return mk
        _cases[key] = dict(prob=base, x0=x0, xref=None, uref=None, kw=kw, make=make, fam=(A, Bm, Q, R, rho),
                           tag=f"per-instance cartpole families N={N}")
    return _cases[key]


# ---- continued solves and closed loops (parts b, c): persistent oracles, one per instance ----
def continued_pair(case):
    """two solves of persistent per-instance oracles: x0, then A x0 + B u0 with orc64's u0 (the same second state for both
    oracles and for the kernel), no reset in between.  Returns (x1 (nx, B), orc64's second result, limit, e32, share)."""
    key = ("continued", case["tag"])
    if key not in _oracles:
        prob, x0 = case["prob"], case["x0"]
        B = x0.shape[1]
        r64 = _loop(make_oracle(case, "orc64"), x0, case["xref"], case["uref"])          # (cold: only u0 is needed here)
        x1 = np.asfortranarray(prob.A @ x0 + prob.B @ r64["u"][:, 0, :])
        out = {}
        for kind in ("orc64", "orc32"):
            res = None
            mk = make_oracle(case, kind)
            for b in range(B):
                o = mk(b)
                for x in (x0, x1):
                    o.set_x0(x[:, b])
                    o.solve()
                r = o.get_solution()
                if res is None:
                    res = dict(x=np.zeros(r["x"].shape + (B,)), u=np.zeros(r["u"].shape + (B,)),
                               iter=np.zeros(B, dtype=np.int32), solved=np.zeros(B, dtype=np.int32), res=np.zeros((B, 4)))
                res["x"][:, :, b], res["u"][:, :, b] = r["x"], r["u"]
                res["iter"][b], res["solved"][b], res["res"][b] = r["iter"], r["solved"], r["res"]
                o.close()
            out[kind] = _freeze(res)
        limit, e32, same = precision1_limit(out["orc32"], out["orc64"])
        _oracles[key] = (x1, out["orc64"], limit, e32, same)
    return _oracles[key]


def closed_loop_pair(case, steps):
    """the host-stepped closed loop (cartpole_example_mpc.jl:35-51; the plant is the family's own A, B) on persistent oracles:
    applied controls (nu, steps, B) and plant states (nx, steps, B) of orc64, and the bar from orc32's loop"""
    key = ("loop", case["tag"], steps)
    if key not in _oracles:
        prob, x0 = case["prob"], case["x0"]
        B = x0.shape[1]
        out = {}
        for kind in ("orc64", "orc32"):
            mk = make_oracle(case, kind)
            U, X = np.zeros((prob.nu, steps, B)), np.zeros((prob.nx, steps, B))
            for b in range(B):
                o = mk(b)
                x = x0[:, b].copy()
                for k in range(steps):
                    o.set_x0(x)
                    o.solve()
                    u = o.get_solution()["u"][:, 0]
                    x = prob.A @ x + prob.B @ u
                    U[:, k, b], X[:, k, b] = u, x
                o.close()
            it = np.zeros(B, dtype=np.int32)
            out[kind] = _freeze(dict(x=X, u=U, iter=it, solved=it))
        limit, e32, same = precision1_limit(out["orc32"], out["orc64"])
        _oracles[key] = (out["orc64"], limit, e32, same)
    return _oracles[key]


# part d: name -> case builder.  Box-only cases carry the quad recipe's inputs (state bounds on, tolerance-terminated) at
# horizons without a lanes-per-instance kernel
STREAM_CASES = {f"{fam}{N}_{refs}": (lambda nx=nx, nu=nu, N=N, refs=refs: quad_case(nx, nu, N, STREAM_B, True, refs, "tol"))
                for fam, nx, nu, N in (("cartpole", 4, 1, 17), ("quadrotor", 12, 4, 7)) for refs in REFS}
STREAM_CASES.update(rocket_cones12=rocket_cone_case, linear9=linear_rows_case, families17=families_case,
                    random_3_2_3=lambda: random_case(3, 2, 3), random_5_2_9=lambda: random_case(5, 2, 9))


# ---- adaptive rho (part e): the oracle side of tests/test_gpu_parity.py::test_adaptive_rho_through_dropin_api ----
ADAPTIVE = dict(rho_min=0.1, rho_max=10.0, clip=True)


def adaptive_case(N):
    """cartpole, tolerance-terminated (both exits), rho adapted every fifth iteration within [0.1, 10]; the sensitivities are
    the library's own host finite differences (what the solver computes on first use), handed to both oracles"""
    from oracle import cpu_oracle
    key = ("adaptive", N)
    if key not in _cases:
        prob = t.problems.cartpole(N, u_bound=0.5)
        x0 = t.problems.cartpole_x0(STREAM_B, seed=100 + N)
        kw = settings(4, N, "tol")
        dK, dP, _, _ = t.host_sensitivity(prob.A, prob.B, prob.Q, prob.R, prob.rho)

        def make(kind):
            def mk(b=None):
                o = cpu_oracle.CpuSolver(kind, prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
                o.update_settings(**kw)
                o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
                o.set_sensitivity(dK, dP)
                o.set_adaptive_rho(1, ADAPTIVE["rho_min"], ADAPTIVE["rho_max"], ADAPTIVE["clip"])
                return o
            return mk
        _cases[key] = dict(prob=prob, x0=x0, xref=None, uref=None, kw=kw, make=make, sens=(dK, dP),
                           tag=f"cartpole adaptive rho N={N}")
    return _cases[key]


def adaptive_pair(case):
    """(orc64 result with its adapted rho (B,), limit_case, e32_case, agreement share, rho limit).  The rho limit is the same
    rule on the adapted rho: max(1e-5 — the bar of the fp64-recurrence kernels' adaptive tests —, 4 x orc32's worst relative
    distance from orc64's rho)"""
    key = case["tag"]
    if key not in _oracles:
        x0 = case["x0"]
        B = x0.shape[1]
        out = {}
        for kind in ("orc64", "orc32"):
            res, rho = None, np.zeros(B)
            mk = case["make"](kind)
            for b in range(B):
                o = mk(b)
                o.set_x0(x0[:, b])
                o.solve()
                r = o.get_solution()
                if res is None:
                    res = dict(x=np.zeros(r["x"].shape + (B,)), u=np.zeros(r["u"].shape + (B,)),
                               iter=np.zeros(B, dtype=np.int32), solved=np.zeros(B, dtype=np.int32), res=np.zeros((B, 4)))
                res["x"][:, :, b], res["u"][:, :, b] = r["x"], r["u"]
                res["iter"][b], res["solved"][b], res["res"][b] = r["iter"], r["solved"], r["res"]
                rho[b] = o.get_adapted()["rho"]
                o.close()
            res["rho"] = rho
            out[kind] = _freeze(res)
        limit, e32, same = precision1_limit(out["orc32"], out["orc64"])
        agree = (out["orc32"]["iter"] == out["orc64"]["iter"]) & (out["orc32"]["solved"] == out["orc64"]["solved"])
        drho = float((np.abs(out["orc32"]["rho"] - out["orc64"]["rho"]) / out["orc64"]["rho"])[agree].max())
        _oracles[key] = (out["orc64"], limit, e32, same, max(1e-5, 4.0 * drho), drho)
    return _oracles[key]
