"""Inputs of the "every form of every shape" tests of the two run-time-shape kernels: one place, used by the CPU-only conditions
(tests/test_stream_forms_inputs.py, the two oracles alone) and by the GPU comparison (tests/test_stream_forms_gpu.py), so that
what the conditions establish is what the kernels are run on.  Drawn once with fixed seeds; oracle results are cached per
session and handed out read-only.

A case (one per shape) is the model of test_gpu_parity._random_problem(bounded=True) with per-knot state bounds (the upper ones
tighter from knot N / 2 on, so that states reach them), 70 initial states inside the state box and the state cone, shared
non-zero references, an affine term, one cone per side placed across the lane boundary, linear rows built by
the recipe of tests/test_instance_rows_gpu.py::_rows from the oracle's own trajectory, 70 families around the model
(families_cases.perturbed) and the library's host sensitivities.  An ARM picks what of that a solve uses:

  plain     box sets, shared references                                   ext1     + affine term, cones (no references)
  ext2      ext1 + 2 state rows, 2 input rows                             het      one family per instance, box sets, references
  het_ext2  het + ext2's affine term, cones and rows (no references)      adp      plain + adaptive rho
and for the generic kernel also  ib (per-instance bounds), il (per-instance rows), adp_ext (adaptive rho, affine term, a cone).

arm(case, name) -> dict(tag, make(kind) -> mk(b) -> cold configured CpuSolver, xref, uref, rho: the largest rho an instance can
hold — the band of parity_every_instance —, adaptive: bool)."""
import numpy as np

import tinympc_julia_amd as t
from tests import precision1_cases as pc
from tests.families_cases import perturbed
from tests.util import precision1_limit

B = 70                                    # two stream workgroups of 64 instances, the second ragged with 6
GRID = [(nx, nu) for nx in (2, 3, 4, 6, 8, 10, 12) for nu in (1, 2, 3, 4) if nu <= nx]
KW = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=50, check_termination=1)
ADAPTIVE = pc.ADAPTIVE
MU_X, MU_U = 1.5, 0.8                     # cone slopes: |head| <= mu * axis, the axis being the block's last row
# the initial states fill this share of the state box of knot 0, row by row: every x0 is feasible (an instance whose x0 is not
# never converges: knot 0 of the slack is the projection of x0) and a fifth of the batch and more runs into a bound later
X0_FILL = 0.98
X_TIGHTER = 0.5                           # the upper state bounds from knot N / 2 on, as a share of the earlier knots'
X_TIGHTER_ROWS = 12                       # ... of the first 12 rows (with 64 rows tightened, no instance converges in 50 iterations)
# as many inputs as states, or one fewer of four: the controller holds every state off a bound at 0.5 (no seed of 80 met the
# state condition on every arm), so these shapes' bounds tighten further
X_TIGHTER_SHAPE = {(2, 2): 0.3, (3, 3): 0.3, (4, 3): 0.3, (4, 4): 0.15}
STREAM_ARMS = ("plain", "ext1", "ext2", "het", "het_ext2", "adp")
FLOAT_ARMS = ("plain", "ext2", "het_ext2", "adp")          # the arms run again at precision 1
# One seed per shape: the first of 100 nx + nu (+ 7 for the generic cases) + 1000 k, k = 0, 1, .., at which the oracles meet every
# input condition (conditions() below) on every arm of the shape.
SEEDS = {(2, 1): 2201, (2, 2): 13202, (3, 1): 2301, (3, 2): 45302, (3, 3): 9303, (4, 1): 401, (4, 2): 2402, (4, 3): 403,
         (4, 4): 1404, (6, 1): 601, (6, 2): 3602, (6, 3): 603, (6, 4): 13604, (8, 1): 801, (8, 2): 802, (8, 3): 803, (8, 4): 4804,
         (10, 1): 2001, (10, 2): 13002, (10, 3): 2003, (10, 4): 2004, (12, 1): 1201, (12, 2): 5202, (12, 3): 1203, (12, 4): 2204}
GENERIC_SEEDS = {(1, 1, 4): 4108, (5, 5, 4): 3512, (13, 1, 4): 2308, (16, 5, 4): 1612, (64, 1, 4): 7408, (33, 32, 4): 5339,
                 (64, 32, 4): 27439, (5, 2, 2): 1509, (4, 1, 2): 37408}


def shape_id(s):
    return "_".join(str(v) for v in s)


def horizon(nx, nu):
    """5 .. 9, another one for the next shape of the grid; (4,1) -> 6, off the built-in on-chip horizons of every shape"""
    return 5 + (GRID.index((nx, nu)) + 1) % 5


def _grid(a):
    """coefficients on a grid of 2^-10 (tests/test_instance_rows_gpu.py::_grid): fp32 values whose squares are fp32 values too"""
    return np.round(np.asarray(a) * 1024.0) / 1024.0


def cone_layout(nx, nu):
    """((input starts, dims, mus), (state starts, dims, mus)): one cone per side whose rows cover RX - 1 and RX (inputs RU - 1 and
    RU) of the four-lane row deal RX = ceil(nx / 4), RU = ceil(nu / 4), three rows where the side has three; no input cone for
    one input"""
    rx = (nx + 3) // 4
    cx = ([rx - 1], [3 if nx >= 3 else 2], [MU_X]) if nx >= 2 else ([], [], [])
    cu = ([0], [min(3, nu)], [MU_U]) if nu >= 2 else ([], [], [])
    return cu, cx


_cases, _oracles, _rows_cache = {}, {}, {}


def _f32(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float32).astype(np.float64))


def make_case(nx, nu, N, seed, tag, f32=False):
    from tests.test_gpu_parity import _random_problem
    rng = np.random.default_rng(seed)
    prob = _random_problem(rng, nx, nu, N, bounded=True)
    if nu > 4:    # (the generic cases) with three constraint sets on the inputs — box, cone, rows — the iteration carries three slacks
        prob.R = prob.R * 10.0            # on a cache built for one rho and does not settle at 32 inputs unless R outweighs rho: orc64's
                                          # own residuals stay at 0.3 .. 6 after 50 iterations, and orc32 drifts 1e-4 off it
    if f32:       # diag(Q) + rho and diag(R) + rho reach the device as fp32 values: on a grid of 2^-12 the sums are exact there
        prob.Q, prob.R, prob.rho = np.round(prob.Q * 4096.0) / 4096.0, np.round(prob.R * 4096.0) / 4096.0, round(prob.rho * 4096.0) / 4096.0
    prob.x_max[:X_TIGHTER_ROWS, N // 2:] *= X_TIGHTER_SHAPE.get((nx, nu), X_TIGHTER)
    mid, half = 0.5 * (prob.x_max[:, :1] + prob.x_min[:, :1]), 0.5 * (prob.x_max[:, :1] - prob.x_min[:, :1])
    x0 = np.asfortranarray(mid + X0_FILL * half * rng.uniform(-1.0, 1.0, (nx, B)))
    cx = cone_layout(nx, nu)[1]
    if len(cx[0]):   # ... and inside the state cone: an x0 outside it leaves knot 0 of the cone set unmeetable, its dual grows with
        s0, d = cx[0][0], cx[1][0]        # every iteration and the fp32 loop drifts off the fp64 one (1e-4 .. 1e-3 at 33 and 64 states)
        ax = s0 + d - 1
        x0[ax] = np.clip(np.abs(x0[ax]), 0.1 * prob.x_max[ax, 0], None)
        head = np.sqrt((x0[s0:ax] ** 2).sum(axis=0))
        x0[s0:ax] *= np.minimum(1.0, 0.9 * MU_X * x0[ax] / np.maximum(head, 1e-12))
        x0[ax] = np.minimum(x0[ax], X0_FILL * prob.x_max[ax, 0])
    xref = np.asfortranarray(0.2 * rng.standard_normal((nx, N)))
    uref = np.asfortranarray(0.1 * rng.standard_normal((nu, N - 1)))
    fdyn = 0.02 * rng.standard_normal(nx)
    if f32:       # what reaches the device as fp32 arrays holds fp32 values: the oracle of a precision-2 solve is fed the same numbers
        x0, xref, uref = _f32(x0), _f32(xref), _f32(uref)
        prob.x_min, prob.x_max, prob.u_min, prob.u_max = (_f32(m) for m in (prob.x_min, prob.x_max, prob.u_min, prob.u_max))
    fam = perturbed(prob, B, seed + 5000) if (nx, nu) in GRID else None
    return dict(nx=nx, nu=nu, N=N, prob=prob, x0=x0, xref=xref, uref=uref, fdyn=fdyn, cones=cone_layout(nx, nu), fam=fam,
                kw=dict(KW), tag=tag, seed=seed)


def stream_case(nx, nu):
    key = ("stream", nx, nu)
    if key not in _cases:
        _cases[key] = make_case(nx, nu, horizon(nx, nu), SEEDS.get((nx, nu), 100 * nx + nu), f"stream ({nx},{nu})")
    return _cases[key]


# ---- the generic kernel at the edges of its shape range: (nx, nu, N) ----
GENERIC_SHAPES = [(1, 1, 4), (5, 5, 4), (13, 1, 4), (16, 5, 4), (64, 1, 4), (33, 32, 4), (64, 32, 4), (5, 2, 2), (4, 1, 2)]
# the adaptive arms may be left out at the two nx = 64 shapes if their host-side setup takes more than a few seconds there:
# t.host_sensitivity (finite differences over Riccati recursions) measured 2.1 s at (64,1) and 0.12 s at (64,32) on the CPU,
# so they stay
NO_ADAPTIVE = []


def generic_case(nx, nu, N):
    key = ("generic", nx, nu, N)
    if key not in _cases:
        c = make_case(nx, nu, N, GENERIC_SEEDS.get((nx, nu, N), 100 * nx + nu + 7), f"generic ({nx},{nu},{N})", f32=True)
        c["state_rows"] = 8 if (nx, nu) == (16, 5) else 2          # LIN_MAX_ROWS rows on the state side
        if nx == 64:      # a 64-state solve of 70 instances takes the generic kernel 7 ms an iteration: 25 keep the test at a few seconds
            c["kw"]["max_iter"] = 25
        _cases[key] = c
    return _cases[key]


def generic_arms(case):
    arms = ("plain", "ext2", "ib", "il", "adp", "adp_ext")
    return arms[:4] if (case["nx"], case["nu"], case["N"]) in NO_ADAPTIVE else arms


# ---- long horizons on the stream kernel: the LDS image of (12,4) around 48 KiB, 64 KiB and the 150 KiB routing limit ----
def stream_lds_bytes(nx, nu, N, rt=8):
    """streamg_lds_bytes<NX, NU, 4> (csrc/streamg_entry.hip.h) restated: rt * 4 * CP + 4 * (N * 4 * BW + 4 * DW), CP from
    QuadShape / StreamPackG's offsets"""
    pad8 = lambda n: (n + 7) // 8 * 8
    rx, ru = (nx + 3) // 4, (nu + 3) // 4
    nxp, nup = 4 * rx, 4 * ru
    fwd = pad8(rx * nxp + ru * nxp + rx * nup)
    bwd = pad8(rx * nxp + ru * nxp + rx * nup + ru * nup)
    cp_s = fwd + bwd + pad8(rx * nxp)
    cp = pad8(cp_s + 2 * rx + ru) + pad8(rx * nxp)
    return rt * 4 * cp + 4 * (N * 4 * (2 * rx + 2 * ru) + 4 * (rx + ru))


def long_horizons():
    """(12,4): the first horizon past 48 KiB of LDS (hipFuncSetAttribute is called from there on), the first past 64 KiB, the last
    under 150 KiB — all three solved on the stream kernel — and the first past 150 KiB, which goes to the generic kernel"""
    first = lambda lim: next(N for N in range(2, 5000) if stream_lds_bytes(12, 4, N) > lim)
    return dict(solved=[first(48 * 1024), first(64 * 1024), first(150 * 1024) - 1], generic=first(150 * 1024))


def long_case(N):
    from tests.test_gpu_parity import _random_problem
    key = ("long", N)
    if key not in _cases:
        rng = np.random.default_rng(12400 + N)
        prob = _random_problem(rng, 12, 4, N, bounded=False)
        x0 = np.asfortranarray(rng.uniform(-1.0, 1.0, (12, 5)))
        kw = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=10, check_termination=1)
        _cases[key] = dict(prob=prob, x0=x0, xref=None, uref=None, kw=kw, tag=f"long horizon (12,4,{N}) B=5")
    return _cases[key]


def long_pair(case):
    return pc.oracle_pair(case)


def sensitivity(case):
    if "sens" not in case:
        p = case["prob"]
        case["sens"] = t.host_sensitivity(p.A, p.B, p.Q, p.R, p.rho)[:2]
    return case["sens"]


def shared_rows(case, state_rows=2):
    """(Alin_x (state_rows, nx), blin_x, Alin_u (2, nu), blin_u), shared by the batch, from orc64's solutions of the ext1 arm (the
    free trajectories): state row 0 a unit direction in coordinates (0, 1) — (0) for one state —, the others the coordinates
    that move most, scaled in [0.5, 2]; each points where the batch's trajectories move away from x0 on average, b is the larger
    of the batch's largest a.x0 plus a margin (every x0 is feasible) and the batch's 0.8 quantile of the free maximum of a.x
    over the knots after the first; the input rows are single-coordinate rows (coordinates 0 and 1, each on the side the free
    inputs reach further; one input: both sides of it) scaled in [0.5, 2], b at 0.9 of the batch's 0.8 quantile of the free
    maximum on that side: the rows cut a tenth off the fifth of the batch that goes furthest"""
    key = (case["tag"], state_rows)
    if key in _rows_cache:
        return _rows_cache[key]
    free = arm_ref(case, "ext1")
    nx, nu = case["nx"], case["nu"]
    rng = np.random.default_rng(case["seed"] + 9000)
    X, U = free["x"], free["u"]
    order = np.argsort(-(X.max(axis=1) - X.min(axis=1)).mean(axis=1))
    Ax, bx = np.zeros((state_rows, nx)), np.zeros(state_rows)
    th = rng.uniform(0.0, 2.0 * np.pi)
    Ax[0, 0] = _grid(np.cos(th)) if nx > 1 else 1.0
    if nx > 1:
        Ax[0, 1] = _grid(np.sin(th))
    for k in range(1, state_rows):
        Ax[k, order[(k - 1) % nx]] = _grid(rng.uniform(0.5, 2.0))
    for k in range(state_rows):
        p = np.einsum("j,jkb->kb", Ax[k], X)
        if (p[1:].max(axis=0) - p[0]).mean() < (p[0] - p[1:].min(axis=0)).mean():
            Ax[k], p = -Ax[k], -p
        bx[k] = max(p[0].max() + 1e-3 * (1.0 + np.abs(p[0]).max()), np.quantile(p[1:].max(axis=0), 0.8))
    Au, bu = np.zeros((2, nu)), np.zeros(2)
    s = _grid(rng.uniform(0.5, 2.0, 2))
    scale = np.abs(U).max()
    for k in range(2):
        c = k if nu > 1 else 0
        reach = [np.quantile((sg * U[c]).max(axis=0), 0.8) for sg in (1.0, -1.0)]
        sg = (1.0 if reach[0] >= reach[1] else -1.0) if nu > 1 else (1.0 if k == 0 else -1.0)
        Au[k, c] = sg * s[k]
        bu[k] = 0.9 * s[k] * max(reach[0 if sg > 0 else 1], 0.05 * scale)
    out = tuple(np.array(a.astype(np.float32), dtype=np.float64) for a in (Ax, bx, Au, bu))
    _rows_cache[key] = out
    return out


def instance_bounds(case):
    """(x_min, x_max (nx, N, B), u_min, u_max (nu, N-1, B)): the case's per-knot bounds scaled per instance in [0.7, 1.3], fp32 values"""
    rng = np.random.default_rng(case["seed"] + 7000)
    p = case["prob"]
    sx, su = rng.uniform(0.7, 1.3, (case["nx"], 1, B)), rng.uniform(0.7, 1.3, (case["nu"], 1, B))
    return tuple(np.asfortranarray((m[:, :, None] * s).astype(np.float32).astype(np.float64))
                 for m, s in ((p.x_min, sx), (p.x_max, sx), (p.u_min, su), (p.u_max, su)))


def instance_rows(case):
    """the shared rows (from the ext1 arm's trajectories) with every instance's right-hand sides scaled in [0.8, 1.25] (state side: never
    below the instance's own a.x0 plus a margin), and every third instance without its second row on either side"""
    key = (case["tag"], "il")
    if key in _rows_cache:
        return _rows_cache[key]
    rng = np.random.default_rng(case["seed"] + 8000)
    Ax, bx, Au, bu = shared_rows(case)
    x0 = case["x0"]
    Axb, Aub = np.repeat(Ax[:, :, None], B, axis=2), np.repeat(Au[:, :, None], B, axis=2)
    bxb = bx[:, None] * rng.uniform(0.8, 1.25, (len(bx), B))
    bxb = np.maximum(bxb, Ax @ x0 + 1e-3 * (1.0 + np.abs(Ax @ x0)))
    bub = bu[:, None] * rng.uniform(0.8, 1.25, (len(bu), B))
    third = np.arange(B) % 3 == 2
    Axb[1:, :, third], bxb[1:, third], Aub[1:, :, third], bub[1:, third] = 0.0, 0.0, 0.0, 0.0
    out = tuple(np.asfortranarray(a.astype(np.float32).astype(np.float64)) for a in (Axb, bxb, Aub, bub))
    _rows_cache[key] = out
    return out


def arm(case, name):
    from oracle import cpu_oracle
    prob, kw = case["prob"], case["kw"]
    refs = name in ("plain", "het", "adp", "ib", "p2")
    het = name.startswith("het")
    ext = name in ("ext1", "ext2", "het_ext2", "adp_ext")
    rows = shared_rows(case, case.get("state_rows", 2)) if name in ("ext2", "het_ext2") else None
    adaptive = name.startswith("adp")
    sens = sensitivity(case) if adaptive else None
    ib = instance_bounds(case) if name == "ib" else None
    il = instance_rows(case) if name == "il" else None
    cu, cx = case["cones"]
    if name == "adp_ext":                       # the affine term and the state cone
        cu = ([], [], [])
    fam = case["fam"]

    def make(kind):
        def mk(b=None):
            m = tuple(a[..., b] for a in fam[:4]) + (float(fam[4][b]),) if het else (prob.A, prob.B, prob.Q, prob.R, prob.rho)
            o = cpu_oracle.CpuSolver(kind, *m, prob.N)
            o.update_settings(**kw)
            if ib is not None:
                o.set_bound_constraints(*[a[:, :, b] for a in ib])
            else:
                o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
            if refs:
                o.set_x_ref(case["xref"])
                o.set_u_ref(case["uref"])
            if ext:
                o.set_fdyn(case["fdyn"])
                o.set_cone_constraints(cu[0], cu[1], cu[2], cx[0], cx[1], cx[2])
            if rows is not None:
                o.set_linear_constraints(*rows)
            if il is not None:
                kx, ku = np.abs(il[0][:, :, b]).sum(axis=1) > 0, np.abs(il[2][:, :, b]).sum(axis=1) > 0
                o.set_linear_constraints(il[0][kx, :, b], il[1][kx, b], il[2][ku, :, b], il[3][ku, b])
            if adaptive:
                o.set_sensitivity(*sens)
                o.set_adaptive_rho(1, ADAPTIVE["rho_min"], ADAPTIVE["rho_max"], ADAPTIVE["clip"])
            return o
        return mk
    rho = ADAPTIVE["rho_max"] if adaptive else (float(fam[4].max()) if het else prob.rho)
    return dict(name=name, tag=f"{case['tag']} {name}", make=make, refs=refs, het=het, ext=ext, rows=rows, adaptive=adaptive,
                sens=sens, cones=(cu, cx), rho=rho, ib=ib, il=il)


def _loop(mk, x0, adaptive):
    """every instance on its own CpuSolver, on pc.NTHREADS threads (the library calls release the interpreter; the Riccati
    recursion of a 64-state family 70 times over is what an arm's oracle side costs): dict like solve_batch's, with the adapted
    rho, Kinf, Pinf of an adaptive solve"""
    from concurrent.futures import ThreadPoolExecutor
    nx, Bn = x0.shape

    def one(b):
        o = mk(b)
        o.set_x0(x0[:, b])
        o.solve()
        r = o.get_solution()
        if adaptive:
            r["adapted"] = o.get_adapted()
        o.close()
        return r
    with ThreadPoolExecutor(pc.NTHREADS) as pool:
        rs = list(pool.map(one, range(Bn)))
    out = dict(x=np.stack([r["x"] for r in rs], axis=2), u=np.stack([r["u"] for r in rs], axis=2),
               iter=np.array([r["iter"] for r in rs], dtype=np.int32), solved=np.array([r["solved"] for r in rs], dtype=np.int32),
               res=np.stack([r["res"] for r in rs], axis=0))
    if adaptive:
        out.update(rho=np.array([r["adapted"]["rho"] for r in rs]), Kinf=np.stack([r["adapted"]["Kinf"] for r in rs], axis=2),
                   Pinf=np.stack([r["adapted"]["Pinf"] for r in rs], axis=2))
    for a in out.values():
        a.setflags(write=False)
    return out


def arm_ref(case, name):
    """orc64's result of an arm, computed once"""
    key = (case["tag"], name, "orc64")
    if key not in _oracles:
        a = arm(case, name)
        _oracles[key] = _loop(a["make"]("orc64"), case["x0"], a["adaptive"])
    return _oracles[key]


def arm_pair(case, name):
    """(orc64 result, orc32 result, limit, e32, agreement share) of an arm, computed once.  limit = precision1_limit: the bar of
    the arm at precision 1"""
    key = (case["tag"], name)
    if key not in _oracles:
        a = arm(case, name)
        r64 = arm_ref(case, name)
        r32 = _loop(a["make"]("orc32"), case["x0"], a["adaptive"])
        limit, e32, same = precision1_limit(r32, r64)
        _oracles[key] = (r64, r32, limit, e32, same)
    return _oracles[key]


def rho_limit(r64, r32):
    """(limit, orc32's worst relative distance from orc64's adapted rho over the agreeing instances): adaptive_pair's rule"""
    agree = (r32["iter"] == r64["iter"]) & (r32["solved"] == r64["solved"])
    drho = float((np.abs(r32["rho"] - r64["rho"]) / r64["rho"])[agree].max())
    return max(1e-5, 4.0 * drho), drho


def binding_share(case, a, r64):
    """share of the instances with an input at its bound, on the input cone's surface or at an input row, at some knot, in orc64's
    solution (the box set's slack: at a bound exactly, on the other sets to the solve's tolerance)"""
    prob, u = case["prob"], r64["u"]
    if a["ib"] is not None:
        lo, hi = a["ib"][2], a["ib"][3]
    else:
        lo, hi = prob.u_min[:, :, None], prob.u_max[:, :, None]
    scale = np.abs(u).max()
    hit = ((u >= hi - 1e-9 * scale) | (u <= lo + 1e-9 * scale)).any(axis=(0, 1))
    cu = a["cones"][0]
    if a["ext"] and len(cu[0]):
        s, d, mu = cu[0][0], cu[1][0], cu[2][0]
        head, axis = np.sqrt((u[s:s + d - 1] ** 2).sum(axis=0)), u[s + d - 1]
        hit |= ((head >= 0.999 * mu * axis) & (head > 1e-6)).any(axis=0)
    if a["rows"] is not None:
        hit |= (np.einsum("ij,jkb->ikb", a["rows"][2], u) >= a["rows"][3][:, None, None] - 1e-9).any(axis=(0, 1))
    if a["il"] is not None:
        au = np.einsum("ijb,jkb->ikb", a["il"][2], u)
        present = np.abs(a["il"][2]).sum(axis=1) > 0
        hit |= ((au >= a["il"][3][:, None, :] - 1e-9) & present[:, None, :]).any(axis=(0, 1))
    return float(hit.mean())


def state_share(case, a, r64):
    """share of the instances with a state at its bound at some knot after the first (precision1_cases.state_bound_share)"""
    prob = case["prob"]
    lo, hi = (a["ib"][0][:, 1:, :], a["ib"][1][:, 1:, :]) if a["ib"] is not None else (prob.x_min[:, 1:, None], prob.x_max[:, 1:, None])
    scale = np.abs(r64["x"]).max(axis=(1, 2), keepdims=True)
    x = r64["x"][:, 1:, :]
    return float(((x >= hi - 1e-9 * scale) | (x <= lo + 1e-9 * scale)).any(axis=(0, 1)).mean())


def sweep_counts(case):
    A, Bm, Q, R, rho = case["fam"]
    return [t.host_precompute_sweeps(A[:, :, b], Bm[:, :, b], Q[:, :, b], R[:, :, b], rho[b]) for b in range(B)]


def conditions(case, arms, report=print):
    """the figures of every arm of a case and the list of the conditions it misses (empty: all met) — what
    tests/test_stream_forms_inputs.py asserts, and what the seeds were chosen by"""
    from tests.util import FP32_TOL
    missed, shares = [], []
    for name in arms:
        a = arm(case, name)
        r64, r32, limit, e32, same = arm_pair(case, name)
        ub, sb, solved = binding_share(case, a, r64), state_share(case, a, r64), float(r64["solved"].mean())
        line = f"{a['tag']}: e32 {e32:.2e} agreement {same:.2f} solved {solved:.2f} binding {ub:.2f} state {sb:.2f}"
        shares.append(solved)
        if e32 > FP32_TOL:
            missed.append(f"{a['tag']}: orc32 is {e32:.2e} from orc64")
        if same < 0.9:
            missed.append(f"{a['tag']}: the oracles agree on the exit of {same:.2f} of the instances only")
        if ub < 0.1:
            missed.append(f"{a['tag']}: an input at a bound, cone or row on {ub:.2f} of the instances only")
        if sb < 0.2:
            missed.append(f"{a['tag']}: a state at its bound on {sb:.2f} of the instances only")
        if a["adaptive"]:
            rl, drho = rho_limit(r64, r32)
            moved = float((np.abs(r64["rho"] - case["prob"].rho) > 0.05).mean())
            line += f" rho {r64['rho'].min():.3f}..{r64['rho'].max():.3f} moved {moved:.2f} orc32 within {drho:.1e}"
            if moved < 0.5:
                missed.append(f"{a['tag']}: rho leaves the family's value on {moved:.2f} of the instances only")
            if drho > 1e-5:
                missed.append(f"{a['tag']}: orc32's rho is {drho:.1e} from orc64's")
        if a["het"] and name == "het":
            n = len(set(sweep_counts(case)))
            line += f" sweep counts {n}"
            if n < 8:
                missed.append(f"{a['tag']}: {n} distinct Riccati sweep counts only")
        report(line)
    if not any(0.1 <= s <= 0.9 for s in shares):
        missed.append(f"{case['tag']}: solved shares {shares}: no arm with both exits")
    return missed
