"""Inputs and route table of the batch-independence tests: one place, used by the CPU-only conditions
(tests/test_independence_inputs.py, the oracles alone) and by the GPU comparisons (tests/test_batch_independence_gpu.py,
tests/test_history_independence_gpu.py), so that what the conditions establish is what the kernels are run on.  Its model is
tests/precision1_cases.py.

The rule under test: an instance's result depends only on its own current inputs — not on where it sits in the batch, not on its
neighbours, not on the batch size, not on what the solver was configured for before.

A *route* (ROUTES) is a kernel family, the switches that force it, a shape, a batch size and a calling pattern:
    id        name of the route
    group     routes of one group run in one parametrised GPU case
    geom      key of GEOMETRY: the sizes, in instances, of the units the kernel lays the batch out in
    env       the TINYMPC_HIP_* switches that force the family
    kernel    what last_launch_name must report in every run (the kernel the comparisons are of)
    family    what kernel_name must report (the routed family; equal to `kernel` unless stated)
    scaled    lean routes: what the hook tmpc_lean_last_scaled must report
    B         batch size: the suite's smallest ragged size of the family
    inputs    name and arguments of the builder of the base batch (BUILDERS)
    pattern   "oneshot" (cold, nothing kept), "kept2" (two warm-started solves, the second from A x0), "rollout" (mpc_rollout(3))
    arrangements  which of "permuted", "neighbours", "truncated" the route is held to (noise routes: the last two — noise is
              keyed by (seed, b, t) by design, so an instance's draw moves with its position)
    hard      the factor a hard instance's x0 starts from (replace_neighbours)
    first_check  whether a trivial instance stops at the first check (below)
    specialised  the kernel is compiled for the solver's layout at setup (csrc/jit.cpp): the route runs with specialisation on, its
              names are matched as prefixes, and it is skipped where there is no compiler

A base batch is (shared, per): `shared` holds what every instance has in common (the family, shared bounds and references, the
affine term, cones, rows, adaptive settings, precision, metric configuration, noise factors); `per` holds the per-instance
inputs, each with the instance on its LAST axis: x0 and, where the route takes them, xref / uref, ib_* (set_instance_bounds),
fam_* (from_families), plant_* (set_plant), w (set_disturbance), traj_x / traj_u (set_ref_trajectory), est_C / est_L
(set_estimator).  An arrangement is an index operation on `per` alone (take, replace_neighbours).

The three arrangements of a batch of B instances:
    permuted    one fixed permutation of every per-instance input (permutation(): drawn with a fixed seed, rejected unless it
                moves an instance across and within every unit of the family's geometry and into and out of every ragged tail)
    neighbours  S = every third instance plus the whole ragged tail stays; every other instance is replaced, alternately, by a
                hard one (the same draw scaled up until the oracle runs it to max_iter unsolved with the input bound active:
                replace_neighbours) and a trivial one (x0 = 0, zero per-instance references, trajectory and disturbance)
    truncated   the first B' instances, B' = truncated_size(): the largest size <= B - 17 that is no multiple of any unit

A trivial instance stops at the first check wherever zero is the solution of the zero-state problem.  Where the route has
non-zero shared references or an affine term (the rocket's gravity) it is not: x0 = 0 then is a tracking problem like any other.
Those routes carry first_check = False; nothing is asked of their trivial instances' exit.

Seeds.  The x0 draws are the families' generators (tinympc_julia_amd.problems) at the seeds below, each instance's state scaled
by its own factor in [0.05, 1] so that the instances of a batch leave at many different iterations (the rocket's are spread
around xinit instead: rocket()): cartpole 11, quadrotor 4 (tests/mfma_cases.py's), random families 300 + 10 nx + nu
(tests/precision1_cases.py's), the rocket's own draw 1300 + N.  With these orc32 takes orc64's exit on >= 0.9 of S in every route
(tests/test_independence_inputs.py asserts it and prints the share: 1.000 on all but four routes, 0.944 at the lowest — the
rocket with cones at N = 10 and 13), so none had to be replaced."""
import os

import numpy as np

import tinympc_julia_amd as t

STEPS = 3                       # closed loops
NTHREADS = max(1, min(16, len(os.sched_getaffinity(0))))
SWITCHES = ("TINYMPC_HIP_GROUP", "TINYMPC_HIP_NO_QUAD", "TINYMPC_HIP_NO_MFMA", "TINYMPC_HIP_NO_MFMAT", "TINYMPC_HIP_NO_MFMAR",
            "TINYMPC_HIP_NO_MFMAC", "TINYMPC_HIP_MFMAC_ALL", "TINYMPC_HIP_NO_STREAM", "TINYMPC_HIP_NO_LEAN", "TINYMPC_HIP_NO_REFILL",
            "TINYMPC_HIP_LEAN_DENSE", "TINYMPC_HIP_LEAN_UNSCALED", "TINYMPC_HIP_LEAN_WS", "TINYMPC_HIP_LEAN_LOOP",
            "TINYMPC_HIP_STREAM_F64", "TINYMPC_HIP_STREAM_MPC", "TINYMPC_HIP_STREAM_LOOP", "TINYMPC_HIP_ESTIMATOR_SPLIT",
            "TINYMPC_HIP_NO_UNI", "TINYMPC_HIP_NO_OS", "TINYMPC_HIP_STRICT_FP32", "TINYMPC_HIP_MFMAT_ALL")

# Units of a family's batch layout, in instances, smallest first.  Lanes-per-instance kernels (G lanes an instance, 256-thread
# workgroups): the DPP quad holds 4 / G instances, the DPP row 16 / G, the wavefront 64 / G, the workgroup 256 / G.  The lean
# kernel and the quad g1 entries run one lane an instance.  The matrix-core kernels work on tiles of 16 instances, mfma with four
# tiles a workgroup.  The stream kernel runs four lanes an instance.  The generic kernel one thread an instance; its workgroup of
# 256 exceeds the batch, so the wavefront is its only boundary here.
GEOMETRY = dict(lean=(4, 16, 64, 256), quad_g4=(4, 16, 64), quad_g2=(2, 8, 32, 128), quad_g1=(4, 16, 64, 256), mfma=(16, 64),
                mfmat=(16,), stream=(4, 16, 64), generic=(4, 16, 64))
BATCH = dict(lean=289, quad_g4=70, quad_g2=131, quad_g1=259, mfma=87, mfmat=39, stream=70, generic=70)
ARRANGEMENTS = ("permuted", "neighbours", "truncated")
SETTING_NAMES = ("tol", "fixed")


# ---- arrangements ----
def tails(B, units):
    """{unit: first instance of its ragged tail} for every unit the batch is no multiple of"""
    return {u: (B // u) * u for u in units if B % u and B > u}


def crosses(perm, units):
    """the condition on a permutation (arranged instance j holds base instance perm[j]): per unit, some instance changes its
    unit and some its place within the unit; per ragged tail, some instance moves into it and some out of it"""
    perm = np.asarray(perm)
    B, pos = len(perm), np.arange(len(perm))
    for u in units:
        if u >= B:
            continue
        if not np.any(perm // u != pos // u) or not np.any(perm % u != pos % u):
            return False
    for u, start in tails(B, units).items():
        if not np.any((perm >= start) & (pos < start)) or not np.any((perm < start) & (pos >= start)):
            return False
    return True


def permutation(B, units, seed=2024):
    rng = np.random.default_rng(seed)
    for _ in range(100):
        perm = rng.permutation(B)
        if crosses(perm, units):
            return perm
    raise AssertionError("no permutation crosses every boundary")


def kept_set(B, units):
    """S: every third instance plus the whole ragged tail of the largest unit the batch is no multiple of"""
    keep = np.zeros(B, dtype=bool)
    keep[::3] = True
    tl = tails(B, units)
    if tl:
        keep[tl[max(tl)]:] = True
    return np.nonzero(keep)[0]


def truncated_size(B, units):
    """the largest B' <= B - 17 that cuts through every unit: no multiple of any of them"""
    for Bp in range(B - 17, 0, -1):
        if all(Bp % u for u in units if u > 1):
            return Bp
    raise AssertionError("no truncated size")


def take(per, idx):
    return {k: np.asfortranarray(v[..., idx]) for k, v in per.items()}


ZEROED = ("xref", "uref", "traj_x", "traj_u", "w")


ESCALATIONS = 6


def replace_neighbours(route, shared, per, keep):
    """(arranged per, indices of the hard instances, indices of the trivial ones).  A hard instance is its draw at full size
    (the spread factor divided out, its largest component brought to the batch's largest) times the route's `hard` factor,
    doubled — at most ESCALATIONS times — until orc64 runs it to max_iter unsolved with the input bound active"""
    B = per["x0"].shape[-1]
    out = {k: np.array(v, order="F") for k, v in per.items()}
    others = np.setdiff1d(np.arange(B), keep)
    hard_idx, trivial_idx = others[0::2], others[1::2]
    full = out["x0"] / out["spread"]
    rel = (np.abs(full) / np.abs(full).max(axis=1, keepdims=True)).max(axis=0)
    out["x0"][:, hard_idx] = (full / rel)[:, hard_idx] * route["hard"]
    kw = shared["kw"]["tol"]
    todo = hard_idx
    for _ in range(ESCALATIONS):
        r = oracle_first_solve(shared, out, "orc64", kw, todo)
        ok = np.array([r["iter"][j] == kw["max_iter"] and not r["solved"][j] and input_bound_active(shared, out, int(b), r["u"][:, :, j])
                       for j, b in enumerate(todo)], dtype=bool)
        todo = todo[~ok]
        if not len(todo):
            break
        out["x0"][:, todo] *= 2.0
    out["x0"][:, trivial_idx] = 0.0
    for k in ZEROED:
        if k in out:
            out[k][..., trivial_idx] = 0.0
    return out, hard_idx, trivial_idx


_arranged = {}


def arrange(route, name):
    """(arranged per, columns of the arranged batch to compare, the base columns they must equal, hard, trivial), built once per
    (inputs, geometry, hard factor) and handed out read-only"""
    shared, per = base_batch(route)
    key = (route["inputs"][0], tuple(sorted(route["inputs"][1].items())), route["B"], route["geom"], route["hard"], name)
    if key in _arranged:
        return _arranged[key]
    B, units = route["B"], GEOMETRY[route["geom"]]
    none = np.zeros(0, dtype=int)
    if name == "permuted":
        perm = permutation(B, units)
        out = (take(per, perm), np.arange(B), perm, none, none)
    elif name == "neighbours":
        keep = kept_set(B, units)
        arr, hard, trivial = replace_neighbours(route, shared, per, keep)
        out = (arr, keep, keep, hard, trivial)
    else:
        Bp = truncated_size(B, units)
        out = (take(per, np.arange(Bp)), np.arange(Bp), np.arange(Bp), none, none)
    for a in out[0].values():
        a.setflags(write=False)
    _arranged[key] = out
    return out


# ---- the base batches ----
def _spread(x0, seed):
    """(x0 with each instance's state scaled by its own factor in [0.05, 1] — many different iteration counts in one batch —,
    the factors: per["spread"], which no solver reads and a hard instance divides out again)"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 1.0, x0.shape[1])
    return np.asfortranarray(x0 * f[None, :]), f


def _references(nx, nu, N, B, mode, seed, sx, su, base=None):
    if mode == "zero":
        return None, None
    rng = np.random.default_rng(seed)
    xr0, ur0 = base if base is not None else (np.zeros((nx, N)), np.zeros((nu, N - 1)))
    if mode == "shared":
        return np.asfortranarray(xr0 + sx * rng.standard_normal((nx, N))), np.asfortranarray(ur0 + su * rng.standard_normal((nu, N - 1)))
    amp = rng.uniform(0.0, 1.0, B)            # (an instance's references scale with a factor of its own: easy and hard targets)
    return (np.asfortranarray(xr0[:, :, None] + sx * amp * rng.standard_normal((nx, N, B))),
            np.asfortranarray(ur0[:, :, None] + su * amp * rng.standard_normal((nu, N - 1, B))))


def _kw(tol_pri=1e-3, tol_dua=1e-3, max_iter=40, fixed_iter=15):
    return dict(tol=dict(abs_pri_tol=tol_pri, abs_dua_tol=tol_dua, max_iter=max_iter, check_termination=1),
                fixed=dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=fixed_iter, check_termination=1))


def _put_refs(shared, per, xref, uref):
    if xref is None:
        return
    if xref.ndim == 3:
        per["xref"], per["uref"] = xref, uref
    else:
        shared["xref"], shared["uref"] = xref, uref


def cartpole(B, N=20, refs="zero", xb=False, adaptive=False, precision=0, tol=1e-3):
    prob = t.problems.cartpole(N, u_bound=0.5)
    x0, spread = _spread(t.problems.cartpole_x0(B, seed=11), 1100 + N)
    if xb:      # rows 0, 1 at +-0.5 max |x0[row]|, the upper bound 10 % higher from knot N/2 on (per-knot bounds)
        lim = 0.5 * np.abs(x0).max(axis=1)
        for r in range(2):
            prob.x_min[r, :], prob.x_max[r, :] = -lim[r], lim[r]
            prob.x_max[r, N // 2:] = 1.1 * lim[r]
    shared, per = dict(prob=prob, kw=_kw(tol, tol), precision=precision), dict(x0=x0, spread=spread)
    _put_refs(shared, per, *_references(4, 1, N, B, refs, 7000 + 10 * N + len(refs), 0.05, 0.02))
    if adaptive:
        dK, dP, _, _ = t.host_sensitivity(prob.A, prob.B, prob.Q, prob.R, prob.rho)
        shared["adaptive"] = dict(sens=(dK, dP), rho_min=0.1, rho_max=10.0, clip=True)
    return shared, per


def quadrotor(B, N=10, refs="zero", xb=False, adaptive=False):
    prob = t.problems.quadrotor(N)
    x0, spread = _spread(t.problems.quadrotor_x0(B, seed=4), 1200 + N)
    if xb:      # rows 0-2 at +-0.15: half the states' largest size, as tests/mfma_cases.py's +-0.31 is of its unscaled draw
        prob.x_min[:3, :], prob.x_max[:3, :] = -0.15, 0.15
    shared, per = dict(prob=prob, kw=_kw()), dict(x0=x0, spread=spread)
    _put_refs(shared, per, *_references(12, 4, N, B, refs, 9000 + 10 * N + len(refs), 0.05, 0.02))
    if adaptive:
        from tests import mfma_cases
        shared["adaptive"] = dict(sens=mfma_cases.tables(), rho_min=0.1, rho_max=10.0, clip=True)
    return shared, per


ROCKET_CONES = ([0], [3], [0.25], [0], [3], [0.5])


def rocket(B, N=10, refs="per_instance", cones=True, fdyn=True, lin=False):
    """the rocket with its affine term, one cone per side and its own box.  The family's references start at xinit, so the states
    are spread AROUND it: x0[b] = xinit (1 + d_b U(-1, 1)^6) with d_b in [0, 0.5] — an instance close to the references leaves
    early, one far from them late.  A hard instance is the same draw twice as far out: the thrust then sits on its bound of 105"""
    prob = t.problems.rocket(N)
    rng = np.random.default_rng(1300 + N)
    d = rng.uniform(0.0, 0.5, B)
    x0 = np.asfortranarray(prob.extra["xinit"][:, None] * (1.0 + d[None, :] * rng.uniform(-1.0, 1.0, (6, B))))
    shared = dict(prob=prob, kw=_kw(2e-3, 1e-3))
    per = dict(x0=x0, spread=np.ones(B))
    if fdyn:
        shared["fdyn"] = prob.fdyn
    if cones:
        shared["cones"] = ROCKET_CONES
    if lin:
        shared["lin"] = (np.array([[0.0, 0.0, 0.0, 1.0, 1.0, 0.0]]), np.array([0.5]), np.array([[1.0, -1.0, 0.0]]), np.array([4.0]))
    xr, ur = t.problems.rocket_refs(N)
    if refs == "per_instance":      # the family's references plus a perturbation of each instance's own size
        amp = rng.uniform(0.0, 1.0, B)
        per["xref"] = np.asfortranarray(xr[:, :, None] + 0.2 * amp * rng.standard_normal((6, N, B)))
        per["uref"] = np.asfortranarray(ur[:, :, None] + 0.2 * amp * rng.standard_normal((3, N - 1, B)))
    elif refs == "shared":
        shared["xref"], shared["uref"] = xr, ur
    return shared, per


def random_family(B, nx=5, nu=2, N=9, precision=0):
    """tests/precision1_cases.py's random family outside the built-in shapes (the generic kernel's)"""
    rng = np.random.default_rng(300 + 10 * nx + nu)
    A = np.eye(nx) + 0.1 * rng.standard_normal((nx, nx))
    Bm = rng.standard_normal((nx, nu))
    prob = t.problems.Problem("rand", A, Bm, np.diag(np.array([5.0, 2.0, 1.0, 3.0, 0.5])[:nx]), np.diag([1.0, 2.0][:nu]), 2.0, N)
    prob.x_min, prob.x_max = np.full((nx, N), -2.0), np.full((nx, N), 2.0)
    prob.u_min, prob.u_max = np.full((nu, N - 1), -0.3), np.full((nu, N - 1), 0.3)
    x0, spread = _spread(np.asfortranarray(rng.uniform(-1, 1, (nx, B))), 1500)
    return dict(prob=prob, kw=_kw(), precision=precision), dict(x0=x0, spread=spread)


def cartpole_families(B, N=17):
    """one family per instance, perturbed cartpoles (tests/precision1_cases.py::families_case's draw)"""
    shared, per = cartpole(B, N)
    base = shared["prob"]
    rng = np.random.default_rng(41)
    per["fam_A"] = np.asfortranarray(np.repeat(base.A[:, :, None], B, axis=2) * (1.0 + 0.02 * rng.standard_normal((4, 4, B))))
    per["fam_B"] = np.asfortranarray(np.repeat(base.B[:, :, None], B, axis=2) * (1.0 + 0.05 * rng.standard_normal((4, 1, B))))
    Q, R = np.zeros((4, 4, B), order="F"), np.zeros((1, 1, B), order="F")
    for b in range(B):
        Q[:, :, b] = np.diag(np.array([10.0, 1.0, 10.0, 1.0]) * rng.uniform(0.5, 2.0, 4))
        R[:, :, b] = rng.uniform(0.5, 2.0)
    per["fam_Q"], per["fam_R"], per["fam_rho"] = Q, R, rng.uniform(0.5, 3.0, B)
    return shared, per


def cartpole_instance_bounds(B, N=17):
    """box bounds per instance and knot: the input box at +-U(0.3, 0.7), 10 % wider from knot N/2 on; rows 0, 1 of the state at
    +-U(0.4, 0.8) of the batch's largest |x0[row]|"""
    shared, per = cartpole(B, N)
    rng = np.random.default_rng(43)
    ub = rng.uniform(0.3, 0.7, B)
    umax = np.ones((1, N - 1, 1)) * ub
    umax[:, N // 2:, :] *= 1.1
    xmax = np.full((4, N, B), 1e17)
    lim = np.abs(per["x0"]).max(axis=1)
    for r in range(2):
        xmax[r] = lim[r] * rng.uniform(0.4, 0.8, B)
    per["ib_xmin"], per["ib_xmax"] = np.asfortranarray(-xmax), np.asfortranarray(xmax)
    per["ib_umin"], per["ib_umax"] = np.asfortranarray(-umax), np.asfortranarray(umax)
    return shared, per


def own_plant(B, N=20, traj="per_instance", noise=False):
    """the own-plant chain on the cartpole: one plant per instance (the model off by 2 % / 5 %, an offset), one disturbance per
    instance, a reference trajectory, an estimator measuring rows 0 and 2 with a sensor gain and the steady-state Kalman gain of
    its own, metrics on; with `noise` process and measurement noise at 1 % of the states' scale"""
    shared, per = cartpole(B, N)
    prob, x0 = shared["prob"], per["x0"]
    rng = np.random.default_rng(51)
    scale = np.abs(x0).max(axis=1)
    per["plant_A"] = np.asfortranarray(prob.A[:, :, None] * (1.0 + 0.02 * rng.standard_normal((4, 4, B))))
    per["plant_B"] = np.asfortranarray(prob.B[:, :, None] * (1.0 + 0.05 * rng.standard_normal((4, 1, B))))
    per["plant_f"] = np.asfortranarray(0.002 * scale[:, None] * rng.standard_normal((4, B)))
    per["w"] = np.asfortranarray(0.01 * scale[:, None, None] * rng.standard_normal((4, STEPS, B)))
    L = N + STEPS
    amp = rng.uniform(0.0, 1.0, B)
    tx = 0.05 * amp * np.sin(np.linspace(0.0, 2.0, L))[None, :, None] * rng.standard_normal((4, 1, B))
    tu = 0.02 * amp * rng.standard_normal((1, L, B))
    if traj == "per_instance":
        per["traj_x"], per["traj_u"] = np.asfortranarray(tx), np.asfortranarray(tu)
    else:
        shared["traj"] = (np.asfortranarray(tx[:, :, 0]), np.asfortranarray(tu[:, :, 0]))
    sel = np.eye(4)[[0, 2]]
    C = np.asfortranarray(sel[:, :, None] * rng.uniform(0.9, 1.1, B))
    gain = np.zeros((4, 2, B), order="F")
    for b in range(B):
        gain[:, :, b] = t.kalman_gain(prob.A, C[:, :, b], 0.01 * scale, 0.01 * scale)
    per["est_C"], per["est_L"] = C, gain
    shared["metrics"] = dict(x_lo=-0.5 * scale, x_hi=0.5 * scale, u_lo=[-0.45], u_hi=[0.45])
    if noise:
        shared["noise"] = dict(gw=0.01 * scale, gv=0.01 * scale, seed_w=77, seed_v=78)
    return shared, per


BUILDERS = dict(cartpole=cartpole, quadrotor=quadrotor, rocket=rocket, random_family=random_family, cartpole_families=cartpole_families,
                cartpole_instance_bounds=cartpole_instance_bounds, own_plant=own_plant)
_built = {}


def base_batch(route):
    """(shared, per) of a route, built once and handed out read-only"""
    name, kwargs = route["inputs"]
    key = (name, route["B"], tuple(sorted(kwargs.items())))
    if key not in _built:
        shared, per = BUILDERS[name](route["B"], **kwargs)
        for a in per.values():
            a.setflags(write=False)
        _built[key] = (shared, per)
    return _built[key]


# ---- the route table ----
def _route(id, group, geom, env, kernel, inputs, pattern="oneshot", hard=4.0, family=None, scaled=None, first_check=True,
           arrangements=ARRANGEMENTS, B=None, specialised=False):
    return dict(id=id, group=group, geom=geom, env=dict(env), kernel=kernel, family=family or kernel, scaled=scaled,
                B=B or BATCH[geom], inputs=inputs, pattern=pattern, hard=hard, first_check=first_check, arrangements=tuple(arrangements),
                specialised=specialised)


LEAN, LEAN5 = "lean<4,1,20>", "lean<4,1,5>"
G1 = {"TINYMPC_HIP_GROUP": "1"}
NOISY = ("neighbours", "truncated")
ROUTES = []

# lean<4,1,20>, one-shot: the scaled sparse sweeps (the default), the unscaled sparse ones, the dense ones; with a state bound;
# with shared references; lean<4,1,5>
for _id, _env, _inp, _scaled, _fc in (
        ("lean_scaled", {}, dict(), 1, True), ("lean_unscaled", {"TINYMPC_HIP_LEAN_UNSCALED": "1"}, dict(), 0, True),
        ("lean_dense", {"TINYMPC_HIP_LEAN_DENSE": "1"}, dict(), 0, True), ("lean_state_bound", {}, dict(xb=True), 0, True),
        ("lean_shared_refs", {}, dict(refs="shared"), 0, False)):
    ROUTES.append(_route(_id, "lean_oneshot", "lean", dict(G1, **_env), LEAN, ("cartpole", _inp), family="quad<4,1,20,g1>",
                         scaled=_scaled, first_check=_fc))
ROUTES.append(_route("lean_N5", "lean_oneshot", "lean", G1, LEAN5, ("cartpole", dict(N=5, tol=2e-4)), family="quad<4,1,5,g1>", scaled=0, hard=8.0))
# lean<4,1,20>, the other calling patterns: the workspace-keeping kernels and the in-kernel loop
_WS = dict(G1, TINYMPC_HIP_LEAN_WS="1")
ROUTES.append(_route("lean_ws_kept2", "lean_ws", "lean", _WS, LEAN, ("cartpole", dict()), "kept2", family="quad<4,1,20,g1>", scaled=0))
ROUTES.append(_route("lean_ws_loop", "lean_ws", "lean", dict(_WS, TINYMPC_HIP_LEAN_LOOP="1"), LEAN, ("cartpole", dict()), "rollout",
                     family="quad<4,1,20,g1>", scaled=0))

# quad<4,1,20>, 4, 2 and 1 lanes an instance (the lean kernel switched off): the three reference modes x the three patterns
for _g in (4, 2, 1):
    for _refs in ("zero", "shared", "per_instance"):
        for _pat in ("oneshot", "kept2", "rollout"):
            ROUTES.append(_route(f"quad_g{_g}_{_refs}_{_pat}", f"quad_g{_g}_{_refs}", f"quad_g{_g}",
                                 {"TINYMPC_HIP_GROUP": str(_g), "TINYMPC_HIP_NO_LEAN": "1"}, f"quad<4,1,20,g{_g}>",
                                 ("cartpole", dict(refs=_refs)), _pat, first_check=_refs != "shared"))
# quad, other shapes: trajectories or rows in LDS, the shortest horizon, the adaptive variant
_G4 = {"TINYMPC_HIP_GROUP": "4", "TINYMPC_HIP_NO_MFMA": "1", "TINYMPC_HIP_NO_MFMAT": "1"}
ROUTES.append(_route("quad_12_4_20", "quad_shapes", "quad_g4", _G4, "quad<12,4,20,g4>", ("quadrotor", dict(N=20, refs="per_instance", xb=True)),
                     hard=3.0))
ROUTES.append(_route("quad_6_3_10", "quad_shapes", "quad_g4", _G4, "quad<6,3,10,g4>", ("rocket", dict(N=10, cones=False, fdyn=False)),
                     hard=2.0))
ROUTES.append(_route("quad_4_1_2", "quad_shapes", "quad_g4", _G4, "quad<4,1,2,g4>", ("cartpole", dict(N=2, tol=1e-5)), hard=8.0))
ROUTES.append(_route("quad_adp", "quad_shapes", "quad_g4", _G4, "quad<4,1,20,g4>", ("cartpole", dict(adaptive=True)), "kept2"))

# mfma<12,4,10> and <12,4,30>: one-shot, kept workspace, per-instance references, a state bound, adaptive rho
for _N in (10, 30):
    _m = f"mfma<12,4,{_N}>"
    ROUTES.append(_route(f"mfma{_N}_oneshot", f"mfma{_N}", "mfma", {}, _m, ("quadrotor", dict(N=_N)), hard=3.0))
    ROUTES.append(_route(f"mfma{_N}_kept2", f"mfma{_N}", "mfma", {}, _m, ("quadrotor", dict(N=_N)), "kept2", hard=3.0))
    ROUTES.append(_route(f"mfma{_N}_refs", f"mfma{_N}", "mfma", {}, _m, ("quadrotor", dict(N=_N, refs="per_instance")), "kept2", hard=3.0))
    ROUTES.append(_route(f"mfma{_N}_xb", f"mfma{_N}", "mfma", {}, _m, ("quadrotor", dict(N=_N, xb=True)), hard=3.0))
    ROUTES.append(_route(f"mfma{_N}_adp", f"mfma{_N}", "mfma", {}, _m, ("quadrotor", dict(N=_N, adaptive=True)), "kept2", hard=3.0))

# mfmat<6,3,10>: the rocket with its affine term, both cones and per-instance references (the second set of LDS cells)
for _pat in ("oneshot", "kept2", "rollout"):
    ROUTES.append(_route(f"mfmat_{_pat}", "mfmat", "mfmat", {}, "mfmat<6,3,10>", ("rocket", dict(N=10)), _pat, hard=2.0, first_check=False))
# ... and one specialised layout: the same solver with a linear row on either side
ROUTES.append(_route("mfmat_rows", "mfmat_rows", "mfmat", {}, "mfmat<6,3,10>", ("rocket", dict(N=10, lin=True)), hard=2.0, first_check=False,
                     specialised=True))
# the three-wavefront kernels behind it: mfmar<6,3,10>, and mfmac at a horizon without a compiled entry; one-shot with cones
_NOT = {"TINYMPC_HIP_NO_MFMAT": "1"}
ROUTES.append(_route("mfmar", "mfmar", "mfmat", _NOT, "mfmar<6,3,10>", ("rocket", dict(N=10, refs="shared")), hard=2.0, first_check=False))
ROUTES.append(_route("mfmac", "mfmar", "mfmat", _NOT, "mfmac<6,3>", ("rocket", dict(N=13, refs="shared")), hard=2.0, first_check=False))

# stream4: (4,1) at N = 17, (6,3) at N = 12, (12,4) at N = 7 — horizons without a lanes-per-instance entry
_NQ = {"TINYMPC_HIP_NO_QUAD": "1", "TINYMPC_HIP_NO_MFMAT": "1", "TINYMPC_HIP_NO_MFMAR": "1", "TINYMPC_HIP_NO_MFMAC": "1"}
_MPC = dict(_NQ, TINYMPC_HIP_STREAM_MPC="1")
ROUTES.append(_route("stream_4_1", "stream_plain", "stream", _NQ, "stream4<4,1>", ("cartpole", dict(N=17, refs="per_instance")), "kept2"))
ROUTES.append(_route("stream_6_3", "stream_plain", "stream", _NQ, "stream4<6,3>", ("rocket", dict(N=12, cones=False, fdyn=False)), hard=2.0))
ROUTES.append(_route("stream_12_4", "stream_plain", "stream", _NQ, "stream4<12,4>", ("quadrotor", dict(N=7, refs="shared")), hard=3.0,
                     first_check=False))
ROUTES.append(_route("stream_ext", "stream_ext", "stream", _NQ, "stream4<6,3>", ("rocket", dict(N=12, lin=True)), "kept2", hard=2.0,
                     first_check=False))
ROUTES.append(_route("stream_families", "stream_ext", "stream", _NQ, "stream4<4,1>", ("cartpole_families", dict()), "kept2"))
ROUTES.append(_route("stream_ib", "stream_ext", "stream", _NQ, "stream4<4,1;ib>", ("cartpole_instance_bounds", dict())))
ROUTES.append(_route("stream_adp", "stream_ext", "stream", _NQ, "stream4<4,1>", ("cartpole", dict(N=17, adaptive=True)), "kept2"))
ROUTES.append(_route("stream_f64", "stream_ext", "stream", dict(_NQ, TINYMPC_HIP_STREAM_F64="1"), "stream4<4,1;f64>",
                     ("cartpole", dict(N=17, precision=2))))
ROUTES.append(_route("stream_mpc", "stream_loop", "stream", _MPC, "stream4<4,1>", ("cartpole", dict(N=17)), "rollout"))
ROUTES.append(_route("stream_mpc_loop", "stream_loop", "stream", dict(_MPC, TINYMPC_HIP_STREAM_LOOP="1"), "stream4<4,1>",
                     ("cartpole", dict(N=17)), "rollout"))

# generic (5,2,9) at precision 0 and 2
ROUTES.append(_route("generic_p0", "generic", "generic", {}, "generic", ("random_family", dict())))
ROUTES.append(_route("generic_p2", "generic", "generic", {}, "generic<f64>", ("random_family", dict(precision=2))))

# the own-plant chain (plant_step_kernel, estimator_step_kernel, rollout_metrics_kernel; 256 / nx = 64 instances a workgroup)
# on a lean, a quad and a stream solver: the estimator fused and split, and with noise.  The lean kernel takes zero or shared
# references, so its solver tracks one shared trajectory; the quad and stream solvers one trajectory per instance.
_SPLIT = {"TINYMPC_HIP_ESTIMATOR_SPLIT": "1"}
for _tag, _geom, _env, _kernel, _family, _inp in (
        ("lean", "lean", _WS, LEAN, "quad<4,1,20,g1>", dict(traj="shared")),
        ("quad", "quad_g4", {"TINYMPC_HIP_GROUP": "4"}, "quad<4,1,20,g4>", None, dict()),
        ("stream", "stream", _NQ, "stream4<4,1>", None, dict(N=17))):
    ROUTES.append(_route(f"chain_{_tag}", f"chain_{_tag}", _geom, _env, _kernel, ("own_plant", _inp), "rollout", family=_family))
    ROUTES.append(_route(f"chain_{_tag}_split", f"chain_{_tag}", _geom, dict(_env, **_SPLIT), _kernel, ("own_plant", _inp), "rollout",
                         family=_family))
    ROUTES.append(_route(f"chain_{_tag}_noise", f"chain_{_tag}", _geom, _env, _kernel, ("own_plant", dict(_inp, noise=True)), "rollout",
                         family=_family, arrangements=NOISY))

# mfma refill (admm_mfma_kernel<..., WS = false, RF = true>): a finished instance's slot takes the next unstarted instance, the most
# position-dependent code in the library.  One case at tests/test_gpu_parity.py::test_mfma_refill_is_the_same_solve's size, draw
# and settings (a multiple of 64 and more than two rounds of resident workgroups: launch_mfma_refill refills; zero references, a
# check every 10 iterations), held to the permuted and the neighbours arrangement — a truncated batch is another launch geometry
# and, below two rounds, not the refill kernel.  Its oracle is the batch oracle (cpu_oracle.solve_batch), 40 960 instances in
# seconds; its hard instances start at six times the batch's largest state.
REFILL = dict(id="mfma_refill", geom="mfma", env={}, kernel="mfma<12,4,30>", family="mfma<12,4,30>", B=40960, N=30, hard=6.0,
              kw=dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=10), arrangements=("permuted", "neighbours"))
_refill = {}


def refill_batch():
    """(prob, x0) of the refill route"""
    if "base" not in _refill:
        prob = t.problems.quadrotor(REFILL["N"], u_bound=0.5)
        rng = np.random.default_rng(5)
        x0 = t.problems.quadrotor_x0(REFILL["B"], seed=9)
        x0[:, rng.integers(0, REFILL["B"], REFILL["B"] // 3)] *= 0.1      # a third of the instances are easy: slots turn over at different rates
        x0.setflags(write=False)
        _refill["base"] = (prob, x0)
    return _refill["base"]


def refill_oracle(x0, kind="orc64"):
    from oracle import cpu_oracle
    return cpu_oracle.solve_batch(kind, refill_batch()[0], np.asfortranarray(x0), nthreads=NTHREADS, **REFILL["kw"])


def refill_neighbours():
    """(x0 with the neighbours replaced, S, hard, trivial): replace_neighbours' rule on the batch oracle"""
    if "neighbours" not in _refill:
        prob, x0 = refill_batch()
        B = REFILL["B"]
        keep = kept_set(B, (1,) + GEOMETRY["mfma"])      # (no ragged tail at a multiple of 64: every third instance)
        others = np.setdiff1d(np.arange(B), keep)
        hard_idx, trivial_idx = others[0::2], others[1::2]
        full = t.problems.quadrotor_x0(B, seed=9)
        rel = (np.abs(full) / np.abs(full).max(axis=1, keepdims=True)).max(axis=0)
        out = np.array(x0, order="F")
        out[:, hard_idx] = (full / rel)[:, hard_idx] * REFILL["hard"]
        todo = hard_idx
        for _ in range(ESCALATIONS):
            r = refill_oracle(out[:, todo])
            ok = (r["iter"] == REFILL["kw"]["max_iter"]) & (r["solved"] == 0) & (np.abs(r["u"]).max(axis=(0, 1)) >= 0.5 - 1e-9)
            todo = todo[~ok]
            if not len(todo):
                break
            out[:, todo] *= 2.0
        out[:, trivial_idx] = 0.0
        out.setflags(write=False)
        _refill["neighbours"] = (out, keep, hard_idx, trivial_idx)
    return _refill["neighbours"]


def refill_oracle_on_kept(kind="orc64"):
    key = ("kept", kind)
    if key not in _refill:
        keep = refill_neighbours()[1]
        r = refill_oracle(refill_batch()[1][:, keep], kind)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refill[key] = r
    return _refill[key]


# ---- part B: configuration history ----
# Three routes, each with a target configuration T (a base batch above; metrics on, so that the rollout after the solve has
# them) and a decoy that differs from T in every setter the route accepts.  The decoy is installed in four stages, because the
# library refuses some combinations: (0, a cold and a warm solve on T's own kernel) other settings, other input bounds, other
# references of T's kind, overridden cache terms; (A, a solve) other settings, other bounds with a finite state bound, references of the other
# kind, a non-zero affine term, other cones and rows, adaptive rho, precision 1, compaction, overridden cache terms; (B, a solve)
# adaptive rho off (it does not go with per-instance bounds), per-instance bounds; (C, a rollout) shared bounds again, compaction off
# (a chunked solve has no closed loop), a per-instance plant, a disturbance, a per-instance reference trajectory, an estimator,
# process and measurement noise, metrics with other weights and limits.
# The way back to T is the public API: every setter again with T's value; None drops the plant, the disturbance, the trajectory,
# the estimator, the noise; set_rollout_metrics(False); set_compaction(0); set_precision(0); set_adaptive_rho(False) and reset()
# (which returns the adapted rho to the family's); the affine term as zeros; no cones / rows as empty lists and enable_cones(0, 0) /
# enable_linear(0, 0); zero references as all-zero arrays (set_ref maps them to "no references"); the cache terms as
# get_cache_terms() returned them before the override.  No decoy setting is left out: the API has a way back from each.
HISTORY = [
    dict(id="lean", route="lean_shared_refs", kernel=LEAN, family="quad<4,1,20,g1>", rollout_kernel="quad<4,1,20,g1>", env=G1),
    dict(id="mfma", route="mfma10_refs", kernel="mfma<12,4,10>", family="mfma<12,4,10>", rollout_kernel="mfma<12,4,10>", env={}),
    dict(id="stream", route="stream_ext", kernel="stream4<6,3>", family="stream4<6,3>", rollout_kernel="stream4<6,3>", env=_MPC),
]


def route_by_id(id):
    return [r for r in ROUTES if r["id"] == id][0]


def target_of(case):
    """(shared with T's metric configuration, per) of a history case: the route's base batch"""
    shared, per = base_batch(route_by_id(case["route"]))
    scale = np.abs(per["x0"]).max(axis=1)
    nu = shared["prob"].nu
    return dict(shared, metrics=dict(x_lo=-0.5 * scale, x_hi=0.5 * scale, u_lo=np.full(nu, -0.4), u_hi=np.full(nu, 0.4))), per


def decoy_of(shared, per):
    """the decoy's arrays, drawn with a fixed seed from the target's shapes"""
    prob, x0 = shared["prob"], per["x0"]
    nx, nu, N, B = prob.nx, prob.nu, prob.N, x0.shape[1]
    rng = np.random.default_rng(97)
    scale = np.abs(x0).max(axis=1)
    d = dict(kw=dict(abs_pri_tol=5e-3, abs_dua_tol=5e-3, max_iter=25, check_termination=5))
    d["x0"] = np.asfortranarray(0.7 * x0[:, rng.permutation(B)])
    xmin, xmax = np.array(prob.x_min), np.array(prob.x_max)
    xmin[0, :], xmax[0, :] = -0.4 * scale[0], 0.4 * scale[0]
    d["bounds"] = (xmin, xmax, 0.6 * prob.u_min, 0.6 * prob.u_max)
    sx, su = 0.1 * scale.mean(), 0.1 * float(np.abs(prob.u_max).min())
    if "xref" in per:         # T per instance: the decoy's shared
        d["xref"], d["uref"] = sx * rng.standard_normal((nx, N)), su * rng.standard_normal((nu, N - 1))
    else:
        d["xref"], d["uref"] = sx * rng.standard_normal((nx, N, B)), su * rng.standard_normal((nu, N - 1, B))
    # (0) ... and references of T's own kind with other values: the first decoy solves stay on T's kernel, whose images they fill
    d["xref_same"], d["uref_same"] = (sx * rng.standard_normal((nx, N, B)), su * rng.standard_normal((nu, N - 1, B))) if "xref" in per else \
        (sx * rng.standard_normal((nx, N)), su * rng.standard_normal((nu, N - 1)))
    d["fdyn"] = 0.01 * scale * rng.standard_normal(nx) + (shared["fdyn"] if "fdyn" in shared else 0.0)
    d["cones"] = ([], [], [], [1], [2], [0.7]) if nu < 2 else ([0], [2], [0.6], [1], [2], [0.7])
    d["lin"] = (rng.standard_normal((1, nx)), np.array([0.3 * scale.mean()]), rng.standard_normal((1, nu)), np.array([0.3 * float(np.abs(prob.u_max).min())]))
    d["adaptive"] = dict(rho_min=0.5, rho_max=5.0, clip=True)
    d["compaction"] = 5
    d["ib"] = (np.asfortranarray(-scale[:, None] * rng.uniform(0.3, 0.9, (nx, B))), np.asfortranarray(scale[:, None] * rng.uniform(0.3, 0.9, (nx, B))),
               np.asfortranarray(prob.u_min[:, :1] * rng.uniform(0.3, 0.9, (nu, B))), np.asfortranarray(prob.u_max[:, :1] * rng.uniform(0.3, 0.9, (nu, B))))
    d["plant"] = (np.asfortranarray(prob.A[:, :, None] * (1.0 + 0.02 * rng.standard_normal((nx, nx, B)))),
                  np.asfortranarray(prob.B[:, :, None] * (1.0 + 0.05 * rng.standard_normal((nx, nu, B)))),
                  np.asfortranarray(0.002 * scale[:, None] * rng.standard_normal((nx, B))))
    d["w"] = np.asfortranarray(0.01 * scale[:, None, None] * rng.standard_normal((nx, STEPS, B)))
    d["traj"] = (np.asfortranarray(sx * rng.standard_normal((nx, N + STEPS, B))), np.asfortranarray(su * rng.standard_normal((nu, N + STEPS, B))))
    C = np.eye(nx)[[0, 2] if nx == 4 else list(range(nx // 2))]      # the position rows: a detectable pair on all three families
    d["est"] = (C, t.kalman_gain(prob.A, C, 0.01 * scale, 0.01 * scale))
    d["noise"] = dict(gw=0.01 * scale, gv=0.01 * scale, seed_w=5, seed_v=6)
    d["metrics"] = dict(qw=np.full(nx, 2.0), rw=np.full(nu, 3.0), x_lo=-0.1 * scale, x_hi=0.2 * scale, u_lo=np.full(nu, -0.1), u_hi=np.full(nu, 0.1))
    return d


GROUPS = list(dict.fromkeys(r["group"] for r in ROUTES))


def routes_of(group):
    return [r for r in ROUTES if r["group"] == group]


# ---- the oracle side ----
def settings_of(route, setting):
    return base_batch(route)[0]["kw"][setting]


def first_references(shared, per, b):
    """the references instance b's first solve runs against: its own, the window of its trajectory at cursor 0, or the shared"""
    N = shared["prob"].N
    if "xref" in per:
        return per["xref"][:, :, b], per["uref"][:, :, b]
    if "traj_x" in per:
        f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
        return t.ref_window(f32(per["traj_x"][:, :, b]), 0, N), t.ref_window(f32(per["traj_u"][:, :, b]), 0, N - 1)
    if "traj" in shared:
        f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
        return t.ref_window(f32(shared["traj"][0]), 0, N), t.ref_window(f32(shared["traj"][1]), 0, N - 1)
    if "xref" in shared:
        return shared["xref"], shared["uref"]
    return None, None


def oracle_solver(shared, per, b, kind, kw):
    """a cold, fully configured CpuSolver of instance b's first solve"""
    from oracle import cpu_oracle
    prob = shared["prob"]
    if "fam_A" in per:
        fam = (per["fam_A"][:, :, b], per["fam_B"][:, :, b], per["fam_Q"][:, :, b], per["fam_R"][:, :, b], float(per["fam_rho"][b]))
    else:
        fam = (prob.A, prob.B, prob.Q, prob.R, prob.rho)
    o = cpu_oracle.CpuSolver(kind, *fam, prob.N)
    o.update_settings(**kw)
    if "ib_umin" in per:
        o.set_bound_constraints(*[per[k][:, :, b] for k in ("ib_xmin", "ib_xmax", "ib_umin", "ib_umax")])
    else:
        o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if "fdyn" in shared:
        o.set_fdyn(shared["fdyn"])
    if "cones" in shared:
        o.set_cone_constraints(*shared["cones"])
    if "lin" in shared:
        o.set_linear_constraints(*shared["lin"])
    xr, ur = first_references(shared, per, b)
    if xr is not None:
        o.set_x_ref(xr)
        o.set_u_ref(ur)
    if "adaptive" in shared:
        a = shared["adaptive"]
        o.set_sensitivity(*a["sens"])
        o.set_adaptive_rho(1, a["rho_min"], a["rho_max"], a["clip"])
    return o


def oracle_first_solve(shared, per, kind, kw, cols=None):
    """the first (cold) solve of the instances `cols` (default: all), each on its own CpuSolver: dict like solve_batch's, the
    instance on the last axis, columns in `cols`' order"""
    prob = shared["prob"]
    cols = np.arange(per["x0"].shape[-1]) if cols is None else np.asarray(cols)
    n = len(cols)
    out = dict(x=np.zeros((prob.nx, prob.N, n)), u=np.zeros((prob.nu, prob.N - 1, n)), iter=np.zeros(n, dtype=np.int32),
               solved=np.zeros(n, dtype=np.int32), res=np.zeros((n, 4)))
    for j, b in enumerate(cols):
        o = oracle_solver(shared, per, int(b), kind, kw)
        o.set_x0(per["x0"][:, b])
        o.solve()
        r = o.get_solution()
        out["x"][:, :, j], out["u"][:, :, j] = r["x"], r["u"]
        out["iter"][j], out["solved"][j], out["res"][j] = r["iter"], r["solved"], r["res"]
        o.close()
    return out


_oracles = {}


def oracle_on_kept(route, setting="tol", kind="orc64"):
    """the base batch's first solve on S, computed once per (inputs, setting, kind) and handed out read-only"""
    shared, per = base_batch(route)
    keep = kept_set(route["B"], GEOMETRY[route["geom"]])
    key = (route["inputs"][0], tuple(sorted(route["inputs"][1].items())), route["B"], route["geom"], setting, kind)
    if key not in _oracles:
        r = oracle_first_solve(shared, per, kind, shared["kw"][setting], keep)
        for a in r.values():
            a.setflags(write=False)
        _oracles[key] = r
    return _oracles[key]


def input_bound_active(shared, per, b, u):
    """whether |u| sits on instance b's input bound somewhere in a solution u (nu, N-1)"""
    prob = shared["prob"]
    lo, hi = (per["ib_umin"][:, :, b], per["ib_umax"][:, :, b]) if "ib_umin" in per else (prob.u_min, prob.u_max)
    scale = max(1.0, float(np.abs(u).max()))
    return bool(np.any(u >= hi - 1e-9 * scale) or np.any(u <= lo + 1e-9 * scale))
