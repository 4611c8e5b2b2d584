"""Routes, transitions and inputs of the setter-transition tests: one place, used by the CPU-only conditions
(tests/test_transition_inputs.py, the oracles alone) and by the GPU comparisons (tests/test_setter_transitions_gpu.py).  Its model
is tests/independence_cases.py, whose builders, switches and oracle side it reuses.

The rule under test: a solver that has solved under configuration A and then receives EXACTLY ONE setter call taking it to A'
gives, bit for bit, what a fresh solver configured as A' gives.  One call, so that no neighbouring setter can invalidate a cached
device image (packs_dirty, lin_dirty, adapt_dirty, sens_dirty, the routing key, lean_jit, lean_ok, lean_knot_bounds,
state_bounds_active, g_maybe_nonzero) on behalf of the one that forgot to.

A *configuration* is a dict (base_cfg): prob (the family with its shared bounds), kw (the settings, en_state_bound /
en_input_bound included), precision, strict, warm (the workspace is kept), compaction, fdyn, cones, cones_on, lin, lin_on (the
enable switches as last set by tinympc_enable_cones / enable_linear; None: never called), xref, uref (None: zero; 2-D shared;
3-D per instance), cache (overridden cache terms), adaptive, ib (per-instance bounds), il (per-instance rows).

A *route* (ROUTES) is a base configuration and the name its first launch must report:
    id, n       name and number in the list below
    env         the TINYMPC_HIP_* switches that force the family
    jit         the route exists only with specialisation on (tests/test_jit.py: the jit_on fixture)
    inputs      builder of tests/independence_cases.py and its arguments
    B           batch size: a full unit of the route's layout plus a ragged tail — 256 + 37 on the lean routes, three tiles of 16 + 5 on
                the matrix-core routes, 64 + 6 elsewhere; route 11 from 20 480 up, where one lane per instance becomes the variant of a
                shape specialised at setup (Solver::upload_packs: lean_jit) and lean_plan is asked at all
    precision, warm   of the base configuration
    kernel, family    last_launch_name and kernel_name of the first solve
     1 lean           lean<4,1,20>, cold one-shot, precision 0
     2 quad_kept      quad<4,1,20,g1>, workspace kept
     3 mfma           mfma<12,4,10>, cold one-shot
     4 mfmat          mfmat<6,3,10>: the rocket with its affine term and one cone per side, shared references
     5 stream_ext     stream4<6,3> with cones and rows, N = 12, workspace kept
     6 stream_plain   stream4<4,1>, N = 17, workspace kept
     7 generic        generic: (5, 2, 9), no instantiation
     8 p2_lean        precision 2 with specialisation on: lean<4,1,20;f64> under the family generic<f64>
     9 p2_generic     precision 2 on generic<f64>, N = 17
    10 p2_stream      precision 2 with TINYMPC_HIP_STREAM_F64: stream4<4,1;f64>, workspace kept
    11 p0_lean_jit    precision 0 with specialisation on: cartpole N = 12, the lean variant specialised at the first solve

A *transition* (TRANSITIONS) is (id, group, kind, base, delta, fwd, rev, routes):
    group   the number of the list in the issue this work answers (1 rows ... 13 compaction; 14, set_batch_size on the
            process-global surface, is a test of its own in the GPU file)
    kind    "change": orc64 at A' must differ from orc64 at A by more than CHANGE on at least half of the instances (a condition on
            the inputs: tests/test_transition_inputs.py); "neutral": the solution stays, the launch may change
    base    keys the route's base configuration is given first, to make A (a transition that needs rows starts from rows)
    delta   keys that differ between A and A'
    fwd, rev   the key whose ONE public call takes A to A', and A' back to A (one_call)
Every transition runs in both directions.  Values are functions of the route's data (data_of), all rounded to fp32 first, so
that the precision-2 routes see on the device exactly what the oracle sees.

Left out, with the reason:
    route 11, groups 1-4 (rows, cones, their switches, the affine term): with specialisation on at precision 0 each would
    specialise a constraint-layout unit (jit_trans_for), tens of seconds a piece; tests/test_mfmat_general_gpu.py covers that path.
    At precision 2 routing returns before any layout is specialised, so route 8 takes every transition.
    set_strict_precision on the precision-2 routes: strict_fp32() is read by the routes of precision 0 and 1 only.

Instances compared: all of the batch.  Instances anchored to orc64 and checked on the CPU (cols_of): all of them up to 300; of
route 11's 20 517 the first workgroup of 256 and the ragged tail of 37."""
import copy

import numpy as np

import tinympc_julia_amd as t
from tests import independence_cases as ic

CHANGE = 1e-3          # 100 x FP32_TOL: what "A' is another problem than A" means
MIN_SHARE = 0.5


def f32(a):
    """rounded to fp32 (what the device holds); +-1e17, "no bound", stays what it is"""
    if a is None:
        return None
    a = np.asarray(a, dtype=np.float64)
    return np.asfortranarray(np.where(np.abs(a) >= 1e17, a, a.astype(np.float32).astype(np.float64)))


_NQ = ic._NQ
ROUTES = [
    dict(id="lean", n=1, env=ic.G1, jit=False, inputs=("cartpole", dict(N=20)), B=293, precision=0, warm=False,
         kernel="lean<4,1,20>", family="quad<4,1,20,g1>"),
    dict(id="quad_kept", n=2, env=ic.G1, jit=False, inputs=("cartpole", dict(N=20)), B=70, precision=0, warm=True,
         kernel="quad<4,1,20,g1>", family="quad<4,1,20,g1>"),
    dict(id="mfma", n=3, env={}, jit=False, inputs=("quadrotor", dict(N=10)), B=53, precision=0, warm=False,
         kernel="mfma<12,4,10>", family="mfma<12,4,10>"),
    dict(id="mfmat", n=4, env={}, jit=False, inputs=("rocket", dict(N=10, refs="shared")), B=53, precision=0, warm=False,
         kernel="mfmat<6,3,10>", family="mfmat<6,3,10>"),
    dict(id="stream_ext", n=5, env=_NQ, jit=False, inputs=("rocket", dict(N=12, refs="shared", lin=True)), B=70, precision=0, warm=True,
         kernel="stream4<6,3>", family="stream4<6,3>"),
    dict(id="stream_plain", n=6, env=_NQ, jit=False, inputs=("cartpole", dict(N=17)), B=70, precision=0, warm=True,
         kernel="stream4<4,1>", family="stream4<4,1>"),
    dict(id="generic", n=7, env={}, jit=False, inputs=("random_family", dict()), B=70, precision=0, warm=False,
         kernel="generic", family="generic"),
    dict(id="p2_lean", n=8, env={}, jit=True, inputs=("cartpole", dict(N=20)), B=293, precision=2, warm=False,
         kernel="lean<4,1,20;f64>", family="generic<f64>"),
    dict(id="p2_generic", n=9, env={}, jit=False, inputs=("cartpole", dict(N=17)), B=70, precision=2, warm=False,
         kernel="generic<f64>", family="generic<f64>"),
    dict(id="p2_stream", n=10, env=dict(_NQ, TINYMPC_HIP_STREAM_F64="1"), jit=False, inputs=("cartpole", dict(N=17)), B=70, precision=2,
         warm=True, kernel="stream4<4,1;f64>", family="stream4<4,1;f64>"),
    dict(id="p0_lean_jit", n=11, env={}, jit=True, inputs=("cartpole", dict(N=12)), B=20480 + 37, precision=0, warm=False,
         kernel="lean<4,1,12>", family="quad<4,1,12,g4>"),
]


def route_by_id(id):
    return [r for r in ROUTES if r["id"] == id][0]


def cols_of(route):
    B = route["B"]
    return np.arange(B) if B <= 300 else np.concatenate([np.arange(256), np.arange(B - 37, B)])


# ---- base configurations ----
_base = {}


def base_cfg(route):
    """(configuration, per-instance inputs) of a route, built once; the inputs are read-only"""
    if route["id"] not in _base:
        name, kwargs = route["inputs"]
        shared, per = ic.BUILDERS[name](route["B"], **kwargs)
        prob = copy.copy(shared["prob"])
        prob.x_min, prob.x_max, prob.u_min, prob.u_max = (f32(a) for a in (prob.x_min, prob.x_max, prob.u_min, prob.u_max))
        cfg = dict(prob=prob, kw=dict(shared["kw"]["tol"], en_state_bound=1, en_input_bound=1), precision=route["precision"], strict=False,
                   warm=route["warm"], compaction=0, fdyn=f32(shared.get("fdyn")), cones=shared.get("cones"), cones_on=None,
                   lin=tuple(f32(a) for a in shared["lin"]) if "lin" in shared else None, lin_on=None, xref=f32(shared.get("xref")),
                   uref=f32(shared.get("uref")), cache=None, adaptive=None, ib=None, il=None)
        x0 = f32(per["x0"])
        x0.setflags(write=False)
        _base[route["id"]] = (cfg, dict(x0=x0))
    return _base[route["id"]]


# ---- what the transitions set: per route, rounded to fp32 ----
# Chosen on the CPU until tests/test_transition_inputs.py holds on every route (the shares it prints are in
# profiles/transition_routes.txt): a cone or a state bound that the fixed x0 itself violates on most instances acts from the first
# iteration on; the tight input box lies well inside what the instances ask for.  And chosen so that fp32 state reaches them:
# where orc32, the same loop in fp32, leaves orc64 by 1e-4 and more, FP32_TOL is not what the kernels are documented to hold
# (DESIGN.md section 9.3).  That ruled out the rocket without gravity UNDER its thrust cone, whose apex the inputs then sit on
# (orc32 off by 1.4e-3: the affine-term transition starts from a configuration without cones, and the rocket's non-zero vector
# is its gravity), a state row most x0 violate beside an input row that forces every input negative (cartpole N = 12: 4e-5), and
# per-instance boxes narrower than the tight shared one (quadrotor: 6e-5).
U_TIGHT = dict(cartpole=(-0.0625, 0.0625), quadrotor=(-0.03125, 0.03125), rocket=(-0.5, 10.5), rand=(-0.0625, 0.0625))
_data = {}


def data_of(route):
    if route["id"] in _data:
        return _data[route["id"]]
    cfg, per = base_cfg(route)
    prob, x0 = cfg["prob"], per["x0"]
    nx, nu, N, B = prob.nx, prob.nu, prob.N, x0.shape[1]
    rng = np.random.default_rng(500 + route["n"])
    scale = np.abs(x0).max(axis=1)
    rocket = prob.name == "rocket"
    d = {}
    # 1 rows: the first state below a line that some x0 lie above and others reach later (the rocket's: most lie above), the
    # first input below a small positive number, which most instances ask to exceed at some knot (the rocket's: a negative one)
    Ax, Au = np.zeros((1, nx)), np.zeros((1, nu))
    Ax[0, 0], Au[0, 0] = 1.0, 1.0
    d["lin"] = tuple(f32(a) for a in (Ax, [0.75 * scale[0] if rocket else 0.5 * scale[0]], Au, [(-0.05 if rocket else 0.02) * abs(float(prob.u_max[0, 0]))]))
    # 2 a cone: ||(x0, x1)|| <= mu x2 and, where there are inputs enough, ||(u0[, u1])|| <= mu u_last
    mu = 0.125 if rocket else 0.5
    cu = ([0], [min(3, nu)], [mu]) if nu >= 2 else ([], [], [])
    d["cones"] = cu + ([0], [3], [mu])
    d["none_cones"] = ([], [], [], [], [], [])
    d["none_lin"] = (np.zeros((0, nx)), np.zeros(0), np.zeros((0, nu)), np.zeros(0))
    # 4 the affine term
    d["fdyn"] = cfg["fdyn"] if rocket else f32(0.02 * scale * np.where(np.arange(nx) % 2, -1.0, 1.0))      # (the rocket's: gravity)
    # 5 bounds: a tight uniform input box; the same with the upper half of the horizon at half the width; a binding state bound
    lo, hi = U_TIGHT[prob.name]
    inf_x = (np.full((nx, N), -1e17), np.full((nx, N), 1e17))
    tight = copy.copy(prob)
    tight.x_min, tight.x_max, tight.u_min, tight.u_max = inf_x[0], inf_x[1], f32(np.full((nu, N - 1), lo)), f32(np.full((nu, N - 1), hi))
    knot = copy.copy(tight)
    knot.u_min, knot.u_max = tight.u_min.copy(), tight.u_max.copy()
    mid = 0.5 * (lo + hi)
    knot.u_min[:, N // 2:] = f32(mid + 0.5 * (lo - mid))
    knot.u_max[:, N // 2:] = f32(mid + 0.5 * (hi - mid))
    free = copy.copy(prob)
    free.x_min, free.x_max = inf_x
    xb = copy.copy(free)
    xb.x_min, xb.x_max = free.x_min.copy(), free.x_max.copy()
    xb.x_min[0, :], xb.x_max[0, :] = f32(-0.1 * scale[0]), f32(0.1 * scale[0])
    d["prob_tight"], d["prob_knot"], d["prob_free"], d["prob_xb"] = tight, knot, free, xb
    # 6 settings
    kw = cfg["kw"]
    d["kw_no_xb"], d["kw_no_ub"] = dict(kw, en_state_bound=0), dict(kw, en_input_bound=0)
    d["kw_loose"] = dict(kw, abs_pri_tol=32.0 * kw["abs_pri_tol"], abs_dua_tol=32.0 * kw["abs_dua_tol"], max_iter=12)
    d["kw_tight"] = dict(kw, abs_pri_tol=kw["abs_pri_tol"] / 16.0, abs_dua_tol=kw["abs_dua_tol"] / 16.0)      # (most instances pass the fifth iteration, where rho adapts)
    # 7 references: shared, per instance (the shared ones plus a perturbation of each instance's own size)
    base_x = cfg["xref"] if cfg["xref"] is not None else np.zeros((nx, N))
    base_u = cfg["uref"] if cfg["uref"] is not None else np.zeros((nu, N - 1))
    su = 0.25 * float(np.abs(prob.u_max).min()) if not rocket else 2.0
    d["xref_shared"] = f32(base_x + 0.5 * scale[:, None] * rng.standard_normal((nx, N)))
    d["xref_per"] = f32(d["xref_shared"][:, :, None] + 0.5 * scale[:, None, None] * rng.uniform(0.2, 1.0, B) * rng.standard_normal((nx, N, B)))
    d["uref_shared"] = f32(base_u + su * rng.standard_normal((nu, N - 1)))
    # 8 the cache terms, perturbed (tests/test_history_independence_gpu.py's factors)
    d["cache_own"] = t.host_precompute(prob.A, prob.B, prob.Q, prob.R, prob.rho)
    K, P, Qi, Am = (d["cache_own"][k] for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt"))
    d["cache"] = dict(Kinf=1.05 * K, Pinf=1.02 * P, Quu_inv=Qi, AmBKt=0.99 * Am)
    # 9 adaptive rho: the sensitivities are the library's own (computed on first use: host_sensitivity is that computation)
    dK, dP = t.host_sensitivity(prob.A, prob.B, prob.Q, prob.R, prob.rho)[:2]
    d["adaptive"] = dict(sens=(dK, dP), rho_min=0.1, rho_max=10.0, clip=True)
    # 12 per instance and knot: the tight box scaled per instance; the row of 1 with a right-hand side of each instance's own
    w = rng.uniform(1.0, 2.0, B)
    ones_x, ones_u = np.ones((nx, N, 1)), np.ones((nu, N - 1, 1))
    d["ib"] = tuple(f32(a) for a in (-1e17 * ones_x * np.ones(B), 1e17 * ones_x * np.ones(B), mid + (lo - mid) * ones_u * w, mid + (hi - mid) * ones_u * w))
    lx, lu = d["lin"][1][0], d["lin"][3][0]
    d["il"] = (f32(np.repeat(Ax[:, :, None], B, axis=2)), f32((lx + 0.05 * scale[0] * w)[None, :]), f32(np.repeat(Au[:, :, None], B, axis=2)),
               f32((lu * w)[None, :]))
    _data[route["id"]] = d
    return d


# ---- the transition table ----
def _tr(id, group, kind, base, delta, fwd, rev=None, routes=None):
    return dict(id=id, group=group, kind=kind, base=base, delta=delta, fwd=fwd, rev=rev or fwd, routes=routes)


NO_JIT_P0 = tuple(r["id"] for r in ROUTES if r["id"] != "p0_lean_jit")      # groups 1-4 (see above)
P0 = tuple(r["id"] for r in ROUTES if r["precision"] == 0)
P2 = tuple(r["id"] for r in ROUTES if r["precision"] == 2)
V = lambda key: (lambda d: d[key])          # a value of the route's data
C = lambda v: (lambda d: v)                 # a constant

TRANSITIONS = [
    # 1 set_linear_constraints with rows that bind (from no rows)
    _tr("rows", 1, "change", dict(lin=C(None)), dict(lin=V("lin")), "lin", routes=NO_JIT_P0),
    # 2 set_cone_constraints with a cone that binds (from no cones)
    _tr("cone", 2, "change", dict(cones=C(None)), dict(cones=V("cones")), "cones", routes=NO_JIT_P0),
    # 3 the switches, from a configuration that has rows / cones: off, and (the reverse direction) on again with non-zero arguments
    _tr("rows_off", 3, "change", dict(lin=V("lin")), dict(lin_on=C((0, 0))), "lin_on", routes=NO_JIT_P0),
    _tr("cones_off", 3, "change", dict(cones=V("cones")), dict(cones_on=C((0, 0))), "cones_on", routes=NO_JIT_P0),
    # 4 set_fdyn to a non-zero vector, and (reverse) back to zero
    _tr("fdyn", 4, "change", dict(fdyn=C(None), cones=C(None)), dict(fdyn=V("fdyn")), "fdyn", routes=NO_JIT_P0),
    # 5 set_bound_constraints
    _tr("bounds_by_knot", 5, "change", dict(prob=V("prob_tight")), dict(prob=V("prob_knot")), "prob"),
    _tr("state_bound", 5, "change", dict(prob=V("prob_free")), dict(prob=V("prob_xb")), "prob"),
    _tr("bounds_value", 5, "change", dict(prob=V("prob_free")), dict(prob=V("prob_tight")), "prob"),
    # 6 update_settings: one flag, or the tolerances and max_iter
    _tr("en_state_bound", 6, "change", dict(prob=V("prob_xb")), dict(kw=V("kw_no_xb")), "kw"),
    _tr("en_input_bound", 6, "change", dict(prob=V("prob_tight")), dict(kw=V("kw_no_ub")), "kw"),
    _tr("tolerances", 6, "change", dict(), dict(kw=V("kw_loose")), "kw"),
    # 7 references: zero -> shared -> per instance -> shared (the reverse direction of the second), and the inputs' alone
    _tr("xref_zero_shared", 7, "change", dict(xref=C(None)), dict(xref=V("xref_shared")), "xref"),
    _tr("xref_shared_per", 7, "change", dict(xref=V("xref_shared")), dict(xref=V("xref_per")), "xref"),
    _tr("uref_zero_shared", 7, "change", dict(uref=C(None)), dict(uref=V("uref_shared")), "uref"),
    # 8 set_cache_terms with a perturbed cache (reverse: with the family's own terms again)
    _tr("cache", 8, "change", dict(), dict(cache=V("cache")), "cache"),
    # 9 set_adaptive_rho on, and (reverse) off
    _tr("adaptive", 9, "change", dict(kw=V("kw_tight")), dict(adaptive=V("adaptive")), "adaptive"),
    # 10 set_precision 0 -> 2 and (reverse) 2 -> 0, 0 -> 1; set_strict_precision at precision 1
    _tr("precision_0_2", 10, "neutral", dict(), dict(precision=C(2)), "precision", routes=P0),
    _tr("precision_2_0", 10, "neutral", dict(), dict(precision=C(0)), "precision", routes=P2),
    _tr("precision_0_1", 10, "neutral", dict(), dict(precision=C(1)), "precision", routes=P0),
    _tr("strict", 10, "neutral", dict(precision=C(1)), dict(strict=C(True)), "strict", routes=P0),
    # 11 set_warm_start on and off: whichever the route's base is not
    _tr("warm", 11, "neutral", dict(), dict(warm=lambda d: "flip"), "warm"),
    # 12 per-instance bounds and back through set_bound_constraints; per-instance rows and back through set_linear_constraints
    _tr("instance_bounds", 12, "change", dict(prob=V("prob_free")), dict(ib=V("ib")), "ib", rev="prob"),
    _tr("instance_rows", 12, "change", dict(lin=C(None)), dict(il=V("il")), "il", rev="lin"),
    _tr("instance_rows_from_shared", 12, "change", dict(lin=V("lin")), dict(lin=C(None), il=V("il")), "il", rev="lin", routes=NO_JIT_P0),
    # 13 set_compaction to a chunk smaller than max_iter, and (reverse) to 0
    _tr("compaction", 13, "neutral", dict(), dict(compaction=C(7)), "compaction"),
]


def transition_by_id(id):
    return [x for x in TRANSITIONS if x["id"] == id][0]


def applies(route, tr):
    return tr["routes"] is None or route["id"] in tr["routes"]


CASES = [(r["id"], x["id"]) for r in ROUTES for x in TRANSITIONS if applies(r, x)]

# What the neutral transitions must do to the launch, where reading Solver::select_kernel and lean_plan settles it: (route,
# transition) -> last_launch_name at A'.  The others' names are compared between the used and the fresh solver and printed.
LAUNCH_AT = {
    ("lean", "precision_0_2"): "generic<f64>", ("lean", "precision_0_1"): "quad<4,1,20,g1>", ("lean", "warm"): "quad<4,1,20,g1>",
    ("quad_kept", "warm"): "lean<4,1,20>", ("quad_kept", "precision_0_2"): "generic<f64>",
    ("mfma", "precision_0_2"): "generic<f64>", ("mfmat", "precision_0_2"): "generic<f64>", ("generic", "precision_0_2"): "generic<f64>",
    ("stream_ext", "precision_0_2"): "generic<f64>", ("stream_plain", "precision_0_2"): "generic<f64>",
    ("p2_lean", "warm"): "generic<f64>", ("p2_lean", "precision_2_0"): "quad<4,1,20,g4>",
    ("p2_generic", "precision_2_0"): "stream4<4,1>", ("p2_stream", "precision_2_0"): "stream4<4,1>",
    ("p0_lean_jit", "precision_0_2"): "lean<4,1,12;f64>", ("p0_lean_jit", "warm"): "quad<4,1,12,g4>",
}
# Refusals: (route, transition, direction) -> a word of the message.  None is known: every combination above has a kernel.
REFUSALS = {}


def configs(route, tr):
    """(A, A') of a transition on a route"""
    cfg, _ = base_cfg(route)
    d = data_of(route)
    a = dict(cfg)
    for k, f in tr["base"].items():
        a[k] = f(d)
    b = dict(a)
    for k, f in tr["delta"].items():
        v = f(d)
        b[k] = (not a[k]) if (k == "warm" and v == "flip") else v
    return a, b


def label(route, tr, side):
    """a name for a configuration: A of the transitions without a `base` is the route's own base, one configuration"""
    if side == "A" and not tr["base"]:
        return f"{route['id']}/base"
    return f"{route['id']}/{tr['id']}/{side}"


# ---- one public call ----
def one_call(bs, key, target, route):
    """the ONE call that sets `key` to the target configuration's value"""
    d = data_of(route)
    v = target[key]
    if key == "lin":
        bs.set_linear_constraints(*(v if v is not None else d["none_lin"]))
    elif key == "cones":
        bs.set_cone_constraints(*(v if v is not None else d["none_cones"]))
    elif key == "lin_on":
        bs.enable_linear(*(v if v is not None else (1, 1)))
    elif key == "cones_on":
        en = v if v is not None else (1, 1)
        if bs.lib.tinympc_enable_cones(bs.h, int(en[0]), int(en[1])) != 0:
            raise t.TinyMPCError("tinympc_enable_cones failed")
    elif key == "fdyn":
        bs.set_fdyn(v if v is not None else np.zeros(bs.nx))
    elif key == "prob":
        bs.set_bound_constraints(v.x_min, v.x_max, v.u_min, v.u_max)
    elif key == "kw":
        bs.update_settings(**v)
    elif key == "xref":
        bs.set_x_ref(v if v is not None else np.zeros((bs.nx, bs.N)))
    elif key == "uref":
        bs.set_u_ref(v if v is not None else np.zeros((bs.nu, bs.N - 1)))
    elif key == "cache":
        c = v if v is not None else d["cache_own"]
        bs.set_cache_terms(c["Kinf"], c["Pinf"], c["Quu_inv"], c["AmBKt"])
    elif key == "adaptive":
        if v is None:
            bs.set_adaptive_rho(False)
        else:
            bs.set_adaptive_rho(True, v["rho_min"], v["rho_max"], v["clip"])
    elif key == "precision":
        bs.set_precision(v)
    elif key == "strict":
        bs.set_strict_precision(v)
    elif key == "warm":
        bs.set_warm_start(v)
    elif key == "ib":
        bs.set_instance_bounds(*v)
    elif key == "il":
        bs.set_instance_linear(*v)
    elif key == "compaction":
        bs.set_compaction(v)
    else:
        raise KeyError(key)


# ---- the oracle side ----
def _effective(cfg, per, b):
    """the (shared, per) of tests/independence_cases.py::oracle_solver for instance b of a configuration: what is switched off is
    absent, per-instance rows are the instance's own shared rows"""
    prob = cfg["prob"]
    sh, pi = dict(prob=prob), dict(x0=per["x0"])
    if cfg["fdyn"] is not None and np.any(cfg["fdyn"]):
        sh["fdyn"] = cfg["fdyn"]
    if cfg["cones"] is not None:
        en_x, en_u = cfg["cones_on"] if cfg["cones_on"] is not None else (1, 1)
        Acu, qcu, cu, Acx, qcx, cx = cfg["cones"]
        cones = ((Acu, qcu, cu) if en_u else ([], [], [])) + ((Acx, qcx, cx) if en_x else ([], [], []))
        if len(cones[0]) or len(cones[3]):
            sh["cones"] = cones
    lin = cfg["lin"]
    if cfg["il"] is not None:
        Ax, bx, Au, bu = cfg["il"]
        lin = (Ax[:, :, b], bx[:, b], Au[:, :, b], bu[:, b])
    if lin is not None:
        en_x, en_u = cfg["lin_on"] if cfg["lin_on"] is not None else (1, 1)
        nx, nu = prob.nx, prob.nu
        lin = (lin[0] if en_x else np.zeros((0, nx)), lin[1] if en_x else np.zeros(0), lin[2] if en_u else np.zeros((0, nu)), lin[3] if en_u else np.zeros(0))
        if len(lin[1]) or len(lin[3]):
            sh["lin"] = lin
    xr, ur = cfg["xref"], cfg["uref"]
    if xr is not None or ur is not None:
        xr = np.zeros((prob.nx, prob.N)) if xr is None else (xr[:, :, b] if xr.ndim == 3 else xr)
        ur = np.zeros((prob.nu, prob.N - 1)) if ur is None else (ur[:, :, b] if ur.ndim == 3 else ur)
        sh["xref"], sh["uref"] = xr, ur
    if cfg["ib"] is not None:
        for k, a in zip(("ib_xmin", "ib_xmax", "ib_umin", "ib_umax"), cfg["ib"]):
            pi[k] = a
    return sh, pi


def oracle_solver(cfg, per, b, kind="orc64"):
    """a cold, fully configured CpuSolver of instance b under a configuration"""
    sh, pi = _effective(cfg, per, b)
    o = ic.oracle_solver(sh, pi, b, kind, cfg["kw"])
    if cfg["cache"] is not None:
        c = cfg["cache"]
        o.set_cache_terms(c["Kinf"], c["Pinf"], c["Quu_inv"], c["AmBKt"])
    if cfg["adaptive"] is not None:
        a = cfg["adaptive"]
        o.set_sensitivity(*a["sens"])
        o.set_adaptive_rho(1, a["rho_min"], a["rho_max"], a["clip"])
    o.update_settings(**cfg["kw"])      # (set_bound_constraints enables both sides: the flags once more, as the solver's last call)
    return o


_oracles = {}


def oracle_of(route, tr, side, kind="orc64"):
    """the first solve of cols_of(route) under A or A' of a transition: dict like solve_batch's plus, where adaptive rho is on,
    rho / Kinf / Pinf; computed once per configuration and handed out read-only"""
    key = (label(route, tr, side), kind)
    if key not in _oracles:
        cfg = configs(route, tr)[0 if side == "A" else 1]
        _, per = base_cfg(route)
        prob, cols = cfg["prob"], cols_of(route)
        n = len(cols)
        out = dict(x=np.zeros((prob.nx, prob.N, n)), u=np.zeros((prob.nu, prob.N - 1, n)), iter=np.zeros(n, dtype=np.int32),
                   solved=np.zeros(n, dtype=np.int32), res=np.zeros((n, 4)))
        if cfg["adaptive"] is not None:
            out.update(rho=np.zeros(n), Kinf=np.zeros((prob.nu, prob.nx, n)), Pinf=np.zeros((prob.nx, prob.nx, n)))
        for j, b in enumerate(cols):
            o = oracle_solver(cfg, per, int(b), kind)
            o.set_x0(per["x0"][:, b])
            o.solve()
            r = o.get_solution()
            out["x"][:, :, j], out["u"][:, :, j] = r["x"], r["u"]
            out["iter"][j], out["solved"][j], out["res"][j] = r["iter"], r["solved"], r["res"]
            if cfg["adaptive"] is not None:
                ad = o.get_adapted()
                out["rho"][j], out["Kinf"][:, :, j], out["Pinf"][:, :, j] = ad["rho"], ad["Kinf"], ad["Pinf"]
            o.close()
        for a in out.values():
            a.setflags(write=False)
        _oracles[key] = out
    return _oracles[key]


def changed_share(ra, rb):
    """the share of instances on which two oracle runs differ by more than CHANGE, norm-relative, in x or u"""
    from tests.util import nrel_batch
    return float(np.mean(np.maximum(nrel_batch(rb["x"], ra["x"]), nrel_batch(rb["u"], ra["u"])) > CHANGE))
