"""Tours, inputs and cached oracle runs of the workspace hand-over tests: one place, used by the CPU-only conditions
(tests/test_handover_inputs.py, the oracles alone) and by the GPU comparison (tests/test_workspace_handover_gpu.py), so that what
the conditions establish is what the kernels are run on.  Its models are tests/transition_cases.py and
tests/test_lean_ws_gpu.py::_oracle_step / _against_oracle.

The rule under test: a solve warm-starts from the workspace the PREVIOUS solve left, whichever kernel family wrote it.  The
reference's setters leave the workspace alone (admm.cpp:111-115 goes on from d, y, g, v, z as they are), so a route change under a
live workspace — a switch, set_compaction, a bound, rows — must be invisible in the numbers.

A *tour* is one solver with the workspace kept, stepped from the host; reset() is never called.  Each step: (the step's one change
of route), set_x0, solve.  x0 of step k + 1 is the model's own step A x + B u0 (+ f) from step k's first input, rounded to fp32 (what
the device holds, so that the precision-2 tour sees exactly what the oracle sees).  A step is a dict:
    change   what is done before the solve, in words (the table's column)
    env      the complete set of TINYMPC_HIP_* switches in force at the solve (every other one of SWITCHES is unset); where it
             differs from the step before, the solver re-reads them (reload_switches)
    calls    public calls made before the solve, on the solver and — where they change the problem — on the oracle:
             ("compaction", n) set_compaction(n), the solver alone; ("lift",) update_settings with en_state_bound = 0;
             ("rows",) set_linear_constraints with the tour's rows
    kernel   what last_launch_name must report after the solve

The tours (TOURS):
    cartpole   (4,1,20), batch 256 + 37: quad (g1, g2, g4, and g1 chunked by set_compaction(5) on the lean route), lean, stream4, generic;
               every ordered pair of the four; the state bound on row 0 is lifted at step 6, on the lean kernel
    quadrotor  (12,4,30), batch 3 x 16 + 5: mfma, quad g4, stream4, generic; every ordered pair; the state bound on rows 0-2 is
               lifted at step 6, on the matrix-core kernel straight after a quad solve; its launch carries g only when the host flag says so
    rocket     (6,3,10), batch 3 x 16 + 5: mfmat, stream4, generic with the affine term, one cone per side and the box; every
               ordered pair; then two state rows and two input rows are added (stream4) and stream <-> generic repeats
    p2         cartpole N = 17 at precision 2, batch 64 + 6: generic<f64> <-> stream4<4,1;f64>, three solves each way
    adaptive   cartpole (4,1,20), adaptive rho, fixed iterations, batch 64 + 6: quad g4 adaptive, stream4, generic; every pair

The oracle side.  Instance(tour, kind) is one persistent CpuSolver making the tour's calls.  Where the exit it is asked for
differs from its own, the solver is rebuilt, the steps so far are replayed with the exits they took imposed
(CpuSolver.set_forced_exit), and the step is solved with the asked exit imposed: every part of the oracle's state — the cone and
row pairs and the adapted rho, which set_state does not reach — is then the one this history leaves.  No instance is dropped.

oracle_tour(tour, kind) is the oracle's own closed loop on every instance, cached per session and read-only: orc64 on its own
trajectory and exits; orc32 on orc64's x0 sequence with orc64's exits imposed where its own differ."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import tinympc_julia_amd as t
from tests import independence_cases as ic
from tests.util import nrel_batch

SWITCHES = tuple(ic.SWITCHES) + ("TINYMPC_HIP_NO_QUAD_ADP", "TINYMPC_HIP_NO_QUAD_ADP1", "TINYMPC_HIP_NO_MFMA_ADP", "TINYMPC_HIP_NO_STREAM_ADP")
WS_KEYS = ("d", "y", "g", "v", "z")
CHANGE = 1e-3                   # 100 x FP32_TOL: what "another solve" means (tests/transition_cases.py's)
REPLAY_CAP = 0.1                # the GPU test: at most this share of the instances replayed per step (the suite's min_same = 0.9)
ORACLE_CAP = 0.05               # the inputs: orc32 leaves orc64's exit on at most this share per step
FACTOR = 4.0                    # tests/util.py::precision1_limit's


def lean_limit(key):
    """tests/test_lean_ws_gpu.py's limits of a workspace array, of max(|oracle array|_inf, 1e-2)"""
    return 4e-5 if key in ("g", "y") else 2e-5


def f32(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float32).astype(np.float64))


# ---- routes ----
_NQ = dict(ic._NQ)
_GEN = dict(_NQ, TINYMPC_HIP_NO_STREAM="1")
_G = lambda g: {"TINYMPC_HIP_GROUP": str(g)}
_LEAN = {"TINYMPC_HIP_GROUP": "1", "TINYMPC_HIP_LEAN_WS": "1"}
_ADP_S = {"TINYMPC_HIP_NO_QUAD_ADP": "1", "TINYMPC_HIP_NO_MFMA_ADP": "1"}
_ADP_G = dict(_ADP_S, TINYMPC_HIP_NO_STREAM_ADP="1")
_F64 = {"TINYMPC_HIP_STREAM_F64": "1"}


def _st(change, env, kernel, *calls):
    return dict(change=change, env=dict(env), kernel=kernel, calls=tuple(calls))


def _pairs(steps):
    return {(a["kernel"].split("<")[0], b["kernel"].split("<")[0]) for a, b in zip(steps[:-1], steps[1:])}


# every ordered pair of four families a, b, c, d in twelve changes: a b a c d b d c b c a d a
def _cartpole_steps():
    q = lambda g: f"quad<4,1,20,g{g}>"
    L, S, G = "lean<4,1,20>", "stream4<4,1>", "generic"
    return [
        _st("first solve", _G(1), q(1)),
        _st("switches: no quad", _NQ, S),
        _st("switches: quad, 2 lanes", _G(2), q(2)),
        _st("switches: no quad, no stream", _GEN, G),
        _st("switches: lean", _LEAN, L),
        _st("switches: no quad", _NQ, S),
        _st("switches: lean; state bound lifted", _LEAN, L, ("lift",)),
        _st("switches: no quad, no stream", _GEN, G),
        _st("switches: no quad", _NQ, S),
        _st("switches: no quad, no stream", _GEN, G),
        _st("switches: quad, 4 lanes", _G(4), q(4)),
        _st("switches: lean", _LEAN, L),
        _st("set_compaction(5)", _LEAN, q(1), ("compaction", 5)),
    ]


def _quadrotor_steps():
    # the same circuit with a = stream4, b = quad, c = generic, d = mfma: mfma -> quad -> mfma are steps 4, 5, 6, while the state
    # bound binds and inputs sit at their bound; the lift is on mfma straight after a quad solve.  From step 8 on no input is at
    # its bound and no state bound is on: y and g are zero, and the six pairs after it hand over d alone
    M, Q, S, G = "mfma<12,4,30>", "quad<12,4,30,g4>", "stream4<12,4>", "generic"
    return [
        _st("first solve", _NQ, S),
        _st("switches: quad, 4 lanes", _G(4), Q),
        _st("switches: no quad", _NQ, S),
        _st("switches: no quad, no stream", _GEN, G),
        _st("switches: none", {}, M),
        _st("switches: quad, 4 lanes", _G(4), Q),
        _st("switches: none; state bound lifted", {}, M, ("lift",)),
        _st("switches: no quad, no stream", _GEN, G),
        _st("switches: quad, 4 lanes", _G(4), Q),
        _st("switches: no quad, no stream", _GEN, G),
        _st("switches: no quad", _NQ, S),
        _st("switches: none", {}, M),
        _st("switches: no quad", _NQ, S),
    ]


def _rocket_steps():
    T, S, G = "mfmat<6,3,10>", "stream4<6,3>", "generic"
    return [
        _st("first solve", {}, T),
        _st("switches: no quad", _NQ, S),
        _st("switches: none", {}, T),
        _st("switches: no quad, no stream", _GEN, G),
        _st("switches: no quad", _NQ, S),
        _st("switches: no quad, no stream", _GEN, G),
        _st("switches: none", {}, T),
        _st("set_linear_constraints: 2 + 2 rows", {}, S, ("rows",)),
        _st("switches: no stream", {"TINYMPC_HIP_NO_STREAM": "1"}, G),
        _st("switches: none", {}, S),
    ]


def _p2_steps():
    G, S = "generic<f64>", "stream4<4,1;f64>"
    return [_st("first solve", {}, G)] + [_st("switches: stream f64", _F64, S) if k % 2 else _st("switches: none", {}, G) for k in range(1, 7)]


def _adaptive_steps():
    Q, S, G = "quad<4,1,20,g4>", "stream4<4,1>", "generic"
    return [
        _st("first solve", {}, Q),
        _st("switches: no adaptive quad", _ADP_S, S),
        _st("switches: none", {}, Q),
        _st("switches: no adaptive quad, stream", _ADP_G, G),
        _st("switches: no adaptive quad", _ADP_S, S),
        _st("switches: no adaptive quad, stream", _ADP_G, G),
        _st("switches: none", {}, Q),
    ]


# ---- inputs ----
# Chosen on the CPU until tests/test_handover_inputs.py holds (the figures it prints are in profiles/handover_routes.txt).
def _cartpole_tour():
    N, B = 20, 256 + 37
    prob = t.problems.cartpole(N, u_bound=0.5)
    prob.x_min, prob.x_max = prob.x_min.copy(), prob.x_max.copy()
    prob.x_min[0, :], prob.x_max[0, :] = -0.3, 0.3            # tests/test_lean_ws_gpu.py::_cartpole(state_bound=True)
    # tests/test_lean_ws_gpu.py's draw, brought inside the state bound: an x0 outside it leaves knot 0 of the slack unmeetable and
    # the state dual grows by the violation every iteration, for the whole tour (1.05e1 a step at +-0.5: orc32 then leaves orc64 by
    # 1e-4 of g).  Row 0 is scaled into +-0.29; every other instance starts between 0.27 and 0.29 on the side its cart is moving
    # to, at a quarter of the drawn speed: the cart reaches the bound within the horizon and the input bound lets it be held there
    x0 = np.array(t.problems.cartpole_x0(B, seed=41))
    x0[0] *= 0.58
    out = np.arange(B) % 2 == 0
    x0[0, out] = (np.sign(x0[1]) * (0.27 + 0.02 * np.abs(x0[0]) / 0.29))[out]
    x0[1] *= 0.25
    x0[:, np.arange(B) % 4 == 3] *= SETTLED           # (see SETTLED; none of those at the state bound)
    x0 = f32(x0)
    kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=CARTPOLE_MAX_ITER, check_termination=1)
    return dict(id="cartpole", prob=prob, B=B, kw=kw, x0=x0, steps=_cartpole_steps(), precision=0, lift=6, terminated=True,
                families=("quad", "lean", "stream4", "generic"))


def _quadrotor_tour():
    N, B = 30, 3 * 16 + 5
    # tests/mfma_cases.py's draw and state bound (every x0 inside it), changed in three ways so that the loop does not settle: at the
    # family's input bound of 0.5 no input is at its bound after three steps and every instance converges in 4 to 7 iterations once
    # the state bound is lifted.  (1) The input bound is QUADROTOR_UB = 0.3 and a solve has 6 iterations, the middle of the
    # iteration counts.  Not tighter: at 0.1 the inputs ask for many times their bound, the input dual grows to two hundred times
    # the inputs, and u, then a small difference of large terms, leaves what an fp32 workspace resolves — single unsolved instances
    # 1.3e-5 .. 5.1e-5 off on every family alike, orc32 1e-5 .. 7e-5 off; at 0.15 and above the worst u of a run stays below 8e-6, at 0.3
    # below 1e-6.  (2) Every other instance starts between 0.27 and 0.30 on the side it is moving to, in all three position
    # coordinates (the cartpole tour's recipe): it reaches the state bound within the horizon.  (3) Every third instance starts
    # 0.02 to 0.15 times as far out: those converge while the others run to max_iter
    prob = t.problems.quadrotor(N, u_bound=QUADROTOR_UB)
    prob.x_min, prob.x_max = np.full((12, N), -1e17), np.full((12, N), 1e17)
    prob.x_min[:3, :], prob.x_max[:3, :] = -QUADROTOR_XB, QUADROTOR_XB
    x0 = np.array(t.problems.quadrotor_x0(B, seed=4))
    out = np.arange(B) % 2 == 0
    x0[:3, out] = (np.sign(x0[6:9]) * (0.27 + 0.03 * np.abs(x0[:3]) / 0.3))[:, out]
    f = np.where(np.arange(B) % 3 == 0, np.random.default_rng(77).uniform(*QUADROTOR_SMALL, B), 1.0)
    x0 = f32(x0 * f[None, :])
    kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=QUADROTOR_MAX_ITER, check_termination=1)
    return dict(id="quadrotor", prob=prob, B=B, kw=kw, x0=x0, steps=_quadrotor_steps(), precision=0, lift=6, terminated=True,
                families=("mfma", "quad", "stream4", "generic"))


def _rocket_tour():
    N, B = 10, 3 * 16 + 5
    shared, _ = ic.rocket(B, N=N, refs="shared")
    prob = shared["prob"]
    # tests/independence_cases.py::rocket's draw around xinit at 0.4 of its width: every x0 inside the state box (at +-0.5 the
    # first coordinate starts beyond its bound of 5, the state dual grows all tour long and orc32 leaves orc64 by 4e-4 of g)
    rng = np.random.default_rng(1300 + N)
    d = rng.uniform(0.0, ROCKET_SPREAD, B)
    x0 = prob.extra["xinit"][:, None] * (1.0 + d[None, :] * rng.uniform(-1.0, 1.0, (6, B)))
    x0 = f32(np.clip(x0, 0.98 * prob.x_min[:, :1], 0.98 * prob.x_max[:, :1]))
    # 2e-2 on residuals of a problem whose thrust is of the order of 100: at the family's 2e-3 / 1e-3 a solve needs 16 to 40
    # iterations, after which the warm and the cold solve of a step agree to 1e-3 on four instances of five
    kw = dict(abs_pri_tol=2e-2, abs_dua_tol=2e-2, max_iter=ROCKET_MAX_ITER, check_termination=1)
    tour = dict(id="rocket", prob=prob, B=B, kw=kw, x0=x0, steps=_rocket_steps(), precision=0, lift=None, terminated=True,
                fdyn=np.array(shared["fdyn"]), cones=ROCKET_CONES, xref=f32(shared["xref"]), uref=f32(shared["uref"]),
                families=("mfmat", "stream4", "generic"))
    return tour


def _p2_tour():
    N, B = 17, 64 + 6
    prob = t.problems.cartpole(N, u_bound=0.5)
    x0 = np.array(t.problems.cartpole_x0(B, seed=43))
    x0[:, np.arange(B) % 4 == 2] *= SETTLED
    x0 = f32(x0)
    kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=P2_MAX_ITER, check_termination=1)
    return dict(id="p2", prob=prob, B=B, kw=kw, x0=x0, steps=_p2_steps(), precision=2, lift=None, terminated=True,
                families=("generic", "stream4"))


def _adaptive_tour():
    N, B = 20, 64 + 6
    prob = t.problems.cartpole(N, u_bound=0.5)
    x0 = f32(t.problems.cartpole_x0(B, seed=45))
    kw = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=ADAPTIVE_ITERS, check_termination=1)
    dK, dP = t.host_sensitivity(prob.A, prob.B, prob.Q, prob.R, prob.rho)[:2]
    return dict(id="adaptive", prob=prob, B=B, kw=kw, x0=x0, steps=_adaptive_steps(), precision=0, lift=None, terminated=False,
                adaptive=dict(sens=(dK, dP), rho_min=0.1, rho_max=10.0, clip=True), families=("quad", "stream4", "generic"))


# max_iter small enough that an instance far from the origin leaves unsolved in every step of the loop, large enough that one
# close to it converges (both exits of solve() write the workspace differently: tests/test_lean_ws_gpu.py's docstring)
CARTPOLE_MAX_ITER = 30
# every fourth cartpole starts at 0.02 of its draw: states of the order of 1e-2, ten times the tolerance, that move by less than the
# tolerance a step — some of them leave a warm solve at its first check, the exit that hands the loaded v, z, d back untouched
# (admm.cpp:181-193) and the only place where v and z, the previous slack the dual residual is taken against, decide anything
SETTLED = 0.02
QUADROTOR_MAX_ITER = 6
QUADROTOR_XB = 0.31             # rows 0-2: tests/mfma_cases.py::X_BOUND
QUADROTOR_UB = 0.3
QUADROTOR_SMALL = (0.02, 0.15)
ROCKET_MAX_ITER = 20
ROCKET_SPREAD = 0.5             # tests/independence_cases.py::rocket's, clipped into the state box
# the thrust cone at 0.15 instead of the family's 0.25: inside the state box the lateral thrust a landing asks for stays below a
# quarter of the vertical one and the cone touches 0.00 to 0.15 of the instances; at 0.15 it touches 0.5 to 0.8 in every step
ROCKET_CONES = ([0], [3], [0.15], [0], [3], [0.5])
# (coordinate, sign) of the single-coordinate rows: the lateral position and velocity the rocket starts moving outwards in; both
# lateral thrusts on their negative side.  Rows on the descent rate or the vertical thrust bind on every instance at every knot
# (gravity decides both): no instance converges in 40 iterations and the cones no longer touch
ROCKET_STATE_ROWS = ((1, 1.0), (4, 1.0))
ROCKET_INPUT_ROWS = ((0, -1.0), (1, -1.0))
ROCKET_ROW_QUANTILE = 0.97
P2_MAX_ITER = 40
ADAPTIVE_ITERS = 12             # rho adapts every fifth iteration: twice a solve

_BUILD = dict(cartpole=_cartpole_tour, quadrotor=_quadrotor_tour, rocket=_rocket_tour, p2=_p2_tour, adaptive=_adaptive_tour)
TOURS = tuple(_BUILD)
_tours = {}


def tour_of(id):
    if id not in _tours:
        tour = _BUILD[id]()
        tour["x0"].setflags(write=False)
        _tours[id] = tour
    return _tours[id]


def rows_of(tour):
    """(Alin_x (2, nx), blin_x, Alin_u (2, nu), blin_u) of the rocket tour, fp32 values, from orc64's own solve of the step that adds
    them, without them (tests/stream_forms_cases.py::shared_rows' recipe, reduced): single-coordinate rows (ROCKET_STATE_ROWS,
    ROCKET_INPUT_ROWS), each at the batch's ROCKET_ROW_QUANTILE of the largest value the free trajectories reach on that side —
    a state row never below the batch's largest value at knot 0, which no input moves"""
    if "rows" in tour:
        return tour["rows"]
    k = next(i for i, s in enumerate(tour["steps"]) if ("rows",) in s["calls"])
    X, U = free_step(tour, k)
    nx, nu = tour["prob"].nx, tour["prob"].nu
    Ax, Au = np.zeros((2, nx)), np.zeros((2, nu))
    for i, (c, s) in enumerate(ROCKET_STATE_ROWS):
        Ax[i, c] = s
    for i, (c, s) in enumerate(ROCKET_INPUT_ROWS):
        Au[i, c] = s
    bx, bu = np.zeros(2), np.zeros(2)
    for i in range(2):
        p = np.einsum("j,jkb->kb", Ax[i], X)
        bx[i] = max(p[0].max() + 1e-3 * (1.0 + np.abs(p[0]).max()), np.quantile(p[1:].max(axis=0), ROCKET_ROW_QUANTILE))
        q = np.einsum("j,jkb->kb", Au[i], U).max(axis=0)
        bu[i] = np.quantile(q, ROCKET_ROW_QUANTILE)
    tour["rows"] = tuple(f32(a) for a in (Ax, bx, Au, bu))
    return tour["rows"]


def free_step(tour, k):
    """(x (nx, N, B), u (nu, N-1, B)): orc64's step k of the tour WITHOUT the calls of step k (the rocket's: before the rows exist)"""
    run = oracle_tour(tour, "orc64", upto=k)
    xk = plant(tour, run[k - 1]["x0"], run[k - 1]["u"][:, 0, :])

    def one(b):
        inst = Instance(tour)
        inst.history = [(run[j]["x0"][:, b], int(run[j]["iter"][b]), int(run[j]["solved"][b])) for j in range(k)]
        inst.rebuild()
        r = inst._solve(xk[:, b], None)
        inst.close()
        return r
    rs = _pool_map(one, tour["B"])
    return _stack(rs, "x"), _stack(rs, "u")


def plant(tour, x, u0):
    """the model's own step from (nx, B) states and (nu, B) first inputs, as fp32 values"""
    prob = tour["prob"]
    nxt = prob.A @ x + prob.B @ u0
    if "fdyn" in tour:
        nxt = nxt + tour["fdyn"][:, None]
    return f32(nxt)


def settings_at(tour, k):
    """the arguments of update_settings in force at step k (set_bound_constraints enables both sides)"""
    lifted = tour["lift"] is not None and k >= tour["lift"]
    return dict(tour["kw"], en_state_bound=0 if lifted else 1, en_input_bound=1)


# ---- the oracle side ----
class Instance:
    """one instance's persistent oracle on a tour (see the module docstring)"""

    def __init__(self, tour, kind="orc64"):
        self.tour, self.kind, self.history = tour, kind, []
        self.o = self._fresh()

    def _fresh(self):
        from oracle import cpu_oracle
        tour, prob = self.tour, self.tour["prob"]
        o = cpu_oracle.CpuSolver(self.kind, prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
        o.update_settings(**tour["kw"])
        o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        if "fdyn" in tour:
            o.set_fdyn(tour["fdyn"])
        if "cones" in tour:
            o.set_cone_constraints(*tour["cones"])
        if "xref" in tour:
            o.set_x_ref(tour["xref"])
            o.set_u_ref(tour["uref"])
        if "adaptive" in tour:
            a = tour["adaptive"]
            o.set_sensitivity(*a["sens"])
            o.set_adaptive_rho(1, a["rho_min"], a["rho_max"], a["clip"])
        o.update_settings(**settings_at(tour, 0))
        return o

    def _calls(self, k):
        for call in self.tour["steps"][k]["calls"]:
            if call[0] == "lift":
                self.o.update_settings(**settings_at(self.tour, k))
            elif call[0] == "rows":
                self.o.set_linear_constraints(*rows_of(self.tour))

    def _solve(self, x, forced):
        if forced is not None:
            self.o.set_forced_exit(int(forced[0]) if forced[1] else -1)
        self.o.set_x0(x)
        self.o.solve()
        if forced is not None:
            self.o.set_forced_exit(0)
        return self.o.get_solution()

    def rebuild(self, upto=None):
        """a new solver in the state the first `upto` steps of the history leave (default: all of it)"""
        self.o.close()
        self.o = self._fresh()
        for k, (x, it, so) in enumerate(self.history[:upto]):
            self._calls(k)
            r = self._solve(x, (it, so))
            assert (r["iter"], r["solved"]) == (it, so), (self.tour["id"], k, r["iter"], r["solved"], it, so)

    def step(self, x, want=None):
        """step len(history) from state x.  want: the (iter, solved) to take (None: the oracle's own).  Returns (solution,
        workspace, the oracle's own (iter, solved), replayed)"""
        k = len(self.history)
        self._calls(k)
        r = self._solve(x, None)
        own = (int(r["iter"]), int(r["solved"]))
        replayed = want is not None and own != (int(want[0]), int(want[1]))
        if replayed:
            self.rebuild()
            self._calls(k)
            r = self._solve(x, want)
            assert (int(r["iter"]), int(r["solved"])) == (int(want[0]), int(want[1])), (self.tour["id"], k, want, r["iter"], r["solved"])
        self.history.append((np.array(x), int(r["iter"]), int(r["solved"])))
        return r, self.o.get_state(), own, replayed

    def adapted(self):
        return self.o.get_adapted()

    def close(self):
        self.o.close()


def cold(tour, k, x, kind="orc64"):
    """step k's problem solved from a zero workspace: the solution a family that ignored the workspace would give"""
    inst = Instance(tour, kind)
    for j in range(k + 1):
        inst._calls(j)
    r = inst._solve(x, None)
    inst.close()
    return r


def _stack(rs, key):
    return np.stack([r[key] for r in rs], axis=-1)


def _pool_map(fn, n):
    with ThreadPoolExecutor(ic.NTHREADS) as pool:
        return list(pool.map(fn, range(n)))


_runs = {}


def oracle_tour(tour, kind="orc64", upto=None):
    """the oracle's closed loop on every instance: a list over the steps of dict(x0 (nx, B), x, u, iter, solved, own_iter,
    own_solved, ws: {key: (.., B)}, replayed (B,) and, on the adaptive tour, rho, Kinf, Pinf).  orc64 follows its own
    trajectory and exits; another kind is fed orc64's x0 sequence and takes orc64's exits (replayed where its own differ).
    upto: the first `upto` steps only (rows_of needs the loop before the rows exist)"""
    n = len(tour["steps"]) if upto is None else upto
    key = (tour["id"], kind, n)
    if key in _runs:
        return _runs[key]
    B = tour["B"]
    base = None if kind == "orc64" else oracle_tour(tour, "orc64", upto)
    if upto is None and any(("rows",) in s["calls"] for s in tour["steps"]):
        rows_of(tour)           # (before the threads need them)
    insts = [Instance(tour, kind) for _ in range(B)]
    x, out = np.array(tour["x0"]), []
    for k in range(n):
        if base is not None:
            x = base[k]["x0"]

        def one(b):
            want = None if base is None else (base[k]["iter"][b], base[k]["solved"][b])
            r, ws, own, rep = insts[b].step(x[:, b], want)
            ad = insts[b].adapted() if "adaptive" in tour else None
            return r, ws, own, rep, ad
        rs = _pool_map(one, B)
        rec = dict(x0=np.array(x), x=_stack([r[0] for r in rs], "x"), u=_stack([r[0] for r in rs], "u"),
                   iter=np.array([r[0]["iter"] for r in rs]), solved=np.array([r[0]["solved"] for r in rs]),
                   own_iter=np.array([r[2][0] for r in rs]), own_solved=np.array([r[2][1] for r in rs]),
                   replayed=np.array([r[3] for r in rs], dtype=bool), ws={key_: _stack([r[1] for r in rs], key_) for key_ in WS_KEYS})
        if "adaptive" in tour:
            rec.update(rho=np.array([r[4]["rho"] for r in rs]), Kinf=_stack([r[4] for r in rs], "Kinf"), Pinf=_stack([r[4] for r in rs], "Pinf"))
        for a in rec.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        for a in rec["ws"].values():
            a.setflags(write=False)
        out.append(rec)
        x = plant(tour, x, rec["u"][:, 0, :])
    for i in insts:
        i.close()
    _runs[key] = out
    return out


def ws_error(ws, ref):
    """{key: (B,) error of a workspace array against the oracle's, of max(|oracle array|_inf, 1e-2) per instance}"""
    out = {}
    for key in WS_KEYS:
        scale = np.maximum(np.abs(ref[key]).max(axis=(0, 1)), 1e-2)
        out[key] = np.abs(np.asarray(ws[key]) - ref[key]).max(axis=(0, 1)) / scale
    return out


_limits = {}


def derived_limits(tour):
    """{key: (limit, e32)}: the workspace limit of a family that does not meet the lean kernel's, from the reference alone —
    e32 the worst orc32-vs-orc64 difference of that array over the tour's steps and instances (orc32 on orc64's x0 sequence and
    exits), limit = max(lean limit, FACTOR x e32)"""
    if tour["id"] not in _limits:
        r64, r32 = oracle_tour(tour, "orc64"), oracle_tour(tour, "orc32")
        e32 = {key: 0.0 for key in WS_KEYS}
        for a, b in zip(r32, r64):
            for key, e in ws_error(a["ws"], b["ws"]).items():
                e32[key] = max(e32[key], float(e.max()))
        _limits[tour["id"]] = {key: (max(lean_limit(key), FACTOR * e32[key]), e32[key]) for key in WS_KEYS}
    return _limits[tour["id"]]


# Which (tour, family) pairs take the derived limit instead of the lean kernel's, and on which arrays: those a first recorded
# run on an MI355X (every bar at the lean kernel's limits, the figures printed before they are asserted) showed above them.  The
# limit itself never comes from that run: derived_limits is the reference's own spread.
#   cartpole, g: 7.6e-5 (stream4, step 1), 8.0e-5 (quad g2, step 2), 4.3e-5 (generic, step 3) against 4e-5, on instances that run to
#     max_iter with a state dual of the order of the scale's floor of 1e-2: a clamped knot's g takes over the absolute error of x
#     (2.4e-6 .. 3.8e-6 of 0.3 in those steps, within FP32_TOL), whichever family runs.  The lean kernel stayed below (2.9e-5).
#   quadrotor: none (every array below a tenth of its limit on all four families).
#   rocket, y: 5.3e-5 (stream4, step 4) against 4e-5, on a thrust of the order of 100 whose dual is of the order of 1: orc32 itself
#     is 4e-4 off there.
DERIVED = {("cartpole", "stream4"): ("g",), ("cartpole", "quad"): ("g",), ("cartpole", "generic"): ("g",),
           ("rocket", "stream4"): ("y",)}


def ws_limit(tour, family, key):
    """(the limit in force for an array a family wrote on a tour, whether it is the derived one)"""
    if key in DERIVED.get((tour["id"], family), ()):
        return derived_limits(tour)[key][0], True
    return lean_limit(key), False


# ---- the input conditions' figures ----
def warm_share(tour, k):
    """share of the instances on which orc64's step k from the kept workspace differs from its cold solve of the same x0 by more
    than CHANGE"""
    run = oracle_tour(tour)
    rec = run[k]
    rs = _pool_map(lambda b: cold(tour, k, rec["x0"][:, b]), tour["B"])
    dx, du = nrel_batch(_stack(rs, "x"), rec["x"]), nrel_batch(_stack(rs, "u"), rec["u"])
    return float(np.mean(np.maximum(dx, du) > CHANGE))


def zeroed_share(tour, k, key):
    """share of the instances on which zeroing workspace array `key` before orc64's step k changes that step's solution by more
    than CHANGE, or its exit"""
    run = oracle_tour(tour)
    rec = run[k]

    def one(b):
        inst = Instance(tour)
        inst.history = [(run[j]["x0"][:, b], int(run[j]["iter"][b]), int(run[j]["solved"][b])) for j in range(k)]
        inst.rebuild()
        ws = inst.o.get_state()
        ws[key] = np.zeros_like(ws[key])
        inst.o.set_state(ws["d"], ws["y"], ws["g"], ws["v"], ws["z"])
        inst._calls(k)
        r = inst._solve(rec["x0"][:, b], None)
        inst.close()
        return r
    rs = _pool_map(one, tour["B"])
    dx, du = nrel_batch(_stack(rs, "x"), rec["x"]), nrel_batch(_stack(rs, "u"), rec["u"])
    exit_moved = (np.array([r["iter"] for r in rs]) != rec["iter"]) | (np.array([r["solved"] for r in rs]) != rec["solved"])
    return float(np.mean((np.maximum(dx, du) > CHANGE) | exit_moved))


def cone_share(tour, rec):
    """share of the instances whose solution touches a cone at some knot (tests/stream_forms_cases.py::binding_share's test, both sides)"""
    Acu, qcu, cu, Acx, qcx, cx = tour["cones"]
    hit = np.zeros(tour["B"], dtype=bool)
    for arr, starts, dims, mus in ((rec["u"], Acu, qcu, cu), (rec["x"][:, 1:, :], Acx, qcx, cx)):
        for s, d, mu in zip(starts, dims, mus):
            head, axis = np.sqrt((arr[s:s + d - 1] ** 2).sum(axis=0)), arr[s + d - 1]
            hit |= ((head >= 0.999 * mu * axis) & (head > 1e-6)).any(axis=0)
    return float(hit.mean())


def row_share(tour, rec):
    """share of the instances whose solution sits at a linear row (to the solve's tolerance) at some knot after the first"""
    Ax, bx, Au, bu = rows_of(tour)
    tol = tour["kw"]["abs_pri_tol"]
    hit = (np.einsum("ij,jkb->ikb", Au, rec["u"]) >= bu[:, None, None] - tol).any(axis=(0, 1))
    hit |= (np.einsum("ij,jkb->ikb", Ax, rec["x"][:, 1:, :]) >= bx[:, None, None] - tol).any(axis=(0, 1))
    return float(hit.mean())


def state_bound_share(tour, rec):
    """share of the instances with a bounded state at its bound at some knot after the first"""
    prob = tour["prob"]
    x = rec["x"][:, 1:, :]
    scale = np.abs(rec["x"]).max(axis=(1, 2), keepdims=True)
    return float(((x >= prob.x_max[:, 1:, None] - 1e-9 * scale) | (x <= prob.x_min[:, 1:, None] + 1e-9 * scale)).any(axis=(0, 1)).mean())


def input_bound_share(tour, rec):
    prob, u = tour["prob"], rec["u"]
    scale = np.abs(u).max()
    return float(((u >= prob.u_max[:, :, None] - 1e-9 * scale) | (u <= prob.u_min[:, :, None] + 1e-9 * scale)).any(axis=(0, 1)).mean())
