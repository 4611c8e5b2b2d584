"""A kept workspace handed from one kernel family to another (tests/handover_cases.py has the tours and the oracle side;
tests/test_handover_inputs.py the conditions that keep this file from passing vacuously).

Every family keeps the warm-start workspace d, y, g, v, z between solves — with cones or rows their slack / dual pairs, under
adaptive rho the per-instance rho / Kinf / Pinf — and each writes it in its own way: mfmat parks the slack of the iteration before
a converged exit and saves d = Quu_inv t, the lean kernel works in scaled coordinates, mfma carries g only when the host flag
g_maybe_nonzero says so, the cone and row pairs are allocated lazily, precision 2 keeps an fp64 block of its own.  The suite holds
each family to the oracle on continued solves of that family and every setter to a fresh solver across a reset(); here one solver
tours the families of its shape with the workspace live: before each solve exactly one thing moves the route (the switches re-read,
or a public setter), reset() is never called, x0 is the model's step from the solver's own previous solve, and
last_launch_name is asserted at every solve.

Every step is compared with persistent per-instance orc64 solvers making the same calls; where the GPU's exit differs from the
oracle's own, the oracle's history is replayed with the GPU's exits imposed (handover_cases.Instance) — no instance is dropped, at
most 0.1 of them may be replayed per step.  Bars: the solution at FP32_TOL; the five arrays of get_workspace() at
tests/test_lean_ws_gpu.py's limits (2e-5; 4e-5 for g and y; of max(|oracle array|_inf, 1e-2)) unless handover_cases.DERIVED names the
(tour, family, array), which then takes max(that, 4 x orc32's worst distance from orc64 on the tour) — a figure of the reference
alone; precision 2 at 1e-6 with exact exits; adaptive rho at tests/test_gpu_parity.py::test_adaptive_rho_vs_reference_golden's (rho
within 1e-5 relative, adapted Kinf / Pinf at FP32_TOL) with get_adaptive_state() compared at every step.  The rocket's cone and
row pairs are not exported: an error in them shows in the next step's solution.

Each step prints "HO <tour> | <step> | <change> | <launch before> -> <launch> | x .. u .. | <array> <error>/<bar> .. | replayed .."
before anything is asserted (profiles/handover_routes.txt holds a run's table)."""
import numpy as np
import pytest

import tinympc_julia_amd as t
from tests import handover_cases as hc
from tests.util import FP32_TOL, nrel_batch

pytestmark = pytest.mark.gpu

P2_TOL = 1e-6


def _switches(monkeypatch, env):
    for name in hc.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)


def _call(bs, tour, k, call):
    if call[0] == "compaction":
        bs.set_compaction(call[1])
    elif call[0] == "lift":
        bs.update_settings(**hc.settings_at(tour, k))
    elif call[0] == "rows":
        bs.set_linear_constraints(*hc.rows_of(tour))
    else:
        raise KeyError(call)


def solver_at(tour, upto=0):
    """a solver configured as the tour's is before the solve of step `upto` (the switches are the caller's)"""
    prob = tour["prob"]
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=tour["B"])
    bs.update_settings(**tour["kw"])
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if "fdyn" in tour:
        bs.set_fdyn(tour["fdyn"])
    if "cones" in tour:
        bs.set_cone_constraints(*tour["cones"])
    if "xref" in tour:
        bs.set_x_ref(tour["xref"])
        bs.set_u_ref(tour["uref"])
    if "adaptive" in tour:
        a = tour["adaptive"]
        bs.set_sensitivity(*a["sens"])
        bs.set_adaptive_rho(True, a["rho_min"], a["rho_max"], a["clip"])
    if tour["precision"]:
        bs.set_precision(tour["precision"])
    bs.set_warm_start(True)
    bs.update_settings(**hc.settings_at(tour, 0))
    for k in range(1, upto + 1):
        for call in tour["steps"][k]["calls"]:
            _call(bs, tour, k, call)
    return bs


def _record(bs, tour, x):
    sol, st = bs.get_solution(), bs.get_status()
    rec = dict(x0=np.array(x), states=sol["states"], controls=sol["controls"], iter=st["iter"], solved=st["solved"],
               residuals=st["residuals"], ws=bs.get_workspace(), name=bs.last_launch_name)
    if "adaptive" in tour:
        rec["adapt"] = bs.get_adaptive_state()
    return rec


_RUNS = {}


def run_tour(monkeypatch, id):
    """the tour on the GPU, once per session: a list of records, one per step"""
    if id in _RUNS:
        return _RUNS[id]
    tour = hc.tour_of(id)
    steps = tour["steps"]
    _switches(monkeypatch, steps[0]["env"])
    bs = solver_at(tour)
    x, out = np.array(tour["x0"]), []
    for k, step in enumerate(steps):
        if k and step["env"] != steps[k - 1]["env"]:
            _switches(monkeypatch, step["env"])
            bs.reload_switches()
        for call in step["calls"] if k else ():
            _call(bs, tour, k, call)
        bs.set_x0(x)
        bs.solve()
        assert bs.last_launch_name == step["kernel"], f"{id} step {k} ({step['change']}): launched {bs.last_launch_name}, the tour has {step['kernel']}"
        out.append(_record(bs, tour, x))
        x = hc.plant(tour, x, out[-1]["controls"][:, 0, :])
    bs.close()
    _RUNS[id] = out
    return out


def against_oracle(tour, run):
    """every step of a GPU run against persistent oracles on every instance.  Prints the table, returns the failures"""
    B, n = tour["B"], len(run)
    p2 = tour["precision"] == 2

    def one(b):
        inst = hc.Instance(tour)
        rows = []
        for k, rec in enumerate(run):
            r, ws, own, rep = inst.step(rec["x0"][:, b], (rec["iter"][b], rec["solved"][b]))
            row = dict(x=r["x"], u=r["u"], ws=ws, rep=rep, res=r["res"])
            if "adaptive" in tour:
                row["adapt"] = inst.adapted()
            rows.append(row)
        inst.close()
        return rows
    per = hc._pool_map(one, B)
    failures = []
    for k, rec in enumerate(run):
        step = tour["steps"][k]
        family = step["kernel"].split("<")[0]
        ref = {key: hc._stack([p[k] for p in per], key) for key in ("x", "u")}
        ref_ws = {key: hc._stack([p[k]["ws"] for p in per], key) for key in hc.WS_KEYS}
        rep = np.array([p[k]["rep"] for p in per])
        ex, eu = nrel_batch(rec["states"], ref["x"]), nrel_batch(rec["controls"], ref["u"])
        ew = hc.ws_error(rec["ws"], ref_ws)
        tol = P2_TOL if p2 else FP32_TOL
        cells = []
        for key in hc.WS_KEYS:
            lim, derived = (P2_TOL, False) if p2 else hc.ws_limit(tour, family, key)
            cells.append(f"{key} {ew[key].max():.1e}/{lim:.0e}{'*' if derived else ''}")
            if ew[key].max() > lim:
                b = int(np.argmax(ew[key]))
                failures.append(f"step {k} ({run[k - 1]['name'] if k else '-'} -> {rec['name']}): {key} of instance {b} off by {ew[key][b]:.2e} (limit {lim:.1e}; iter {rec['iter'][b]}, solved {rec['solved'][b]})")
        line = (f"HO {tour['id']} | {k} | {step['change']} | {run[k - 1]['name'] if k else '-'} -> {rec['name']} | x {ex.max():.1e} u {eu.max():.1e} | "
                + " ".join(cells) + f" | replayed {rep.mean():.3f} | solved {rec['solved'].mean():.2f} iterations {rec['iter'].min()}..{rec['iter'].max()}")
        if "adaptive" in tour:
            rho = np.array([p[k]["adapt"]["rho"] for p in per])
            K, P = hc._stack([p[k]["adapt"] for p in per], "Kinf"), hc._stack([p[k]["adapt"] for p in per], "Pinf")
            er = (np.abs(rec["adapt"]["rho"] - rho) / rho).max()
            ek, ep = nrel_batch(rec["adapt"]["Kinf"], K).max(), nrel_batch(rec["adapt"]["Pinf"], P).max()
            line += f" | rho {er:.1e} Kinf {ek:.1e} Pinf {ep:.1e} (rho {rho.min():.3f}..{rho.max():.3f})"
            if er > 1e-5 or ek > FP32_TOL or ep > FP32_TOL:
                failures.append(f"step {k} ({rec['name']}): adapted state off by rho {er:.2e}, Kinf {ek:.2e}, Pinf {ep:.2e}")
        print(line)
        if ex.max() > tol or eu.max() > tol:
            b = int(np.argmax(np.maximum(ex, eu)))
            failures.append(f"step {k} ({run[k - 1]['name'] if k else '-'} -> {rec['name']}): instance {b} off by x {ex[b]:.2e}, u {eu[b]:.2e} (limit {tol:.0e}; iter {rec['iter'][b]}, solved {rec['solved'][b]})")
        if p2 or not tour["terminated"]:
            if rep.any():
                failures.append(f"step {k} ({rec['name']}): {int(rep.sum())} exits differ from orc64's own")
        elif rep.mean() > hc.REPLAY_CAP:
            failures.append(f"step {k} ({rec['name']}): {rep.mean():.3f} of the instances replayed (cap {hc.REPLAY_CAP})")
    return failures


def _limits_line(tour):
    lim = hc.derived_limits(tour)
    used = {fam: keys for (tid, fam), keys in hc.DERIVED.items() if tid == tour["id"]}
    print(f"HO {tour['id']} | derived limits (max(lean limit, {hc.FACTOR:g} x orc32's worst distance)): "
          + ", ".join(f"{k} {v[0]:.2e} from {v[1]:.2e}" for k, v in lim.items()) + f" | in force (*) for {used if used else 'no family'}")


@pytest.mark.parametrize("id", hc.TOURS)
def test_tour_against_the_oracle(hip_lib, oracle_built, monkeypatch, id):
    """the five tours.  What a first run at the lean kernel's limits everywhere showed is in handover_cases.DERIVED's comment and in
    DESIGN.md section 10, "Workspace hand-over".

    Measured on an MI355X (profiles/handover_routes.txt): every step inside every bar — worst x 3.8e-6 and u 2.7e-7 (cartpole),
    2.2e-7 and 9.5e-7 (quadrotor, every workspace array below a tenth of its limit; g is exactly zero on both sides after the lift),
    5.6e-8 and 3.1e-7 (rocket), 5.7e-8 at precision 2 with the workspace within 6e-14, rho within 4.9e-7 and the adapted Kinf /
    Pinf within 2.7e-8; no exit replayed but one of the rocket's 53 at step 6.  With the quadrotor's input bound at 0.1 instead of
    0.3 the same tour misses FP32_TOL on u (1.3e-5 .. 5.1e-5, single saturated unsolved instances, every family alike): an input
    dual two hundred times the inputs, held in fp32 — the operating point, not a hand-over (handover_cases._quadrotor_tour)."""
    tour = hc.tour_of(id)
    run = run_tour(monkeypatch, id)
    if tour["precision"] == 0:
        _limits_line(tour)
    failures = against_oracle(tour, run)
    assert not failures, f"{id}:\n" + "\n".join(failures)


def _equal(got, want, tag):
    bad = []
    for key in ("states", "controls", "iter", "solved", "residuals"):
        if not np.array_equal(got[key], want[key]):
            d = np.asarray(got[key] != want[key])
            n = int(np.sum(np.any(d.reshape(-1, d.shape[-1]), axis=0))) if key in ("states", "controls") else int(np.sum(np.any(d.reshape(d.shape[0], -1), axis=1)))
            bad.append(f"{key} of {n} instance(s)")
    for key in hc.WS_KEYS:
        if not np.array_equal(got["ws"][key], want["ws"][key]):
            d = got["ws"][key] != want["ws"][key]
            bad.append(f"workspace {key} of {int(np.sum(np.any(d, axis=(0, 1))))} instance(s)")
    if got["name"] != want["name"]:
        bad.append(f"launched {got['name']}, not {want['name']}")
    assert not bad, f"{tag}: " + "; ".join(bad)


# the steps whose workspace goes through get_workspace / set_workspace into a fresh solver: on each box-only tour the step that lifts
# the state bound (the fresh solver never saw the bound enabled: g_maybe_nonzero is what set_workspace says, state_bounds_active
# false from its first launch) and one more — the chunked solve out of the lean kernel's workspace; mfma after the stream kernel
THROUGH = [("cartpole", 6), ("cartpole", 12), ("quadrotor", 6), ("quadrotor", 11)]


@pytest.mark.parametrize("id,k", THROUGH, ids=[f"{i}-{k}" for i, k in THROUGH])
def test_through_the_public_workspace_calls(hip_lib, oracle_built, monkeypatch, id, k):
    """get_workspace() of step k - 1 given to a fresh solver on step k's family with set_workspace, solved from the same x0: bit for
    bit the touring solver's step k (the fp32 workspace survives the round trip through doubles exactly).  What the kernels wrote
    is then all that crosses: not g_maybe_nonzero, state_bounds_active, lean_knot_bounds or any other thing the host remembers"""
    tour = hc.tour_of(id)
    run = run_tour(monkeypatch, id)
    step = tour["steps"][k]
    _switches(monkeypatch, step["env"])
    bs = solver_at(tour, upto=k)
    bs.set_workspace(run[k - 1]["ws"])
    bs.set_x0(run[k]["x0"])
    bs.solve()
    got = _record(bs, tour, run[k]["x0"])
    bs.close()
    print(f"HO {id} | step {k} through get_workspace / set_workspace | {run[k - 1]['name']} -> {got['name']}")
    _equal(got, run[k], f"{id} step {k}: a fresh solver given the workspace of step {k - 1} differs from the touring solver")


P2_ENVS = [("generic", {}), ("stream", dict(hc._F64))]
P2_SEQUENCES = [(0, (2,)), (2, (0,)), (0, (2, 0, 2))]


@pytest.mark.parametrize("tag,env", P2_ENVS, ids=[e[0] for e in P2_ENVS])
@pytest.mark.parametrize("start,seq", P2_SEQUENCES, ids=["0_2", "2_0", "0_2_0_2"])
def test_set_precision_restarts_the_workspace_cold(hip_lib, monkeypatch, tag, env, start, seq):
    """include/tinympc_hip.h: "Switching to or from precision 2 restarts the workspace cold".  A kept-workspace solver that has
    solved twice receives set_precision and solves from a given x0, after every change of a sequence — with no reset() here: the
    library's own is what the comparison sees, and in 0 -> 2 -> 0 -> 2 it has a used fp64 block and used fp32 arrays to clear.
    Required each time, with np.array_equal: a fresh solver's first solve at that precision — solution, status, workspace"""
    tour = hc.tour_of("p2")
    prob, x0 = tour["prob"], tour["x0"]
    _switches(monkeypatch, env)

    def make(precision):
        bs = solver_at(dict(tour, precision=0))
        if precision:
            bs.set_precision(precision)
        return bs
    used = make(start)
    x = np.array(x0)
    for _ in range(2):
        used.set_x0(x)
        used.solve()
        x = hc.plant(tour, x, used.get_solution()["controls"][:, 0, :])
    assert np.abs(used.get_workspace()["y"]).max() > 0.0
    names = [used.last_launch_name]
    for n, p in enumerate(seq):         # after EACH change a solve from a given x0 (another one each time: what the solve before it
        used.set_precision(p)           # left in either block is what the library's reset has to clear)
        given = hc.f32((0.5 + 0.1 * n) * np.array(x0)[:, ::-1])
        used.set_x0(given)
        used.solve()
        got = _record(used, tour, given)
        names.append(got["name"])
        fresh = make(p)
        fresh.set_x0(given)
        fresh.solve()
        want = _record(fresh, tour, given)
        fresh.close()
        assert ("f64" in got["name"]) == (p == 2), got["name"]
        assert np.abs(got["ws"]["y"]).max() > 0.0
        _equal(got, want, f"set_precision {start} -> {seq[:n + 1]} on a used solver ({tag}) differs from a fresh solver's first solve")
    used.close()
    print(f"HO set_precision | {tag} | {start} -> {' -> '.join(str(p) for p in seq)} | {' -> '.join(names)}")
