"""CPU tests of the oracle itself (test infrastructure pinned before it is trusted):
the fp64 C restatement must reproduce every golden vector produced by the compiled reference
snapshot to <= 1e-12 (norm-relative), the fp32+fp64-cache model must stay within the fp32 parity
tolerance, and where the reference library itself is present (dev container) it is re-run live.
"""
import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.util import FP64_TOL, cm, golden_names, load_golden, nrel, problem_of

SINGLE = [n for n in golden_names() if n.startswith(("G1_", "G3", "G4"))]
BATCH = [n for n in golden_names() if n.startswith(("G2_", "G6", "G7_"))]
MPC = [n for n in golden_names() if n.startswith("G5")]
TRACE = [n for n in golden_names() if n.startswith("G8")]


def test_golden_inventory():
    """SURVEY.md §8(c) lists G1..G8; all are committed."""
    names = golden_names()
    for prefix in ("G1_", "G2_", "G3a", "G3b", "G3c", "G3d", "G4_", "G5_", "G6_", "G7_", "G8a", "G8b"):
        assert any(n.startswith(prefix) for n in names), prefix


def _mk(oracle, kind, g, prob=None):
    prob = prob or problem_of(g)
    s = oracle.CpuSolver(kind, prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
    s.update_settings(**g["settings"])
    if prob.has_bounds():
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    return s, prob


def _cmp(o, exp, prob, tol):
    assert nrel(o["x"], cm(exp["x"], prob.nx, prob.N)) <= tol
    assert nrel(o["u"], cm(exp["u"], prob.nu, prob.N - 1)) <= tol


@pytest.mark.parametrize("name", SINGLE)
def test_orc64_single(oracle_built, name):
    g = load_golden(name)
    s, prob = _mk(oracle_built, "orc64", g)
    if g["xref"] is not None:
        s.set_x_ref(cm(g["xref"], prob.nx, prob.N))
    if g["uref"] is not None:
        s.set_u_ref(cm(g["uref"], prob.nu, prob.N - 1))
    s.set_x0(g["x0"])
    status = s.solve()
    o = s.get_solution()
    exp = g["expect"]
    assert (status, o["iter"], o["solved"]) == (exp["status"], exp["iter"], exp["solved"])
    _cmp(o, exp, prob, FP64_TOL)
    assert np.allclose(o["res"], exp["res"], rtol=1e-9, atol=1e-13)
    c = s.get_cache()
    for key, (r, cc) in dict(Kinf=(prob.nu, prob.nx), Pinf=(prob.nx, prob.nx), Quu_inv=(prob.nu, prob.nu),
                             AmBKt=(prob.nx, prob.nx)).items():
        assert nrel(c[key], cm(g["cache"][key], r, cc)) <= FP64_TOL, key
    st = s.get_state()
    for key in ("d", "y", "g", "v", "z"):
        ref = np.asarray(g["state_after"][key])
        assert np.abs(st[key].flatten(order="F") - ref).max() <= FP64_TOL * max(1.0, np.abs(ref).max()), key


def test_known_answer_config1(oracle_built):
    """SURVEY.md §8(c) known-answer for examples/cartpole_example_one_solve.jl."""
    g = load_golden("G1_cartpole_one_solve")
    e = g["expect"]
    assert (e["status"], e["iter"]) == (0, 7)
    assert abs(e["u"][0] - 1.17807593) < 5e-9 and abs(e["u"][18] + 0.67943572) < 5e-9
    assert np.allclose(g["cache"]["Kinf"], [-1.8281816031, -2.4111848780, 20.6738188203, 3.3664150316], atol=5e-10)


@pytest.mark.parametrize("name", BATCH)
def test_orc64_batch(oracle_built, name):
    g = load_golden(name)
    prob = problem_of(g)
    B = g["batch"]
    xr = None if g["xref"] is None else cm(g["xref"], prob.nx, prob.N)
    ur = None if g["uref"] is None else cm(g["uref"], prob.nu, prob.N - 1)
    r = oracle_built.solve_batch("orc64", prob, cm(g["x0"], prob.nx, B), xref=xr, uref=ur, nthreads=2,
                                 **{k: g["settings"][k] for k in ("abs_pri_tol", "abs_dua_tol", "max_iter",
                                                                  "check_termination")})
    for b, exp in enumerate(g["expect"]):
        assert (int(r["iter"][b]), int(r["solved"][b])) == (exp["iter"], exp["solved"])
        _cmp(dict(x=r["x"][:, :, b], u=r["u"][:, :, b]), exp, prob, FP64_TOL)


@pytest.mark.parametrize("name", MPC)
def test_orc64_warm_start_sequence(oracle_built, name):
    """Workspace persistence across solves, closed loop x+ = A x + B u0."""
    g = load_golden(name)
    s, prob = _mk(oracle_built, "orc64", g)
    s.set_x0(g["x0"])
    s.set_x_ref(np.zeros((prob.nx, prob.N)))
    s.set_u_ref(np.zeros((prob.nu, prob.N - 1)))
    x = np.array(g["x0"], dtype=np.float64)
    for step in g["steps"]:
        assert np.abs(x - np.array(step["x0"])).max() <= 1e-12
        status = s.solve()
        o = s.get_solution()
        assert (status, o["iter"]) == (step["status"], step["iter"])
        _cmp(o, step, prob, FP64_TOL)
        st = s.get_state()
        for key in ("d", "y", "g", "v", "z"):
            ref = np.asarray(step["state_after"][key])
            assert np.abs(st[key].flatten(order="F") - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max())
        x = prob.A @ x + prob.B @ o["u"][:, 0]
        s.set_x0(x)


@pytest.mark.parametrize("name", TRACE)
def test_orc64_residual_trace(oracle_built, name):
    g = load_golden(name)
    prob = problem_of(g)
    for tr in g["trace"][::7] + [g["trace"][-1]]:
        s = oracle_built.CpuSolver("orc64", prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
        s.update_settings(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=tr["k"], check_termination=1)
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        s.set_x0(g["x0"])
        assert s.solve() == tr["status"]
        o = s.get_solution()
        assert o["iter"] == tr["iter"]
        assert np.allclose(o["res"], tr["res"], rtol=1e-9, atol=1e-13)
        assert np.abs(o["u"][:, 0] - np.array(tr["u0"])).max() <= 1e-12 * max(1.0, np.abs(tr["u0"]).max())


@pytest.mark.parametrize("name", ["G2_cartpole_box_fixed100", "G6_quadrotor_box_fixed100", "G7_rocket_box_fixed100"])
def test_orc32_model_within_fp32_budget(oracle_built, name):
    """fp32 loop + fp64-computed cache (the all-fp32 kernel's arithmetic model): a few 1e-6 on these
    fixtures — and the reason the kernel's default keeps the recurrences in fp64."""
    g = load_golden(name)
    prob = problem_of(g)
    B = g["batch"]
    xr = None if g["xref"] is None else cm(g["xref"], prob.nx, prob.N)
    ur = None if g["uref"] is None else cm(g["uref"], prob.nu, prob.N - 1)
    r = oracle_built.solve_batch("orc32", prob, cm(g["x0"], prob.nx, B), xref=xr, uref=ur,
                                 abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=100)
    for b, exp in enumerate(g["expect"]):
        assert nrel(r["x"][:, :, b], cm(exp["x"], prob.nx, prob.N)) <= 2e-5
        assert nrel(r["u"][:, :, b], cm(exp["u"], prob.nu, prob.N - 1)) <= 2e-5


def test_live_reference_when_present(oracle_built):
    """The compiled reference snapshot (oracle/_ref) against the restatement on inputs no other fixture uses: re-run live
    where the snapshot is built (guards the fixtures against staleness), else its outputs on these inputs as recorded
    in tests/golden/L1_live_reference.json."""
    g = load_golden("L1_live_reference")
    kw = g["settings"]
    for run, (prob, x0) in zip(g["runs"], ((t.problems.cartpole(20, u_bound=0.4), t.problems.cartpole_x0(16, seed=77)),
                                           (t.problems.quadrotor(20), t.problems.quadrotor_x0(8, seed=78)))):
        assert np.array_equal(cm(run["x0"], prob.nx, run["batch"]), x0)
        if oracle_built.have_ref():
            a = oracle_built.solve_batch("ref", prob, x0, **kw)
        else:
            e = run["expect"]
            a = dict(x=np.reshape(e["x"], (prob.nx, prob.N, -1), order="F"), u=np.reshape(e["u"], (prob.nu, prob.N - 1, -1), order="F"),
                     iter=np.asarray(e["iter"]), solved=np.asarray(e["solved"]))
        b = oracle_built.solve_batch("orc64", prob, x0, **kw)
        assert np.array_equal(a["iter"], b["iter"]) and np.array_equal(a["solved"], b["solved"])
        assert np.abs(a["x"] - b["x"]).max() <= 1e-11 and np.abs(a["u"] - b["u"]).max() <= 1e-11


ADAPTIVE = [n for n in golden_names() if n.startswith("G9")]


def _adaptive_solver(oracle, kind, g):
    prob = problem_of(g)
    s, _ = _mk(oracle, kind, g, prob)
    s.set_sensitivity(cm(g["dKinf_drho"], prob.nu, prob.nx), cm(g["dPinf_drho"], prob.nx, prob.nx))
    a = g["adaptive"]
    s.set_adaptive_rho(1, a["rho_min"], a["rho_max"], a["clip"])
    return s, prob


def test_adaptive_inventory():
    """adaptive rho is pinned by reference outputs too (G9a-d)."""
    assert len(ADAPTIVE) == 4


@pytest.mark.parametrize("name", ADAPTIVE)
def test_orc64_adaptive_rho(oracle_built, name):
    """admm.cpp:147-174 + rho_benchmark.cpp restated without the sparse matrices: same rho path, same adapted
    Kinf / Pinf, same solution as the compiled reference, over consecutive solves of one solver (the adapted cache
    persists)."""
    g = load_golden(name)
    prob = problem_of(g)
    x0 = cm(g["x0"], prob.nx, g["batch"])
    for b, seq in enumerate(g["expect"]):
        s, _ = _adaptive_solver(oracle_built, "orc64", g)
        s.set_x0(x0[:, b])
        for exp in seq:
            status = s.solve()
            o = s.get_solution()
            assert (status, o["iter"], o["solved"]) == (exp["status"], exp["iter"], exp["solved"])
            _cmp(o, exp, prob, 1e-10)
            a = s.get_adapted()
            assert abs(a["rho"] - exp["rho"]) <= 1e-10 * exp["rho"]
            assert nrel(a["Kinf"], cm(exp["Kinf"], prob.nu, prob.nx)) <= 1e-10
            assert nrel(a["Pinf"], cm(exp["Pinf"], prob.nx, prob.nx)) <= 1e-10


def test_adaptive_rho_live_reference(oracle_built):
    """The zero-initialised build of the snapshot against the restatement on a fresh seed: re-run live where it is built,
    else its outputs as recorded in tests/golden/L2_live_reference_adaptive.json (with the built-in tables it hands over)."""
    import os
    live = os.path.isfile(oracle_built.REF_ADAPT_LIB)
    g = load_golden("L2_live_reference_adaptive")
    prob = t.problems.quadrotor(30)
    x0 = t.problems.quadrotor_x0(3, seed=11)
    assert np.array_equal(cm(g["x0"], prob.nx, 3), x0)
    st = g["settings"]
    for b in range(3):
        out = []
        sens = None if live else (cm(g["dKinf_drho"], prob.nu, prob.nx), cm(g["dPinf_drho"], prob.nx, prob.nx))
        if not live:
            e = g["expect"][b]
            out.append(dict(iter=e["iter"], rho=e["rho"], x=cm(e["x"], prob.nx, prob.N), u=cm(e["u"], prob.nu, prob.N - 1)))
        for kind in ("refa", "orc64") if live else ("orc64",):
            s = oracle_built.CpuSolver(kind, prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
            s.update_settings(**st)
            s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
            sens = sens or s.get_builtin_sensitivity()
            s.set_sensitivity(*sens)
            s.set_adaptive_rho(1, 1.0, 20.0, True)
            s.set_x0(x0[:, b])
            s.solve()
            o = s.get_solution()
            o.update(s.get_adapted())
            out.append(o)
        assert out[0]["iter"] == out[1]["iter"]
        assert abs(out[0]["rho"] - out[1]["rho"]) <= 1e-10 * out[0]["rho"]
        assert nrel(out[1]["x"], out[0]["x"]) <= 1e-10 and nrel(out[1]["u"], out[0]["u"]) <= 1e-10


L3_RUNS = ["shared_refs", "state_bound", "refs_and_bound", "refs_and_bound_nonsymmetric"]


@pytest.mark.parametrize("label", L3_RUNS)
def test_adaptive_rho_refs_bounds_live_reference(oracle_built, label):
    """Adaptive rho where G9 / L2 do not reach — shared references, a finite state bound on every knot, both, and both with
    a dPinf/drho that is not symmetric (it alone tells Pinf' x from Pinf x in the terminal rows and the reference term) —
    over two consecutive solves of one solver, the second from the plant's next state.  The restatement is held to the
    zero-initialised snapshot's outputs as recorded in tests/golden/L3_live_reference_adaptive_refs_bounds.json, and to
    the snapshot re-run live where it is built: equal iteration counts and exits, rho, x, u and the adapted Kinf / Pinf
    within 1e-10.  This is what lets orc64 arbitrate the matrix-core kernel's adaptive variants (tests/mfma_cases.py)."""
    import os
    g = load_golden("L3_live_reference_adaptive_refs_bounds")
    assert [r["label"] for r in g["runs"]] == L3_RUNS
    run = g["runs"][L3_RUNS.index(label)]
    prob = problem_of(run)
    B, ad = g["batch"], g["adaptive"]
    x0, x1 = cm(g["x0"], prob.nx, B), cm(run["x1"], prob.nx, B)
    dK, dP = cm(g["dKinf_drho"], prob.nu, prob.nx), cm(run["dPinf_drho"], prob.nx, prob.nx)
    assert (np.abs(dP - dP.T).max() > 0.01 * np.abs(dP).max()) == label.endswith("nonsymmetric")
    assert (np.abs(prob.x_max).min() < 1e17) == ("bound" in label) and (run["xref"] is not None) == ("refs" in label)
    kinds = ("orc64", "refa") if os.path.isfile(oracle_built.REF_ADAPT_LIB) else ("orc64",)
    moved = 0
    for b in range(B):
        for kind in kinds:
            s = oracle_built.CpuSolver(kind, prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
            s.update_settings(**g["settings"])
            s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
            s.set_sensitivity(dK, dP)
            s.set_adaptive_rho(1, ad["rho_min"], ad["rho_max"], ad["clip"])
            if run["xref"] is not None:
                s.set_x_ref(cm(run["xref"], prob.nx, prob.N))
                s.set_u_ref(cm(run["uref"], prob.nu, prob.N - 1))
            for k, x in enumerate((x0[:, b], x1[:, b])):
                exp = run["expect"][b][k]
                s.set_x0(x)
                status = s.solve()
                o = s.get_solution()
                assert (status, o["iter"], o["solved"]) == (exp["status"], exp["iter"], exp["solved"]), (kind, b, k)
                _cmp(o, exp, prob, 1e-10)
                a = s.get_adapted()
                assert abs(a["rho"] - exp["rho"]) <= 1e-10 * exp["rho"], (kind, b, k)
                assert nrel(a["Kinf"], cm(exp["Kinf"], prob.nu, prob.nx)) <= 1e-10, (kind, b, k)
                assert nrel(a["Pinf"], cm(exp["Pinf"], prob.nx, prob.nx)) <= 1e-10, (kind, b, k)
                if k == 0 and kind == "orc64":
                    assert np.abs(prob.A @ x + prob.B @ o["u"][:, 0] - x1[:, b]).max() <= 1e-10
            moved += kind == "orc64" and abs(a["rho"] - prob.rho) > 1e-3
            s.close()
    assert moved >= B // 2                                 # the recorded runs do adapt


def test_host_sensitivity_matches_the_recipe():
    """The library's host finite differences (csrc/host_setup.cpp) against the numpy mirror of TinyMPC.jl:301-352
    in tinympc.py; both difference two Riccati fixed points with h = 1e-6, so agreement is to the fixed points'
    own 1e-10 stopping noise over h."""
    for prob in (t.problems.cartpole(20), t.problems.quadrotor(30), t.problems.rocket(50)):
        got = t.host_sensitivity(prob.A, prob.B, prob.Q, prob.R, prob.rho)
        s = t.TinyMPCSolver()
        s.A, s.B, s.Q, s.R, s.rho, s.is_setup = prob.A, prob.B, prob.Q, prob.R, prob.rho, True
        want = t.compute_sensitivity_autograd(s)
        for a, b in zip(got, want):
            assert a.shape == b.shape
            assert np.abs(a - b).max() <= 2e-3 * max(1.0, np.abs(b).max())
        # and they are derivatives: a centred difference with a larger step agrees to first order
        K0 = t.tinympc._solve_lqr(prob.A, prob.B, prob.Q, prob.R, prob.rho - 1e-3)[0]
        K1 = t.tinympc._solve_lqr(prob.A, prob.B, prob.Q, prob.R, prob.rho + 1e-3)[0]
        assert np.abs((K1 - K0) / 2e-3 - got[0]).max() <= 1e-2 * max(1e-3, np.abs(got[0]).max()) + 1e-3
