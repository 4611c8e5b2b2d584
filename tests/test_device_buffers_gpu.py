"""Who owns the solver's GPU memory (csrc/devbuf.h): every device allocation of the library goes through one counted pair of
functions, and the hook tmpc_device_bytes_live reports the bytes that are live.  Held here: destroying a solver returns all
of them, whatever optional buffer it has used; a re-batch, a repeated setter and a refused setter leave nothing behind.

Every assertion is on a DIFFERENCE of the counter, so a solver another test left alive does not matter (garbage is collected
first, so that none is freed in between).  Inputs: tests/independence_cases.py's builders, cartpole (4, 1) and rocket (6, 3)
at N = 10, batches 70 and 96.  Specialisation at run time is off (TINYMPC_HIP_NO_JIT): nothing here compiles."""
import ctypes
import gc

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests import independence_cases as ic

pytestmark = pytest.mark.gpu
N, STEPS = 10, 3
KW = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=20, check_termination=1)


@pytest.fixture
def live(hip_lib, monkeypatch):
    """the counter, read through the library itself like the other hooks"""
    monkeypatch.setenv("TINYMPC_HIP_NO_JIT", "1")
    lib = ctypes.CDLL(t.LIB_PATH)
    lib.tmpc_device_bytes_live.restype = ctypes.c_longlong
    lib.tmpc_device_bytes_live.argtypes = []
    gc.collect()
    return lambda: int(lib.tmpc_device_bytes_live())


def _solver(shared, per, precision=0):
    prob, B = shared["prob"], per["x0"].shape[1]
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B, device=0)
    if precision:
        bs.set_precision(precision)
    bs.update_settings(**KW)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_x0(per["x0"])
    return bs


def _instance_bounds(prob, B, per_knot=True):
    rep = (lambda a: np.asfortranarray(np.repeat(a[:, :, None], B, axis=2))) if per_knot else \
        (lambda a: np.asfortranarray(np.repeat(a[:, :1], B, axis=1)))
    return [rep(np.asarray(a, dtype=np.float64)) * s for a, s in
            ((prob.x_min, 1.0), (prob.x_max, 1.0), (prob.u_min, 0.9), (prob.u_max, 0.9))]


def _instance_rows(shared, B):
    Ax, bx, Au, bu = shared["lin"]
    scale = np.linspace(1.0, 1.5, B)
    return (np.repeat(Ax[:, :, None], B, axis=2), bx[:, None] * scale, np.repeat(Au[:, :, None], B, axis=2), bu[:, None] * scale)


def _loop_inputs(prob, x0):
    """a per-instance plant, disturbance and trajectory, noise factors and an estimator for a loop of STEPS"""
    nx, nu, B = prob.nx, prob.nu, x0.shape[1]
    rng = np.random.default_rng(7)
    scale = np.abs(x0).max(axis=1) + 1e-3
    C = np.eye(nx)[: nx // 2]
    return dict(plant=(np.asfortranarray(prob.A[:, :, None] * (1.0 + 0.01 * rng.standard_normal((nx, nx, B)))),
                       np.asfortranarray(np.repeat(prob.B[:, :, None], B, axis=2)), np.zeros((nx, B), order="F")),
                w=np.asfortranarray(1e-3 * scale[:, None, None] * rng.standard_normal((nx, STEPS, B))),
                traj=(np.asfortranarray(np.repeat(x0[:, None, :], N + STEPS, axis=1)), np.zeros((nu, N + STEPS, B), order="F")),
                sigma=1e-3 * scale, est=(C, 0.5 * C.T))


def _use_everything(bs, shared, per):
    """every optional buffer of a fixed-rho solver, a solve after each group, one closed loop at the end"""
    prob, x0 = shared["prob"], per["x0"]
    B = x0.shape[1]
    bs.solve()                                                   # shared bounds (set by _solver)
    bs.set_instance_bounds(*_instance_bounds(prob, B))           # per instance and knot
    bs.solve()
    if "lin" in shared:
        bs.set_instance_linear(*_instance_rows(shared, B))
        bs.solve()
    if "cones" in shared:
        bs.set_cone_constraints(*shared["cones"])
        bs.solve()
    if "lin" in shared:
        bs.set_linear_constraints(*shared["lin"])                # (shared rows replace the per-instance ones)
        bs.solve()
    if "fdyn" in shared:
        bs.set_fdyn(shared["fdyn"])
        bs.solve()
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)   # (per-instance bounds have no closed loop)
    rng = np.random.default_rng(3)
    bs.set_x_ref(np.asfortranarray(0.01 * rng.standard_normal((prob.nx, N, B))))
    bs.set_u_ref(np.asfortranarray(0.01 * rng.standard_normal((prob.nu, N - 1, B))))
    bs.solve()
    bs.set_ref_sequence(0.01 * rng.standard_normal((prob.nx, N, STEPS)), 0.01 * rng.standard_normal((prob.nu, N - 1, STEPS)))
    bs.solve()
    lp = _loop_inputs(prob, x0)
    bs.set_ref_trajectory(*lp["traj"])
    bs.solve()
    bs.set_plant(*lp["plant"])
    bs.set_disturbance(lp["w"])
    bs.set_process_noise(lp["sigma"], seed=1)
    bs.set_measurement_noise(lp["sigma"], seed=2)
    bs.set_estimator(*lp["est"])
    bs.set_rollout_metrics(True)
    bs.set_compaction(5)
    bs.solve()
    bs.set_compaction(0)
    bs.set_profiling(True)
    bs.solve()
    pinned = np.zeros((prob.nx, B), dtype=np.float32, order="F")
    bs.pin_host(pinned)                                          # (left pinned: the solver unregisters it when it goes)
    bs.solve()
    bs.mpc_rollout(STEPS)
    bs.get_rollout_summary()
    bs.get_noise(0, 0, STEPS)
    return pinned


# ---- 1. destroy returns everything ----
@pytest.mark.parametrize("name", ["rocket", "cartpole", "cartpole_precision2", "cartpole_adaptive", "families"])
def test_destroy_returns_everything(live, name):
    before = live()
    if name == "rocket":
        shared, per = ic.rocket(70, N=N, refs="none", lin=True)
        bs = _solver(shared, per)
        keep = _use_everything(bs, shared, per)
    elif name == "cartpole":
        shared, per = ic.cartpole(96, N=N)
        bs = _solver(shared, per)
        keep = _use_everything(bs, shared, per)
    elif name == "cartpole_precision2":                          # the generic kernel's fp64-state form: the fp64 workspace block
        shared, per = ic.cartpole(70, N=N)
        bs = _solver(shared, per, precision=2)
        bs.solve()
        bs.set_instance_bounds(*_instance_bounds(shared["prob"], 70))
        bs.solve()
        keep = bs.get_workspace()
    elif name == "cartpole_adaptive":                            # (per-instance inputs refuse adaptive rho: a solver of its own)
        shared, per = ic.cartpole(96, N=N, adaptive=True)
        bs = _solver(shared, per)
        bs.set_sensitivity(*shared["adaptive"]["sens"])
        bs.set_adaptive_rho(True, 0.1, 10.0, True)
        bs.solve()
        bs.solve()
        keep = bs.get_adaptive_state()
    else:
        shared, per = ic.cartpole_families(70, N=N)
        prob = shared["prob"]
        bs = t.BatchSolver.from_families(per["fam_A"], per["fam_B"], per["fam_Q"], per["fam_R"], per["fam_rho"], N, device=0)
        bs.update_settings(**KW)
        bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        bs.set_x0(per["x0"])
        bs.solve()
        bs.set_disturbance(np.zeros((prob.nx, STEPS)))           # (an own-plant solver: the chain, with every instance's A_b, B_b as its plant)
        keep = bs.mpc_rollout(STEPS)
    assert live() > before
    bs.close()
    assert live() == before, name
    del keep


# ---- 2. a re-batch does not accumulate ----
def test_rebatch_does_not_accumulate(live):
    shared, per = ic.rocket(96, N=N, refs="none", lin=True)
    prob, x0 = shared["prob"], per["x0"]
    t.cleanup()                                                  # (a global solver an earlier test left: setup would replace it)
    before = live()
    s = t.TinyMPCSolver()
    t.setup(s, prob.A, prob.B, None, prob.Q, prob.R, prob.rho, prob.nx, prob.nu, N, batch=70, **KW)
    t.set_bound_constraints(s, prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    t.set_cone_constraints(s, *shared["cones"])
    t.set_linear_constraints(s, *shared["lin"])
    at = {}
    for batch in (70, 96, 70, 96, 70):
        if batch != 70 or at:
            t.set_batch_size(s, batch)
        t.set_x0(s, np.asfortranarray(x0[:, :batch]))
        t.solve(s)
        at.setdefault(batch, []).append(live())
    assert at[70][1] == at[70][2] and at[96][0] == at[96][1], at
    t.cleanup()
    assert live() == before


# ---- 3. repeating a setter does not accumulate ----
def test_repeated_setters_do_not_accumulate(live):
    shared, per = ic.rocket(70, N=N, refs="none", lin=True)
    prob, x0 = shared["prob"], per["x0"]
    B = x0.shape[1]
    bs = _solver(shared, per)
    lp = _loop_inputs(prob, x0)
    rng = np.random.default_rng(5)
    xr, ur = np.asfortranarray(0.01 * rng.standard_normal((prob.nx, N, B))), np.asfortranarray(0.01 * rng.standard_normal((prob.nu, N - 1, B)))
    shared_bounds = lambda: bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    solve, loop = bs.solve, lambda: bs.mpc_rollout(STEPS)
    # (setter, what makes its upload happen); in an order in which every step is accepted
    steps = [
        ("bounds", shared_bounds, solve),
        ("instance_bounds", lambda: bs.set_instance_bounds(*_instance_bounds(prob, B, per_knot=False)), solve),
        ("instance_bounds_per_knot", lambda: bs.set_instance_bounds(*_instance_bounds(prob, B)), solve),
        ("instance_rows", lambda: bs.set_instance_linear(*_instance_rows(shared, B)), solve),
        ("rows", lambda: bs.set_linear_constraints(*shared["lin"]), solve),
        ("cones", lambda: bs.set_cone_constraints(*shared["cones"]), solve),
        ("fdyn", lambda: bs.set_fdyn(shared["fdyn"]), solve),
        ("bounds_again", shared_bounds, solve),
        ("references", lambda: (bs.set_x_ref(xr), bs.set_u_ref(ur)), solve),
        ("cache_terms", lambda: bs.set_cache_terms(**bs.get_cache_terms()), solve),
        ("plant", lambda: bs.set_plant(*lp["plant"]), loop),
        ("disturbance", lambda: bs.set_disturbance(lp["w"]), loop),
        ("noise", lambda: (bs.set_process_noise(lp["sigma"], seed=1), bs.set_measurement_noise(lp["sigma"], seed=2)), loop),
        ("estimator", lambda: bs.set_estimator(*lp["est"]), loop),
        ("trajectory", lambda: bs.set_ref_trajectory(*lp["traj"]), loop),
        ("metrics", lambda: bs.set_rollout_metrics(True), loop),
    ]
    for name, setter, use in steps:
        seen = []
        for _ in range(3):
            setter()
            use()
            seen.append(live())
        assert seen[2] == seen[1], (name, seen)
    bs.close()
    # the sensitivity tables are uploaded only under adaptive rho
    shared, per = ic.cartpole(96, N=N, adaptive=True)
    bs = _solver(shared, per)
    bs.set_adaptive_rho(True, 0.1, 10.0, True)
    seen = []
    for _ in range(3):
        bs.set_sensitivity(*shared["adaptive"]["sens"])
        bs.solve()
        seen.append(live())
    assert seen[2] == seen[1], ("sensitivity", seen)
    bs.close()


# ---- 4. a refusal keeps the books ----
def test_refusals_keep_the_books(live):
    shared, per = ic.cartpole(96, N=N, adaptive=True)
    prob = shared["prob"]
    bs = _solver(shared, per)
    bs.set_adaptive_rho(True, 0.1, 10.0, True)
    bs.solve()
    base = live()
    with pytest.raises(t.TinyMPCError):
        bs.set_instance_bounds(*_instance_bounds(prob, 96))
    assert live() == base
    bs.close()
    shared, per = ic.cartpole(70, N=N)
    prob = shared["prob"]
    bs = _solver(shared, per)
    bs.solve()
    base = live()
    with pytest.raises(t.TinyMPCError):
        bs.set_estimator(np.ones((prob.nx + 1, prob.nx)), np.ones((prob.nx, prob.nx + 1)))      # ny > nx
    assert live() == base
    with pytest.raises(t.TinyMPCError):
        bs.set_instance_linear(np.ones((9, prob.nx, 70)), np.ones((9, 70)), None, None)        # nine rows
    assert live() == base
    with pytest.raises(t.TinyMPCError):
        bs.set_rollout_metrics(True, qw=-np.ones(prob.nx))
    assert live() == base
    bs.solve()
    assert live() == base
    bs.close()


# ---- 5. the sharded handle ----
def test_sharded_returns_everything(live):
    import torch
    devices = [0, 1] if torch.cuda.device_count() >= 2 else [0]      # (tests/test_sharded_capi.py's: two real devices where there are two)
    shared, per = ic.cartpole(70, N=N)
    prob = shared["prob"]
    before = live()
    sh = t.ShardedBatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=70, devices=devices)
    sh.update_settings(**KW)
    sh.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    sh.set_x0(per["x0"])
    sh.solve()
    assert live() > before
    sh.close()
    assert live() == before
