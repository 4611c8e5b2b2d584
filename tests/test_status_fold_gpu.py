"""The status fold of every kernel family (csrc/admm_params.h).  The one-shot lean kernels fold with one record per workgroup
(fold_status_records); every other family, and the lean kernel's workspace-keeping forms, with the accumulator (fold_status).
Both share the accumulator block and the ticket, so their launches may follow each other on one solver.  Every case runs with
the records on (the default), off (TINYMPC_HIP_FOLD_SLOTS=0: the accumulator path for every workgroup) and with three records
only (TINYMPC_HIP_FOLD_SLOTS=3: in a lean launch of more than three workgroups both paths run, and the last arriver has to
combine records and accumulator); for the families without records the three settings must not matter.

The invariant is exact and needs no reference: after a solve the device status block, read as bench.py's exchange step reads
it (tests/test_gpu_parity.py::test_rccl_status_allreduce_one_rank), holds in words 0..3 the bitwise maximum over the batch of
the per-instance residuals and in word 4 the number of unsolved instances.  The shapes are the smallest at which a path can go
wrong: one workgroup, a ragged wavefront, two and five workgroups; instances that finish at different times (tolerance 1e-3
with the iteration limit at the oracle's median exit); solves back to back on one solver (a record or an accumulator word left
by an earlier launch would show the earlier, larger maxima); grids that shrink from chunk to chunk (records beyond the grid
are older launches'); a persistent grid whose tile counter shares the accumulator block."""
import os

import numpy as np
import pytest

import tinympc_julia_amd as t

pytestmark = pytest.mark.gpu

SLOTS = [None, "0", "3"]
SLOT_IDS = ["slots_default", "slots_0", "slots_3"]
ROCKET_CONES = ([0], [3], [0.25], [0], [3], [0.5])          # inputs first: tests/test_mfmat_gpu.py
NT = min(16, len(os.sched_getaffinity(0)))


def _slots(monkeypatch, slots):
    if slots is None:
        monkeypatch.delenv("TINYMPC_HIP_FOLD_SLOTS", raising=False)
    else:
        monkeypatch.setenv("TINYMPC_HIP_FOLD_SLOTS", slots)


def _block(bs):
    """the device status block as uint32[8] (the launch must have finished)"""
    import torch
    from tinympc_julia_amd import sharding
    g = sharding.device_tensor(bs.device_buffers()["gstat"], (8,), torch.int32, torch.device("cuda", 0))
    torch.cuda.synchronize()
    return g.cpu().numpy().view(np.uint32).copy()


def _check(bs, tag):
    st = bs.get_status()                                        # (waits for the launch)
    w = _block(bs)
    want = st["residuals"].max(axis=0).astype(np.float32)
    got = w[:4].copy().view(np.float32)
    unsolved = int((st["solved"] == 0).sum())
    print(f"{tag}: block {got} unsolved {int(w[4])} | per-instance {want} unsolved {unsolved}")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tag, got, want)
    assert int(w[4]) == unsolved, (tag, int(w[4]), unsolved)
    return st


def _cartpole(N, B, kw, seed=81, warm=False):
    prob, x0 = t.problems.cartpole(N, u_bound=0.5), t.problems.cartpole_x0(B, seed=seed)
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    bs.update_settings(**kw)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(warm)
    bs.set_x0(x0)
    return bs, prob, x0


_median_exit = {}


def _median(oracle_built, B):
    """the oracle's median exit of the batch at tolerance 1e-3 (computed once per batch)"""
    if B not in _median_exit:
        prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(B, seed=81)
        full = oracle_built.solve_batch("orc64", prob, x0, nthreads=NT, abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100,
                                        check_termination=1)
        _median_exit[B] = int(np.median(full["iter"]))
    return _median_exit[B]


@pytest.mark.parametrize("slots", SLOTS, ids=SLOT_IDS)
@pytest.mark.parametrize("B", [1, 63, 257, 1025])
def test_lean(hip_lib, oracle_built, monkeypatch, B, slots):
    """one workgroup, a ragged wavefront, 2 and 5 workgroups; fixed iterations, and workgroups that finish at different times"""
    monkeypatch.setenv("TINYMPC_HIP_GROUP", "1")
    _slots(monkeypatch, slots)
    bs, _, _ = _cartpole(20, B, dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=20, check_termination=1))
    bs.solve()
    assert bs.last_launch_name == "lean<4,1,20>"
    st = _check(bs, f"lean fixed B={B}")
    assert not st["solved"].any()
    bs.close()
    bs, _, _ = _cartpole(20, B, dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=_median(oracle_built, B), check_termination=1))
    bs.solve()
    assert bs.last_launch_name == "lean<4,1,20>"
    st = _check(bs, f"lean tol B={B}")
    if B > 1:
        assert 0 < st["solved"].sum() < B, "the iteration limit was meant to split the batch"
    bs.close()


@pytest.mark.parametrize("slots", SLOTS, ids=SLOT_IDS)
def test_lean_back_to_back(hip_lib, monkeypatch, slots):
    """three launches with nothing waited for in between: the block behind the last one is the last solve's"""
    monkeypatch.setenv("TINYMPC_HIP_GROUP", "1")
    _slots(monkeypatch, slots)
    B = 1025
    bs, _, x0 = _cartpole(20, B, dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=20, check_termination=1))
    bs.solve()
    _check(bs, "back to back, alone")
    bs.set_x0(x0)
    bs.solve_async()
    bs.set_x0(0.1 * x0)
    bs.solve_async()
    bs.set_x0(0.1 * x0)
    bs.solve_async()
    assert bs.last_launch_name == "lean<4,1,20>"
    _check(bs, "back to back, third")
    bs.close()


@pytest.mark.parametrize("slots", SLOTS, ids=SLOT_IDS)
def test_shrinking_grids(hip_lib, monkeypatch, slots):
    """chunks of five iterations with the unconverged instances compacted in between"""
    monkeypatch.setenv("TINYMPC_HIP_GROUP", "1")
    _slots(monkeypatch, slots)
    bs, _, _ = _cartpole(20, 1025, dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1))
    bs.set_compaction(5)
    bs.solve()
    st = _check(bs, "compaction")
    assert st["iter"].min() < st["iter"].max()
    bs.close()


@pytest.mark.parametrize("slots", SLOTS, ids=SLOT_IDS)
def test_record_and_accumulator_launches_alternate(hip_lib, monkeypatch, slots):
    """one solver, launches of the lean kernel (records) and of the quad kernel (accumulator: the chunked solve) in turn: both
    hand the accumulator block and the ticket back zeroed"""
    monkeypatch.setenv("TINYMPC_HIP_GROUP", "1")
    _slots(monkeypatch, slots)
    bs, _, _ = _cartpole(20, 1025, dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=30, check_termination=1))
    for k, chunk in enumerate((0, 10, 0, 10, 0)):
        bs.set_compaction(chunk)
        bs.solve()
        assert bs.last_launch_name == ("quad<4,1,20,g1>" if chunk else "lean<4,1,20>"), bs.last_launch_name
        _check(bs, f"alternating, solve {k} ({bs.last_launch_name})")
    bs.close()


@pytest.mark.parametrize("slots", SLOTS, ids=SLOT_IDS)
@pytest.mark.parametrize("G", [4, 1])
def test_quad(hip_lib, monkeypatch, G, slots):
    monkeypatch.setenv("TINYMPC_HIP_GROUP", str(G))
    monkeypatch.setenv("TINYMPC_HIP_NO_LEAN", "1")
    _slots(monkeypatch, slots)
    bs, _, _ = _cartpole(10, 130, dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=12, check_termination=1), warm=True)
    bs.solve()
    assert bs.last_launch_name == f"quad<4,1,10,g{G}>", bs.last_launch_name
    _check(bs, f"quad g{G}")
    bs.close()


@pytest.mark.parametrize("slots", SLOTS, ids=SLOT_IDS)
@pytest.mark.parametrize("setting", ["fixed", "tol"])
def test_mfma(hip_lib, monkeypatch, setting, slots):
    """the matrix-core kernel of the quadrotor: fixed iterations, and tolerance-terminated (the refill arm)"""
    _slots(monkeypatch, slots)
    prob, x0 = t.problems.quadrotor(10), t.problems.quadrotor_x0(80, seed=82)
    kw = (dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=20, check_termination=1) if setting == "fixed" else
          dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=40, check_termination=1))
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=80)
    bs.update_settings(**kw)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(False)
    bs.set_x0(x0)
    bs.solve()
    assert bs.last_launch_name == "mfma<12,4,10>", bs.last_launch_name
    _check(bs, f"mfma {setting}")
    bs.close()


@pytest.mark.parametrize("slots", SLOTS, ids=SLOT_IDS)
def test_mfmat_twice(hip_lib, monkeypatch, slots):
    """a persistent grid, its tile counter in the accumulator block: the second solve finds it handed back as zero"""
    _slots(monkeypatch, slots)
    B = 200
    prob, x0 = t.problems.rocket(10), t.problems.rocket_x0(B, seed=2)
    xr, ur = t.problems.rocket_refs(10)
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    bs.update_settings(abs_pri_tol=2e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_fdyn(prob.fdyn)
    bs.set_cone_constraints(*ROCKET_CONES)
    bs.set_x_ref(xr)
    bs.set_u_ref(ur)
    bs.set_warm_start(False)
    seen = []
    for k in range(2):
        bs.set_x0(x0)
        bs.solve()
        assert bs.kernel_name == "mfmat<6,3,10>", bs.kernel_name
        st = _check(bs, f"mfmat solve {k}")
        seen.append((st["iter"].copy(), bs.get_solution()["controls"].copy()))
    assert np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1])
    bs.close()


@pytest.mark.parametrize("slots", SLOTS, ids=SLOT_IDS)
def test_stream(hip_lib, monkeypatch, slots):
    monkeypatch.setenv("TINYMPC_HIP_NO_QUAD", "1")
    _slots(monkeypatch, slots)
    bs, _, _ = _cartpole(17, 70, dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=30, check_termination=1), warm=True)
    bs.solve()
    assert bs.kernel_name == "stream4<4,1>" and bs.last_launch_name == "stream4<4,1>", (bs.kernel_name, bs.last_launch_name)
    _check(bs, "stream")
    bs.close()
