"""The headline form's packed slack / dual update (csrc/admm_lean.hip.h: PK) on the GPU.

Every instance against the fp64 oracle at FP32_TOL (tests/util.parity_every_instance), fixed iterations, one lane per
instance, B = 193 (three wavefronts, the last ragged): the built-in cartpole kernels at N = 5 (4 knots: pairs only), N = 10
(9 knots: pairs and a single) and N = 20, and — specialised at the first solve — the random (3, 2, N) family of
tests/test_lean_epilogue_gpu.py at N = 7 and N = 8 (two input rows; an even and an odd number of knots).  A shape without a
built-in kernel reaches the lean kernel from 20 480 instances up only (Solver::pack: lean_jit; below that the specialised
four-lanes-per-instance unit takes it whatever TINYMPC_HIP_GROUP says), so that family runs at B = 20 480 + 193: the same
ragged tail behind 80 full workgroups, still one wavefront per SIMD.

Packed against scalar, bit for bit: the same 100 sweeps once with tolerances 0 (the PK kernel) and once with tolerances
1e-30 (the tolerance-terminated kernel: scalar; nothing converges at 1e-30 short of a bit-exact fixed point, where a
stopped instance and an iterating one hold the same values)."""
import os

import numpy as np
import pytest

import tinympc_julia_amd as t
from tests.util import FP32_TOL, parity_every_instance

pytestmark = pytest.mark.gpu

B = 193
NT = min(16, len(os.sched_getaffinity(0)))


def _solve(prob, x0, kw):
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=x0.shape[1])
    bs.update_settings(**kw)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(False)
    bs.set_x0(x0)
    status = bs.solve()
    out = dict(name=bs.last_launch_name, status=status, sol=bs.get_solution(), st=bs.get_status())
    bs.close()
    return out


def _against_oracle(oracle_built, prob, x0, kw, out, tag):
    ref = oracle_built.solve_batch("orc64", prob, x0, nthreads=NT, **kw)

    def make(b=None):
        o = oracle_built.CpuSolver("orc64", prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N)
        o.update_settings(**kw)
        o.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        return o
    parity_every_instance(out["sol"], out["st"], ref, make, x0, kw, prob.rho, tol=FP32_TOL, min_same=1.0, tag=tag)


@pytest.mark.parametrize("N", [5, 10, 20])
def test_builtin_horizons(hip_lib, oracle_built, monkeypatch, N):
    monkeypatch.setenv("TINYMPC_HIP_GROUP", "1")
    kw = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=60, check_termination=1)
    prob, x0 = t.problems.cartpole(N, u_bound=0.5), t.problems.cartpole_x0(B, seed=91)
    out = _solve(prob, x0, kw)
    assert out["name"] == f"lean<4,1,{N}>", out["name"]
    assert np.all(out["st"]["iter"] == 60) and not out["st"]["solved"].any()
    _against_oracle(oracle_built, prob, x0, kw, out, f"cartpole N={N}")


@pytest.fixture
def jit_on(monkeypatch, tmp_path_factory):
    monkeypatch.delenv("TINYMPC_HIP_NO_JIT", raising=False)
    cache = os.environ.get("TINYMPC_TEST_JIT_CACHE") or str(tmp_path_factory.getbasetemp() / "lean_pk_jit_cache")
    os.makedirs(cache, exist_ok=True)
    monkeypatch.setenv("TINYMPC_HIP_CACHE", os.path.abspath(cache))


@pytest.mark.parametrize("N", [7, 8])
def test_two_input_rows(hip_lib, oracle_built, jit_on, N):
    nx, nu = 3, 2
    rng = np.random.default_rng(17)
    A = np.eye(nx) + 0.2 * rng.standard_normal((nx, nx)) / np.sqrt(nx)
    A *= 0.97 / np.abs(np.linalg.eigvals(A)).max()
    prob = t.problems.Problem("rand", A, 0.5 * rng.standard_normal((nx, nu)), np.diag(rng.uniform(0.5, 5.0, nx)),
                              np.diag(rng.uniform(0.5, 3.0, nu)), float(rng.uniform(0.5, 2.0)), N)
    prob.x_min, prob.x_max = np.full((nx, N), -1e17), np.full((nx, N), 1e17)
    prob.u_min, prob.u_max = np.full((nu, N - 1), -0.4), np.full((nu, N - 1), 0.4)
    x0 = np.asfortranarray(rng.uniform(-0.5, 0.5, (nx, 20480 + B)))
    kw = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=60, check_termination=10)
    out = _solve(prob, x0, kw)
    assert out["name"] == f"lean<{nx},{nu},{N}>", out["name"]
    _against_oracle(oracle_built, prob, x0, kw, out, f"(3,2,{N})")


def test_packed_equals_scalar_bit_for_bit(hip_lib, monkeypatch):
    monkeypatch.setenv("TINYMPC_HIP_GROUP", "1")
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(B, seed=92)
    packed = _solve(prob, x0, dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=100, check_termination=1))
    scalar = _solve(prob, x0, dict(abs_pri_tol=1e-30, abs_dua_tol=1e-30, max_iter=100, check_termination=1))
    assert packed["name"] == "lean<4,1,20>" and scalar["name"] == "lean<4,1,20>"
    print("iterations of the tolerance-terminated solve:", np.unique(scalar["st"]["iter"]))
    assert np.array_equal(packed["sol"]["states"], scalar["sol"]["states"])
    assert np.array_equal(packed["sol"]["controls"], scalar["sol"]["controls"])
