"""The per-instance families of the device-setup tests (test_families_setup.py on the CPU, test_families_setup_gpu.py on the GPU),
drawn once per shape with fixed seeds, and their caches by the parent's host code (t.host_precompute, t.host_precompute_sweeps),
computed once per session and left unchanged.

  (4,1), (6,3), (12,4)   the base problem (cartpole, rocket, quadrotor) with A perturbed by 2 %, B by 5 %, Q and R scaled in
                         [0.5, 2], rho in [0.5, 3]: the recipe of test_per_instance_families_vs_oracle;
  the grid's corners     (2,1), (3,2), (8,2), (10,3), (12,1): every instance a draw of test_gpu_parity._random_problem.

A set holds 259 instances; the batch-37 case takes instances 100..136 of it and the batch-1 case instance 200, so the host
reference is shared.  Input conditions the seeds were chosen for (checked on the CPU, asserted by the tests): the (4,1) set
holds an instance at the 1000-sweep cap, and every 64 consecutive instances of every set hold at least 8 distinct sweep counts
(the per-instance exit of the kernel is what runs).
"""
import numpy as np

import tinympc_julia_amd as t

MAIN = {(4, 1): ("cartpole", 20, 413), (6, 3): ("rocket", 50, 631), (12, 4): ("quadrotor", 30, 1241)}
CORNERS = {(2, 1): 21, (3, 2): 32, (8, 2): 82, (10, 3): 103, (12, 1): 121}
SHAPES = list(MAIN) + list(CORNERS)
FULL = 259
BATCHES = {1: slice(200, 201), 37: slice(100, 137), 259: slice(0, 259)}
KEYS = ("Kinf", "Pinf", "Quu_inv", "AmBKt")

_FAM, _HOST = {}, {}


def base_problem(shape):
    name, N, _ = MAIN[shape]
    if name == "cartpole":
        return t.problems.cartpole(N, u_bound=0.5)
    return t.problems.rocket(N) if name == "rocket" else t.problems.quadrotor(N)


def perturbed(base, B, seed):
    """B families around `base`: (A, Bm, Q, R, rho), each (.., .., B)"""
    rng = np.random.default_rng(seed)
    nx, nu = base.nx, base.nu
    A = np.repeat(base.A[:, :, None], B, axis=2) * (1.0 + 0.02 * rng.standard_normal((nx, nx, B)))
    Bm = np.repeat(base.B[:, :, None], B, axis=2) * (1.0 + 0.05 * rng.standard_normal((nx, nu, B)))
    Q = np.stack([np.diag(np.diag(base.Q) * rng.uniform(0.5, 2.0, nx)) for _ in range(B)], axis=2)
    R = np.stack([np.diag(np.diag(base.R) * rng.uniform(0.5, 2.0, nu)) for _ in range(B)], axis=2)
    return A, Bm, Q, R, rng.uniform(0.5, 3.0, B)


def families(shape):
    """the 259 families of a shape: (A, Bm, Q, R, rho)"""
    if shape not in _FAM:
        if shape in MAIN:
            _FAM[shape] = perturbed(base_problem(shape), FULL, MAIN[shape][2])
        else:
            from tests.test_gpu_parity import _random_problem
            rng = np.random.default_rng(CORNERS[shape])
            ps = [_random_problem(rng, shape[0], shape[1], 10, bounded=False) for _ in range(FULL)]
            _FAM[shape] = tuple(np.stack([getattr(p, k) for p in ps], axis=2) for k in ("A", "B", "Q", "R")) + (np.array([p.rho for p in ps]),)
    return _FAM[shape]


def take(fam, sl):
    return tuple(np.ascontiguousarray(m[..., sl]) if m.ndim == 1 else np.asfortranarray(m[..., sl]) for m in fam)


def host_reference(shape):
    """the parent's host code on every family of the set: dict(Kinf (nu, nx, 259), ..., sweeps (259,))"""
    if shape not in _HOST:
        A, Bm, Q, R, rho = families(shape)
        cs = [t.host_precompute(A[:, :, b], Bm[:, :, b], Q[:, :, b], R[:, :, b], rho[b]) for b in range(FULL)]
        out = {k: np.stack([c[k] for c in cs], axis=2) for k in KEYS}
        out["sweeps"] = np.array([t.host_precompute_sweeps(A[:, :, b], Bm[:, :, b], Q[:, :, b], R[:, :, b], rho[b]) for b in range(FULL)])
        _HOST[shape] = out
    return _HOST[shape]


def cache_error(got, ref, sl=slice(None)):
    """the worst over the instances of max|got - host| / max|host|, per matrix: dict"""
    out = {}
    for k in KEYS:
        r = ref[k][:, :, sl]
        out[k] = float((np.abs(got[k] - r).max(axis=(0, 1)) / np.abs(r).max(axis=(0, 1))).max())
    return out


def check_input_conditions(shape):
    sw = host_reference(shape)["sweeps"]
    if shape == (4, 1):
        assert (sw == 1000).any(), "the (4,1) set holds no instance at the sweep cap"
    for lo in range(0, FULL - 63):
        assert len(set(sw[lo:lo + 64].tolist())) >= 8, (shape, lo)
