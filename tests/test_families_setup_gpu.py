"""Per-instance families set up on the device (tinympc_create_families_device, tinympc_set_families).

 1 cache parity          riccati_families_kernel against the parent's host code (t.host_precompute) on EVERY instance: the shapes
                         (4,1), (6,3), (12,4) and the grid's corners (2,1), (3,2), (8,2), (10,3), (12,1), at batches 1, 37 (a ragged
                         last group and wavefront) and 259.  Sweep counts are equal on every instance (fixed seeds: a fact, not a
                         statistic).  The normalised error max|dev - host| / max|host| per matrix, worst over every case and instance,
                         was measured on the first GPU run as CACHE_MEASURED (below); asserted: CACHE_TOL = min(1e-9, 10 x that) —
                         the two sides may differ in FMA contraction only as far as the compiler follows the rule's pragma, and
                         1e-9 is four orders below the 1e-5 solution target the caches feed.  The families and their input
                         conditions (an instance at the 1000-sweep cap; at least 8 distinct sweep counts in every 64 consecutive
                         instances): tests/families_cases.py, asserted here too.
 2 batch independence    one family's cache, bit for bit: alone, at position 0 of 37, 36 of 37, 4 098 of 4 099.
 3 solve parity          the cases of test_per_instance_families_vs_oracle and test_families_with_cones_linear_and_fdyn created
                         with setup="device", through parity_every_instance unchanged (the second covers the fill kernel's Pf /
                         apf / bpf images).
 4 host against device   the same families, 50 fixed iterations: nrel_batch <= 2e-6 (what test_per_instance_families_vs_oracle
                         gives two kernels on equal problems); again at precision 1 within precision1_limit.
 5 setter = fresh        solve F1, set_families(F2), reset, solve == a fresh from_families(F2, setup="device"), bit for bit; from a
                         host-mode solver; the partial forms; without reset the workspace is kept (== a fresh solver given it).
 6 closed loop           stream4<4,1> families, a zero disturbance installed (the own-plant chain): an 8-step mpc_rollout after
                         set_families(F2) == a fresh F2 solver's, bit for bit; the same with an estimator (its predict uses A_b, B_b).
 7 refusals              a single-family solver; one singular instance (named, the solver unchanged); families_setup_mode 1 -> 2.
Every test fails without the feature: from_families takes no `setup` there and the symbols do not exist."""
import numpy as np
import pytest

import tinympc_julia_amd as t
from tests import families_cases as fc
from tests.util import nrel_batch, parity_every_instance, precision1_limit

pytestmark = pytest.mark.gpu

CACHE_MEASURED = 0.0                           # worst normalised error of section 1 on the MI355X: every matrix of every instance equals the host's
CACHE_TOL = min(1e-9, 10.0 * CACHE_MEASURED)
KW = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1)


def _horizon(shape):
    return fc.MAIN[shape][1] if shape in fc.MAIN else 10


# ---------------------------------------------------------------------------------------------------------------------------
# 1. cache parity on every instance
@pytest.mark.parametrize("batch", sorted(fc.BATCHES))
@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_device_cache_equals_host_code(hip_lib, shape, batch):
    fc.check_input_conditions(shape)
    sl = fc.BATCHES[batch]
    ref = fc.host_reference(shape)
    bs = t.BatchSolver.from_families(*fc.take(fc.families(shape), sl), _horizon(shape), setup="device")
    assert bs.families_setup_mode == 2 and bs.kernel_name == "stream4<%d,%d>" % shape
    got = bs.family_cache()
    bs.close()
    want = ref["sweeps"][sl]
    bad = np.nonzero(got["sweeps"] != want)[0]
    assert bad.size == 0, f"sweep counts differ on instances {bad[:8].tolist()}: {got['sweeps'][bad[:8]]} vs {want[bad[:8]]}"
    err = fc.cache_error(got, ref, sl)
    print(f"{shape} batch {batch}: device vs host_precompute {err}; sweeps {want.min()}..{want.max()}, {len(set(want.tolist()))} distinct")
    assert max(err.values()) <= CACHE_TOL, err


def test_family_cache_ranges_and_host_mode(hip_lib):
    """family_cache(first, count) in both modes: the host mode's is the host code's own, a range is the slice of the whole"""
    shape = (6, 3)
    fam, ref = fc.take(fc.families(shape), slice(0, 37)), fc.host_reference(shape)
    for setup in ("host", "device"):
        bs = t.BatchSolver.from_families(*fam, 12, setup=setup)
        assert bs.families_setup_mode == (1 if setup == "host" else 2)
        whole, part = bs.family_cache(), bs.family_cache(first=5, count=9)
        for k in fc.KEYS + ("sweeps",):
            assert np.array_equal(part[k], whole[k][..., 5:14]), (setup, k)
        if setup == "host":
            for k in fc.KEYS + ("sweeps",):
                assert np.array_equal(whole[k], ref[k][..., :37]), k
        with pytest.raises(t.TinyMPCError, match="leaves the batch"):
            bs.family_cache(first=30, count=8)
        bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. batch independence
@pytest.mark.parametrize("shape", [(4, 1), (12, 4)], ids=lambda s: "%dx%d" % s)
def test_cache_is_independent_of_batch_and_position(hip_lib, shape):
    fam = fc.families(shape)
    sw = fc.host_reference(shape)["sweeps"]
    pick = int(np.nonzero(sw == 1000)[0][0]) if shape == (4, 1) else 7       # (the capped instance: it runs longest beside its neighbours)
    one = fc.take(fam, slice(pick, pick + 1))

    def cache_at(batch, pos):
        idx = np.arange(batch) % fc.FULL
        idx[pos] = pick
        arrs = tuple(np.ascontiguousarray(m[..., idx]) if m.ndim == 1 else np.asfortranarray(m[..., idx]) for m in fam)
        bs = t.BatchSolver.from_families(*arrs, 5, setup="device")
        c = bs.family_cache(first=pos, count=1)
        bs.close()
        return c

    bs = t.BatchSolver.from_families(*one, 5, setup="device")
    alone = bs.family_cache()
    bs.close()
    assert alone["sweeps"][0] == sw[pick]
    for batch, pos in ((37, 0), (37, 36), (4099, 4098)):
        c = cache_at(batch, pos)
        for k in fc.KEYS + ("sweeps",):
            assert np.array_equal(c[k], alone[k]), (batch, pos, k)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. solve parity against the oracle
def test_device_families_vs_oracle(hip_lib, oracle_built):
    """test_per_instance_families_vs_oracle's case (cartpole, B = 96, N = 20, min_same = 0.95), the solver set up on the device"""
    from tests.test_gpu_parity import _oracle_loop
    rng = np.random.default_rng(41)
    B, N = 96, 20
    base = t.problems.cartpole(N, u_bound=0.5)
    A = np.repeat(base.A[:, :, None], B, axis=2) * (1.0 + 0.02 * rng.standard_normal((4, 4, B)))
    Bm = np.repeat(base.B[:, :, None], B, axis=2) * (1.0 + 0.05 * rng.standard_normal((4, 1, B)))
    Q = np.zeros((4, 4, B))
    R = np.zeros((1, 1, B))
    for b in range(B):
        Q[:, :, b] = np.diag(np.array([10.0, 1.0, 10.0, 1.0]) * rng.uniform(0.5, 2.0, 4))
        R[:, :, b] = rng.uniform(0.5, 2.0)
    rho = rng.uniform(0.5, 3.0, B)
    x0 = t.problems.cartpole_x0(B, seed=5)

    def mk(b):
        o = oracle_built.CpuSolver("orc64", A[:, :, b], Bm[:, :, b], Q[:, :, b], R[:, :, b], float(rho[b]), N)
        o.update_settings(**KW)
        o.set_bound_constraints(base.x_min, base.x_max, base.u_min, base.u_max)
        return o
    ref = _oracle_loop(mk, x0)
    bs = t.BatchSolver.from_families(A, Bm, Q, R, rho, N, setup="device")
    assert bs.kernel_name == "stream4<4,1>" and bs.families_setup_mode == 2
    bs.update_settings(**KW)
    bs.set_bound_constraints(base.x_min, base.x_max, base.u_min, base.u_max)
    bs.set_x0(x0)
    bs.solve()
    sol, st = bs.get_solution(), bs.get_status()
    parity_every_instance(sol, st, ref, mk, x0, KW, float(rho.max()), min_same=0.95, tag="device-set-up families")
    assert len(set(st["iter"].tolist())) > 3
    bs.close()


def test_device_families_with_cones_linear_and_fdyn(hip_lib, oracle_built):
    """test_families_with_cones_linear_and_fdyn's case ((6,3,12), B = 21): the affine term's images Pf, apf, bpf come from the fill kernel"""
    from tests.test_gpu_parity import _oracle_loop, _random_problem
    rng = np.random.default_rng(77)
    nx, nu, N, B = 6, 3, 12, 21
    base = _random_problem(rng, nx, nu, N, bounded=True)
    A = np.repeat(base.A[:, :, None], B, axis=2) * (1.0 + 0.03 * rng.standard_normal((nx, nx, B)))
    Bm = np.repeat(base.B[:, :, None], B, axis=2) * (1.0 + 0.05 * rng.standard_normal((nx, nu, B)))
    Q = np.stack([np.diag(rng.uniform(0.5, 4.0, nx)) for _ in range(B)], axis=2)
    R = np.stack([np.diag(rng.uniform(0.5, 2.0, nu)) for _ in range(B)], axis=2)
    rho = rng.uniform(0.8, 3.0, B)
    fd = 0.02 * rng.standard_normal(nx)
    Ax, bx, Au, bu = rng.standard_normal((2, nx)), rng.uniform(0.5, 1.5, 2), rng.standard_normal((2, nu)), rng.uniform(0.2, 0.5, 2)
    x0 = np.asfortranarray(rng.uniform(-0.5, 0.5, (nx, B)))
    kw = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=50, check_termination=1)

    def mk(b):
        o = oracle_built.CpuSolver("orc64", A[:, :, b], Bm[:, :, b], Q[:, :, b], R[:, :, b], float(rho[b]), N)
        o.update_settings(**kw)
        o.set_bound_constraints(base.x_min, base.x_max, base.u_min, base.u_max)
        o.set_fdyn(fd)
        o.set_cone_constraints([0], [3], [0.5], [2], [3], [0.7])
        o.set_linear_constraints(Ax, bx, Au, bu)
        return o
    ref = _oracle_loop(mk, x0)
    bs = t.BatchSolver.from_families(A, Bm, Q, R, rho, N, setup="device")
    bs.update_settings(**kw)
    bs.set_bound_constraints(base.x_min, base.x_max, base.u_min, base.u_max)
    bs.set_fdyn(fd)
    bs.set_cone_constraints([0], [3], [0.5], [2], [3], [0.7])
    bs.set_linear_constraints(Ax, bx, Au, bu)
    assert bs.kernel_name == "stream4<6,3>" and bs.families_setup_mode == 2
    bs.set_x0(x0)
    for warm in (True, False):
        bs.set_warm_start(warm)
        bs.reset()
        bs.solve()
        sol, st = bs.get_solution(), bs.get_status()
        parity_every_instance(sol, st, ref, mk, x0, kw, float(rho.max()), tag=f"device families + extensions, warm={warm}")
    bs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# shared by 4 - 7: cartpole families F1 and F2 (two slices of the (4,1) set), bounded inputs
B41 = 40
N41 = 20


def _f(which):
    return fc.take(fc.families((4, 1)), slice(0, B41) if which == 1 else slice(60, 60 + B41))


def _solver(fam, setup, kw=KW):
    base = t.problems.cartpole(N41, u_bound=0.5)
    bs = t.BatchSolver.from_families(*fam, N41, setup=setup)
    bs.update_settings(**kw)
    bs.set_bound_constraints(base.x_min, base.x_max, base.u_min, base.u_max)
    bs.set_x0(t.problems.cartpole_x0(B41, seed=5))
    return bs


def _solve(bs):
    bs.solve()
    sol, st = bs.get_solution(), bs.get_status()
    return dict(x=sol["states"], u=sol["controls"], iter=st["iter"], solved=st["solved"])


def _same(a, b, tag):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{tag}: {k} differs"


# ---------------------------------------------------------------------------------------------------------------------------
# 4. host route against device route
def test_host_route_against_device_route(hip_lib, oracle_built):
    from tests.test_gpu_parity import _oracle_loop
    fixed = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=50, check_termination=1)
    fam = _f(1)
    bh, bd = _solver(fam, "host", fixed), _solver(fam, "device", fixed)
    assert (bh.families_setup_mode, bd.families_setup_mode) == (1, 2)
    rh, rd = _solve(bh), _solve(bd)
    ex, eu = nrel_batch(rd["x"], rh["x"]).max(), nrel_batch(rd["u"], rh["u"]).max()
    print(f"host against device route, precision 0: x {ex:.3e} u {eu:.3e}")
    assert ex <= 2e-6 and eu <= 2e-6
    # precision 1: both re-pack (the device route through the fill kernel's float form); the bar from the oracles alone
    A, Bm, Q, R, rho = fam
    base, x0 = t.problems.cartpole(N41, u_bound=0.5), t.problems.cartpole_x0(B41, seed=5)

    def mk(kind):
        def make(b):
            o = oracle_built.CpuSolver(kind, A[:, :, b], Bm[:, :, b], Q[:, :, b], R[:, :, b], float(rho[b]), N41)
            o.update_settings(**fixed)
            o.set_bound_constraints(base.x_min, base.x_max, base.u_min, base.u_max)
            return o
        return make
    limit, e32, share = precision1_limit(_oracle_loop(mk("orc32"), x0), _oracle_loop(mk("orc64"), x0))
    for s in (bh, bd):
        s.set_precision(1)
        s.reset()
    rh, rd = _solve(bh), _solve(bd)
    ex, eu = nrel_batch(rd["x"], rh["x"]).max(), nrel_batch(rd["u"], rh["u"]).max()
    print(f"host against device route, precision 1: x {ex:.3e} u {eu:.3e} (limit {limit:.3e}: orc32 against orc64 {e32:.3e}, share {share:.2f})")
    assert ex <= limit and eu <= limit
    bh.close(); bd.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a setter on a used solver equals a fresh solver
@pytest.mark.parametrize("start", ["device", "host"])
def test_set_families_then_reset_equals_fresh(hip_lib, start):
    f1, f2 = _f(1), _f(2)
    bs = _solver(f1, start)
    r1 = _solve(bs)
    assert bs.families_setup_mode == (2 if start == "device" else 1)
    bs.set_families(*f2)
    assert bs.families_setup_mode == 2
    bs.reset()
    got = _solve(bs)
    fresh = _solver(f2, "device")
    want = _solve(fresh)
    _same(got, want, f"set_families on a used {start}-mode solver")
    assert not np.array_equal(got["u"], r1["u"])         # (the families really changed the answer)
    for k in fc.KEYS + ("sweeps",):
        assert np.array_equal(bs.family_cache()[k], fresh.family_cache()[k]), k
    bs.close(); fresh.close()


@pytest.mark.parametrize("start", ["device", "host"])
@pytest.mark.parametrize("part", ["rho", "AB", "QR"])
def test_partial_set_families_equals_fresh_of_the_combination(hip_lib, part, start):
    f1, f2 = _f(1), _f(2)
    A, Bm, Q, R, rho = f1
    bs = _solver(f1, start)
    _solve(bs)
    if part == "rho":
        bs.set_families(rho=f2[4])
        comb = (A, Bm, Q, R, f2[4])
    elif part == "AB":
        bs.set_families(A=f2[0], B=f2[1])
        comb = (f2[0], f2[1], Q, R, rho)
    else:
        bs.set_families(Q=f2[2], R=f2[3])
        comb = (A, Bm, f2[2], f2[3], rho)
    assert bs.families_setup_mode == 2
    bs.reset()
    got = _solve(bs)
    fresh = _solver(comb, "device")
    _same(got, _solve(fresh), f"set_families({part}) from {start} mode")
    bs.close(); fresh.close()


def test_set_families_keeps_the_workspace(hip_lib):
    f1, f2 = _f(1), _f(2)
    bs = _solver(f1, "device")
    _solve(bs)
    ws = bs.get_workspace()
    assert np.abs(ws["y"]).max() > 0.0 or np.abs(ws["z"]).max() > 0.0     # (the input bound binds for some instance: a workspace worth keeping)
    bs.set_families(*f2)
    kept = bs.get_workspace()
    for k in ws:
        assert np.array_equal(kept[k], ws[k]), k
    got = _solve(bs)
    fresh = _solver(f2, "device")
    cold = _solve(fresh)
    fresh.set_workspace(ws)
    want = _solve(fresh)
    _same(got, want, "set_families without reset against a fresh solver given the workspace")
    assert not np.array_equal(got["iter"], cold["iter"]) or not np.array_equal(got["u"], cold["u"])   # (the workspace mattered)
    bs.close(); fresh.close()


def test_set_families_keeps_precision_and_fdyn(hip_lib):
    """the re-pack behind set_precision(1) and set_fdyn runs the fill kernel: a used solver equals a fresh one given the same calls"""
    f1, f2 = _f(1), _f(2)
    fd = np.array([0.0, 0.01, 0.0, -0.02])
    bs = _solver(f1, "host")
    bs.set_fdyn(fd)
    bs.set_precision(1)
    _solve(bs)
    bs.set_families(*f2)
    bs.reset()
    got = _solve(bs)
    fresh = _solver(f2, "device")
    fresh.set_precision(1)
    fresh.set_fdyn(fd)
    _same(got, _solve(fresh), "set_families under precision 1 and an affine term")
    bs.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the closed loop follows
@pytest.mark.parametrize("estimator", [False, True])
def test_closed_loop_follows_the_new_families(hip_lib, estimator):
    steps = 8
    f1, f2 = _f(1), _f(2)
    C = np.eye(4)[[0, 2]]
    L = np.array([[0.6, 0.0], [0.8, 0.1], [0.0, 0.6], [0.1, 0.9]])

    def arm(bs):
        bs.set_disturbance(np.zeros((4, steps)))          # (the own-plant chain, no switch)
        if estimator:
            bs.set_estimator(C, L)
        return bs
    bs = arm(_solver(f1, "device"))
    assert bs.kernel_name == "stream4<4,1>"
    first = bs.mpc_rollout(steps)
    bs.set_families(*f2)
    bs.reset()
    bs.set_x0(t.problems.cartpole_x0(B41, seed=5))
    if estimator:
        bs.set_estimator_state(None)                      # (re-armed at x0, as a fresh solver's is)
    got = bs.mpc_rollout(steps)
    fresh = arm(_solver(f2, "device"))
    want = fresh.mpc_rollout(steps)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), f"closed loop after set_families (estimator={estimator}): {k} differs"
    assert not np.array_equal(got["x"], first["x"])
    bs.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. refusals and failure
def test_set_families_refusals(hip_lib):
    base = t.problems.cartpole(N41, u_bound=0.5)
    single = t.BatchSolver(base.A, base.B, base.Q, base.R, base.rho, N41, batch=B41)
    assert single.families_setup_mode == 0
    with pytest.raises(t.TinyMPCError, match="not a per-instance-family solver"):
        single.set_families(*_f(2))
    with pytest.raises(t.TinyMPCError, match="not a per-instance-family solver"):
        single.family_cache()
    single.close()
    bs = _solver(_f(1), "host")
    with pytest.raises(t.TinyMPCError, match="come together"):
        bs.set_families(A=_f(2)[0])
    with pytest.raises(t.TinyMPCError, match="must be"):
        bs.set_families(A=_f(2)[0][:, :, :5], B=_f(2)[1][:, :, :5])
    assert bs.families_setup_mode == 1
    bs.close()


@pytest.mark.parametrize("start", ["host", "device"])
def test_singular_instance_fails_and_leaves_the_solver_as_it_was(hip_lib, start):
    f1 = _f(1)
    A, Bm, Q, R, rho = (m.copy() for m in _f(2))
    Bm[:, :, 5] = 0.0
    R[:, :, 5] = -2.0 * rho[5]                       # R + 2 rho = 0 and B = 0: R1 + B'PB = 0
    bs = _solver(f1, start)
    mode = bs.families_setup_mode
    before = _solve(bs)
    cache = bs.family_cache()
    with pytest.raises(t.TinyMPCError, match=r"singular for instance 5 \(1 of 40 instances"):
        bs.set_families(A, Bm, Q, R, rho)
    assert bs.families_setup_mode == mode
    for k in fc.KEYS + ("sweeps",):
        assert np.array_equal(bs.family_cache()[k], cache[k]), k
    bs.reset()
    _same(_solve(bs), before, "the solve after a refused set_families")
    bs.set_families(rho=_f(2)[4])                    # ... and a good call still goes through, from that state
    assert bs.families_setup_mode == 2
    with pytest.raises(t.TinyMPCError, match="singular for instance 5"):
        t.BatchSolver.from_families(A, Bm, Q, R, rho, N41, setup="device")
    bs.close()
