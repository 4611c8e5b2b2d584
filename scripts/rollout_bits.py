"""Every chained closed-loop route once, batch 70 and 5 steps, everything mpc_rollout leaves written into ONE .npz — to compare two
builds of the library byte for byte (a refactor of csrc/solver.hip's chain: run it in both trees, then --compare).  No workload of
its own: the cases are the builders of tests/test_plant_loop_gpu.py, test_noise_loop_gpu.py, test_ref_trajectory_gpu.py,
test_stream_loop_gpu.py and test_rollout_routes_gpu.py (the latter's batch-130 start states cut to 70).

  rollout_bits.py --out FILE.npz      run the cases with the library of THIS tree; arrays are named case/array
  rollout_bits.py --compare A B       per case and array: shape, bytes, equal or NOT EQUAL; exit status 1 on any difference

Per rollout (r0, r1 where a case runs two): the x, u, iter, solved logs and the measured log where there is one; after the last:
x0 as left on the device, the last solution, the status arrays, the workspace, the two status words, and the last launch's
kernel with the number of solve launches of the last rollout."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, STEPS = 70, 5
SWITCHES = ("TINYMPC_HIP_LEAN_WS", "TINYMPC_HIP_LEAN_LOOP", "TINYMPC_HIP_STREAM_MPC", "TINYMPC_HIP_STREAM_LOOP", "TINYMPC_HIP_NO_STREAM",
            "TINYMPC_HIP_GROUP", "TINYMPC_HIP_STREAM_F64", "TINYMPC_HIP_MFMA_ONESHOT_ONLY", "TINYMPC_HIP_NO_MFMAT", "TINYMPC_HIP_NOISE_SPLIT")
MPC = {"TINYMPC_HIP_STREAM_MPC": "1"}


def _env(*sets):
    """the switches a solver reads when it is made: all cleared, then the given ones; nothing specialised at run time, as in the
    suite (tests/conftest.py), whose kernels the cases name"""
    for name in SWITCHES:
        os.environ.pop(name, None)
    os.environ["TINYMPC_HIP_NO_JIT"] = "1"
    for s in sets:
        os.environ.update(s)


def _record(bs, logs):
    from tests.test_stream_loop_gpu import _collect, _launches
    out = {}
    for i, log in enumerate(logs):
        for key in ("x", "u", "iter", "solved", "y"):
            if key in log:
                out[f"r{i}_{key}"] = np.ascontiguousarray(log[key])
    got = _collect(bs, logs[-1])
    out["x0"] = got["x0"]
    out["states"], out["controls"] = got["sol"]["states"], got["sol"]["controls"]
    for key in ("iter", "solved", "residuals"):
        out["status_" + key] = np.asarray(got["st"][key])
    for key in ("d", "y", "g", "v", "z"):
        out["ws_" + key] = np.asarray(got["ws"][key])
    out["status"] = np.array([logs[-1]["status"], got["status"]], dtype=np.int64)
    out["launch_name"] = np.frombuffer(f"{bs.last_launch_name} x {_launches(bs)}".encode(), dtype=np.uint8)
    bs.close()
    return out


def _rollouts(bs, x0, parts=(STEPS,), between=None):
    bs.set_x0(x0)
    logs = []
    for i, n in enumerate(parts):
        if i and between:
            between(bs)
        logs.append(bs.mpc_rollout(n))
    return _record(bs, logs)


def _route_case(name):
    """tests/test_rollout_routes_gpu.py's matrix-core and lean chains at this batch"""
    import tinympc_julia_amd as t
    from tests import test_rollout_routes_gpu as R
    make, env, kw, more, warm, want = R.CASES[name]
    _env(env)
    prob, x0 = make()
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    bs.update_settings(**kw)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(warm)
    out = _rollouts(bs, np.asfortranarray(x0[:, :B]))
    return out, want[1]


def _cases():
    from tests import test_noise_loop_gpu as NZ
    from tests import test_plant_loop_gpu as P
    from tests import test_ref_trajectory_gpu as TR
    from tests import test_stream_loop_gpu as S
    assert (P.B, S.B, TR.B) == (B, B, B)

    def stream(name, precision=None, env=MPC, **kw):
        def run():
            case = S._case(name)
            _env(case.get("env", {}), env)
            return _rollouts(S._solver(case, precision), case["x0"], **kw)
        return run

    def plant(name, env=(), **kw):
        def run():
            case = P._case(name)
            _env(case.get("env", {}), *env)
            return _rollouts(P._solver(case), case["x0"], **kw)
        return run

    def noise(name, drop=(), env=()):
        def run():
            case = NZ._without(NZ._ncase(name), *drop)
            _env(case.get("env", {}), *env)
            bs = P._solver(case)
            NZ._install_noise(bs, case)
            return _rollouts(bs, case["x0"])
        return run

    def trajectory():
        case = TR._case("cartpole20")
        _env(case.get("env", {}))
        return _rollouts(TR._solver(case), case["x0"])

    def refit_fdyn(bs):
        bs.set_fdyn(1.5 * S._case("rocket12_cones_fdyn")["f"])

    return {
        "mfma_chain": lambda: _route_case("mfma_chain")[0],
        "lean_chain": lambda: _route_case("lean_chain")[0],
        "stream_plain": stream("cartpole17"),
        "stream_rocket_f_cones": stream("rocket12_cones_fdyn"),
        "stream_families": stream("cartpole_families"),
        "stream_generic": stream("cartpole17_generic"),
        "stream_precision1": stream("cartpole17", precision=1),
        "stream_precision2_generic": stream("quadrotor10_p2_generic"),
        "stream_precision2_stream": stream("quadrotor10_p2_stream"),
        "own_shared_with_f": plant("quadrotor10_sequence"),
        "own_per_instance": plant("cartpole17_plant"),
        "own_per_instance_rocket": plant("rocket12"),
        "own_disturbance_only": plant("cartpole17"),
        "own_disturbance_only_families": plant("cartpole_families"),
        "noise_process": noise("cartpole20_own"),
        "noise_measurement": noise("cartpole17_plant", drop=("gw",)),
        "noise_both": noise("cartpole17_plant"),
        "noise_both_split": noise("cartpole17_plant", env=({"TINYMPC_HIP_NOISE_SPLIT": "1"},)),
        "trajectory_only": trajectory,
        "twice_3_stream": stream("cartpole17", parts=(3, 3)),
        "twice_3_own": plant("cartpole17_plant", parts=(3, 3)),
        "set_fdyn_between": stream("rocket12_cones_fdyn", parts=(STEPS, STEPS), between=refit_fdyn),
        "set_plant_then_drop_to_stream": plant("rocket12", env=(MPC,), parts=(STEPS, STEPS), between=lambda bs: bs.set_plant(None, None)),
        "set_plant_then_drop_to_disturbance": plant("cartpole17_plant", parts=(3, 3), between=lambda bs: bs.set_plant(None, None)),
    }


def run(path):
    arrays = {}
    for name, case in _cases().items():
        got = case()
        for key, a in got.items():
            arrays[f"{name}/{key}"] = a
        print(f"{name}: {len(got)} arrays, last launch {got['launch_name'].tobytes().decode()}", flush=True)
    np.savez(path, **arrays)
    print(f"{len(arrays)} arrays -> {path}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for key in bad:
        print(f"{key}: only in {pa if key in a.files else pb}")
    for key in sorted(set(a.files) & set(b.files)):
        x, y = a[key], b[key]
        same = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        print(f"{key:58s} {x.dtype!s:8s} {'x'.join(map(str, x.shape)):12s} {x.nbytes:8d} B  {'equal' if same else 'NOT EQUAL'}")
        if not same:
            bad.append(key)
    print(f"{len(a.files)} arrays against {len(b.files)}: " + (f"{len(bad)} differ: {bad}" if bad else "every array byte-equal"))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="run the cases, write this .npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    run(args.out or "rollout_bits.npz")
