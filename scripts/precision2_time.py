"""precision 2 (the reference's fp64 arithmetic end to end) on the headline workload — cartpole (4,1,20), 65 536 instances, 100
iterations, cold one-shot: the generic kernel's fp64-state form (TINYMPC_HIP_NO_JIT=1) against the lean kernel's fp64-state
variant specialised on request, with the library's default precision beside them.

`precision2_time.py --stream`: the stream kernel's fp64-state form (TINYMPC_HIP_STREAM_F64=1, "stream4<NX,NU;f64>") on the shapes
and calling patterns the lean kernel does not take, in ONE process, three alternating runs per arm:
  generic   precision 2, switch off: generic<f64> (what precision 2 runs on without the switch)
  stream64  precision 2, switch on
  stream32  precision 0 forced onto the fp32-state stream kernel (TINYMPC_HIP_NO_QUAD, TINYMPC_HIP_NO_MFMA): the bandwidth
            yardstick — same kernel, state half as wide
Each run: a fresh solver (the switches are read at creation), one warm-up solve, `REPS` timed ones (device events around the
kernel; mean).  Printed per workload: every run, the per-arm median, min..max, and the two ratios."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_arms():
    import statistics
    import numpy as np
    sys.path.insert(0, ROOT)
    import tinympc_julia_amd as t
    P = t.problems
    fixed = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=100, check_termination=1)
    REPS = 2

    def quadrotor(keep):
        return "quadrotor N=30 x 65536 x 100 it, " + ("workspace kept" if keep else "cold"), P.quadrotor(30), P.quadrotor_x0(65536, seed=1), None, False, keep

    def rocket_soc():
        return "config 4: rocket N=50 cones + fdyn x 32768 x 100 it, cold", P.rocket(50), P.rocket_x0(32768, seed=2), P.rocket_refs(50), True, False

    def cartpole_ws():
        return "cartpole N=20 x 65536 x 100 it, workspace kept", P.cartpole(20, u_bound=0.5), P.cartpole_x0(65536, seed=0), None, False, True
    ARMS = (("generic", 2, {}), ("stream64", 2, {"TINYMPC_HIP_STREAM_F64": "1"}),
            ("stream32", 0, {"TINYMPC_HIP_NO_QUAD": "1", "TINYMPC_HIP_NO_MFMA": "1"}))
    names = ("TINYMPC_HIP_STREAM_F64", "TINYMPC_HIP_NO_QUAD", "TINYMPC_HIP_NO_MFMA")
    for label, prob, x0, refs, soc, keep in (quadrotor(False), quadrotor(True), rocket_soc(), cartpole_ws()):
        print(f"== {label}", flush=True)
        ms = {a[0]: [] for a in ARMS}
        kern = {}
        for rep in range(3):
            for arm, prec, env in ARMS:
                for n in names:
                    os.environ.pop(n, None)
                os.environ.update(env)
                bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=x0.shape[1])
                bs.update_settings(**fixed)
                bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
                bs.set_precision(prec)
                if soc:
                    bs.set_fdyn(prob.fdyn)
                    bs.set_cone_constraints([0], [3], [prob.extra["cone_mu_u"]], [0], [3], [prob.extra["cone_mu_x"]])
                bs.set_warm_start(keep)
                bs.set_x0(x0)
                if refs is not None:
                    bs.set_x_ref(refs[0]); bs.set_u_ref(refs[1])
                bs.set_profiling(True)
                for _ in range(1 + REPS): bs.solve()
                v = bs.kernel_elapsed_ms(REPS)
                ms[arm].append(v)
                kern[arm] = bs.last_launch_name
                print(f"   run {rep} {arm:9s} {bs.last_launch_name:20s} {v:10.3f} ms", flush=True)
                bs.close()
        med = {a: statistics.median(v) for a, v in ms.items()}
        for a, v in ms.items():
            print(f"   {a:9s} {kern[a]:20s} median {med[a]:10.3f} ms   min {min(v):10.3f}  max {max(v):10.3f}  spread {100 * (max(v) - min(v)) / med[a]:5.1f} %")
        print(f"   generic<f64> / stream f64 = {med['generic'] / med['stream64']:.1f} x     stream f64 / stream fp32-state = {med['stream64'] / med['stream32']:.2f} x", flush=True)


if "--stream" in sys.argv:
    os.environ["TINYMPC_HIP_NO_JIT"] = "1"     # (no unit specialised at setup: the kernels of the built library only)
    stream_arms()
    sys.exit(0)
code = r'''
import numpy as np, sys, os
sys.path.insert(0, os.getcwd())
import tinympc_julia_amd as t
B = 65536
prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(B, 0)
for prec, kw in ((0, dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=100, check_termination=1)), (2, dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=100, check_termination=1)),
                 (2, dict(abs_pri_tol=1e-30, abs_dua_tol=1e-30, max_iter=100, check_termination=1))):
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=B)
    bs.update_settings(**kw)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_precision(prec); bs.set_warm_start(False); bs.set_x0(x0); bs.set_profiling(True)
    for _ in range(6): bs.solve()
    print(f"NO_JIT={os.environ.get('TINYMPC_HIP_NO_JIT', '0')}  precision {prec}  {'check live' if kw['abs_pri_tol'] > 0 else 'fixed     '}  {bs.last_launch_name:18s} {bs.kernel_elapsed_ms(3):9.3f} ms", flush=True)
    bs.close()
'''
env = dict(os.environ, TINYMPC_HIP_CACHE=os.path.join(ROOT, "gpurun_out", "jit_cache"))
env.pop("TINYMPC_HIP_NO_JIT", None)
subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env)
subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, TINYMPC_HIP_NO_JIT="1"))
