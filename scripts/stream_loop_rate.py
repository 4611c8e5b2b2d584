#!/usr/bin/env python3
"""The closed loop on the stream kernel, timed per step in three arms:

  host    the loop a caller steps itself: set_x0 -> solve -> get_solution per step, the plant on the host  (no switch)
  chain   mpc_rollout as the chain of workspace-carrying launches                                          (TINYMPC_HIP_STREAM_MPC=1)
  loop    mpc_rollout as one launch of the in-kernel loop where one is built, else the chain again         (+ TINYMPC_HIP_STREAM_LOOP=1)

on three workloads, all warm started and tolerance-terminated (1e-3, check_termination 1):

  rocket50    rocket N = 50, the affine term, one cone per side, references; max_iter 40; TINYMPC_HIP_NO_MFMAT=1 in every arm
              (the shape's default route is the transposed-sets kernel, which has a loop of its own)      stream4<6,3>
  quadrotor27 quadrotor N = 27, box; max_iter 20; TINYMPC_HIP_NO_JIT=1 in every arm (a specialised matrix-core
              kernel would take the horizon and its own chain the loop)                                    stream4<12,4> (no loop kernel)
  quadrotor10 quadrotor N = 10 at precision 2, TINYMPC_HIP_STREAM_F64=1 in every arm; max_iter 20         stream4<12,4;f64>

    python scripts/stream_loop_rate.py [--batch 65536] [--steps 10] [--runs 3] [--inner 3] [--host-lib PATH] [--only WORKLOAD] [--out profiles/rNN_stream_loop.txt]

A fresh process per run, the arms alternating, `--runs` runs per arm and workload.  A run is `--inner` loops of `--steps` steps
behind a warm-up loop, each from a reset workspace, timed with the host clock; its figure is the mean per step.  The host arm
runs no code this switch pair touches; --host-lib runs it on another build of the library (an earlier commit's).  Per arm:
ms per step of every run, the median, the spread (max - min) / median; then the one criterion — every run of the chain below
every run of the host-stepped loop — and the loop-to-chain ratio of the medians, which is reported, not judged.
Nothing more is started after a run that fails.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWITCHES = ("TINYMPC_HIP_STREAM_MPC", "TINYMPC_HIP_STREAM_LOOP", "TINYMPC_HIP_NO_MFMAT", "TINYMPC_HIP_STREAM_F64", "TINYMPC_HIP_NO_JIT")
ARMS = (("host", {}), ("chain", {"TINYMPC_HIP_STREAM_MPC": "1"}), ("loop", {"TINYMPC_HIP_STREAM_MPC": "1", "TINYMPC_HIP_STREAM_LOOP": "1"}))
WORKLOADS = (("rocket50", {"TINYMPC_HIP_NO_MFMAT": "1"}), ("quadrotor27", {"TINYMPC_HIP_NO_JIT": "1"}), ("quadrotor10", {"TINYMPC_HIP_STREAM_F64": "1"}))


def make(work, batch):
    import numpy as np
    import tinympc_julia_amd as t
    f = None
    if work == "rocket50":
        prob, x0, max_iter = t.problems.rocket(50), t.problems.rocket_x0(batch, seed=2), 40
        f = prob.fdyn
    elif work == "quadrotor27":
        prob, x0, max_iter = t.problems.quadrotor(27), t.problems.quadrotor_x0(batch, seed=1), 20
    else:
        prob, x0, max_iter = t.problems.quadrotor(10), t.problems.quadrotor_x0(batch, seed=1), 20
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=batch)
    bs.update_settings(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=max_iter, check_termination=1)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if work == "rocket50":
        bs.set_fdyn(prob.fdyn)
        bs.set_cone_constraints([0], [3], [0.25], [0], [3], [0.5])
        xr, ur = t.problems.rocket_refs(50)
        bs.set_x_ref(xr)
        bs.set_u_ref(ur)
    bs.set_warm_start(True)
    if work == "quadrotor10":
        bs.set_precision(2)
    return t, bs, prob, x0, (np.zeros(prob.nx) if f is None else f)


def worker(arm, work, batch, steps, inner):
    import numpy as np
    t, bs, prob, x0, f = make(work, batch)
    launches = ctypes.CDLL(t.LIB_PATH).tmpc_last_rollout_launches
    launches.restype, launches.argtypes = ctypes.c_int, [ctypes.c_void_p]
    dt = 0.0
    for k in range(inner + 1):                                # (the first loop: code objects, buffers, the first launches)
        bs.reset()
        bs.set_x0(x0)
        t0 = time.perf_counter()
        if arm == "host":
            x = x0
            for _ in range(steps):
                bs.set_x0(x)
                bs.solve()
                u0 = bs.get_solution()["controls"][:, 0, :]
                x = np.asfortranarray(prob.A @ x + prob.B @ u0 + f[:, None])
        else:
            st = bs.lib.tinympc_mpc_rollout(bs.h, steps, ctypes.c_void_p(0))
            assert st >= 0, "mpc_rollout failed"
        if k:
            dt += time.perf_counter() - t0
    print(json.dumps(dict(arm=arm, work=work, launched=bs.last_launch_name, launches=launches(bs.h), batch=batch, steps=steps,
                          ms_per_step=round(dt / inner / steps * 1e3, 5))), flush=True)
    bs.close()


def summary(ms):
    s = sorted(ms)
    med = s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])
    return med, (s[-1] - s[0]) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--host-lib", default="")
    ap.add_argument("--only", default="", help="one workload instead of the three")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", nargs=2, metavar=("ARM", "WORKLOAD"))
    a = ap.parse_args()
    if a.worker:
        if a.worker[0] == "host" and a.host_lib:
            import tinympc_julia_amd as t
            t.load_library(a.host_lib)
        worker(a.worker[0], a.worker[1], a.batch, a.steps, a.inner)
        return
    lines, got = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# scripts/stream_loop_rate.py: closed loops on the stream kernel, batch {a.batch}, {a.steps} steps, tolerance 1e-3, warm started; ms per step, "
        f"a fresh process per run ({a.inner} timed loops behind a warm-up loop), arms alternating"
        + (f"; the host arm on {a.host_lib}" if a.host_lib else ""))
    workloads = [w for w in WORKLOADS if not a.only or w[0] == a.only]
    for work, wenv in workloads:
        for rep in range(a.runs):
            for arm, env in ARMS:
                e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
                e.update(wenv)
                e.update(env)
                cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--steps", str(a.steps), "--inner", str(a.inner),
                       "--worker", arm, work] + (["--host-lib", a.host_lib] if a.host_lib else [])
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=e)
                if p.returncode != 0:
                    print(p.stdout[-2000:], p.stderr[-2000:], flush=True)
                    sys.exit(f"{work} {arm}: exit status {p.returncode}")    # (nothing more is started after a failure)
                r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
                got.setdefault((work, arm), []).append(r["ms_per_step"])
                say(f"{work:11s} run {rep} {arm:5s} {r['launched']:18s} {r['launches']:3d} launch(es): {r['ms_per_step']:.5f}")
    for work, _ in workloads:
        for arm, _ in ARMS:
            med, spread = summary(got[(work, arm)])
            say(f"{work:11s} {arm:5s}: {got[(work, arm)]} median {med:.5f} spread {100 * spread:.1f} %")
        ho, ch, lo = got[(work, "host")], got[(work, "chain")], got[(work, "loop")]
        say(f"{work:11s}: every run of the chain below every run of the host-stepped loop: {max(ch) < min(ho)} (host / chain, medians: "
            f"{summary(ho)[0] / summary(ch)[0]:.2f}); loop / chain, medians: {summary(lo)[0] / summary(ch)[0]:.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
