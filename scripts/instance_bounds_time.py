#!/usr/bin/env python3
"""Per-instance box bounds on the stream kernel, timed in three arms:

  shared     bounds shared by the batch: the plain stream kernel                                   stream4<NX,NU>
  constant   per-instance bounds, constant over the horizon (knot stride 0: one line per instance)  stream4<NX,NU;ib>
  per_knot   per-instance bounds per knot (2 nx + 2 nu more floats per knot and iteration)          stream4<NX,NU;ib>

with the same bound values everywhere, so the arithmetic of the three arms is identical (the results are bit-identical:
tests/test_instance_bounds_gpu.py), on two workloads, one-shot solves of 100 fixed iterations:

  quadrotor27  quadrotor N = 27      cartpole17  cartpole N = 17      (TINYMPC_HIP_NO_JIT=1: no specialised on-chip unit takes them)

    python scripts/instance_bounds_time.py [--batch 65536] [--iters 100] [--runs 3] [--inner 5] [--only WORKLOAD] [--out profiles/rNN_instance_bounds.txt]

A fresh process per run, the arms alternating, `--runs` runs per arm and workload.  A run is `--inner` solves behind a warm-up
solve, timed by the events around the kernel (tinympc_set_profiling); its figure is their mean, in ms.  Per arm: every run, the
median, the spread (max - min) / median; then constant / shared and per_knot / shared of the medians beside what the traffic
predicts: the one-shot form moves 10 nx + 12 nu floats per knot and iteration (csrc/admm_streamg.hip.h), the per-knot bounds add
2 nx + 2 nu, the constant ones nothing.  Nothing more is started after a run that fails.
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = ("shared", "constant", "per_knot")
WORKLOADS = ("quadrotor27", "cartpole17")


def worker(arm, work, batch, iters, inner):
    import numpy as np
    import tinympc_julia_amd as t
    if work == "quadrotor27":
        prob, x0 = t.problems.quadrotor(27), t.problems.quadrotor_x0(batch, seed=1)
    else:
        prob, x0 = t.problems.cartpole(17, u_bound=0.5), t.problems.cartpole_x0(batch, seed=0)
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=batch)
    bs.update_settings(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=iters, check_termination=1)
    shared = (prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if arm == "shared":
        bs.set_bound_constraints(*shared)
    elif arm == "constant":
        bs.set_instance_bounds(*[np.repeat(a[:, :1], batch, axis=1) for a in shared])
    else:
        bs.set_instance_bounds(*[np.repeat(a[:, :, None], batch, axis=2) for a in shared])
    bs.set_warm_start(False)
    bs.set_profiling(True)
    bs.set_x0(x0)
    for _ in range(inner + 1):        # (the first solve: code object, buffers, uploads)
        bs.solve()
    ms = bs.kernel_elapsed_ms(last_n=inner)
    print(json.dumps(dict(arm=arm, work=work, launched=bs.last_launch_name, batch=batch, iters=iters, kernel_ms=round(ms, 5),
                          algorithmic_mb=round(bs.algorithmic_bytes() / 1e6, 1))), flush=True)
    bs.close()


def summary(ms):
    s = sorted(ms)
    med = s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])
    return med, (s[-1] - s[0]) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--only", default="", help="one workload instead of the two")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", nargs=2, metavar=("ARM", "WORKLOAD"))
    a = ap.parse_args()
    if a.worker:
        worker(a.worker[0], a.worker[1], a.batch, a.iters, a.inner)
        return
    lines, got = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# scripts/instance_bounds_time.py: one-shot solves on the stream kernel, batch {a.batch}, {a.iters} fixed iterations; kernel ms, "
        f"a fresh process per run ({a.inner} timed solves behind a warm-up solve), arms alternating")
    workloads = [w for w in WORKLOADS if not a.only or w == a.only]
    env = dict(os.environ, TINYMPC_HIP_NO_JIT="1")
    for work in workloads:
        for rep in range(a.runs):
            for arm in ARMS:
                cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--iters", str(a.iters), "--inner", str(a.inner),
                       "--worker", arm, work]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
                if p.returncode != 0:
                    print(p.stdout[-2000:], p.stderr[-2000:], flush=True)
                    sys.exit(f"{work} {arm}: exit status {p.returncode}")    # (nothing more is started after a failure)
                r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
                got.setdefault((work, arm), []).append(r["kernel_ms"])
                say(f"{work:11s} run {rep} {arm:8s} {r['launched']:18s} {r['kernel_ms']:.5f} ms   (algorithmic {r['algorithmic_mb']} MB)")
    shapes = dict(quadrotor27=(12, 4), cartpole17=(4, 1))
    for work in workloads:
        for arm in ARMS:
            med, spread = summary(got[(work, arm)])
            say(f"{work:11s} {arm:8s}: {got[(work, arm)]} median {med:.5f} spread {100 * spread:.1f} %")
        nx, nu = shapes[work]
        share = (2.0 * nx + 2.0 * nu) / (10.0 * nx + 12.0 * nu)
        sh, co, pk = (summary(got[(work, arm)])[0] for arm in ARMS)
        say(f"{work:11s}: constant / shared {co / sh:.3f} (predicted 1.000); per_knot / shared {pk / sh:.3f} (predicted 1 + "
            f"(2 nx + 2 nu) / (10 nx + 12 nu) = {1.0 + share:.3f})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
