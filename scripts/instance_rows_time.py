#!/usr/bin/env python3
"""Per-instance linear rows on the stream kernel, timed in two arms:

  shared     two state and two input rows shared by the batch: the plain stream kernel's EXT = 2 form     stream4<NX,NU>
  instance   the same rows given per instance (tinympc_set_instance_linear), every instance the same values  stream4<NX,NU;il>

so the arithmetic of the two arms is identical (the results are bit-identical: tests/test_instance_rows_gpu.py), on two
workloads, one-shot solves of 100 fixed iterations:

  quadrotor27  quadrotor N = 27      cartpole17  cartpole N = 17      (TINYMPC_HIP_NO_JIT=1: no specialised on-chip unit takes them)

    python scripts/instance_rows_time.py [--batch 65536] [--iters 100] [--runs 3] [--inner 5] [--only WORKLOAD] [--out profiles/rNN_instance_rows.txt]

A fresh process per run, the arms alternating, `--runs` runs per arm and workload.  A run is `--inner` solves behind a warm-up
solve, timed by the events around the kernel (tinympc_set_profiling); its figure is their mean, in ms.  Per arm: every run, the
median, the spread (max - min) / median; then instance / shared of the medians.  The arithmetic predicts no ratio beyond the
one-off read of the rows (rows_x (nx + 2) + rows_u (nu + 2) floats per instance, against 100 iterations of the knot arrays): the
`il` form keeps an instance's rows in LDS between knots and reads its bounds per instance at knot stride 0, so constant rows add
no HBM stream per knot.  Nothing more is started after a run that fails.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("shared", "instance")
WORKLOADS = ("quadrotor27", "cartpole17")


def rows_of(work, prob, x0):
    import numpy as np
    if work == "cartpole17":      # X3's rows (tests/golden/X3_cartpole_linear_rows.json)
        with open(os.path.join(ROOT, "tests", "golden", "X3_cartpole_linear_rows.json")) as f:
            g = json.load(f)["lin"]
        return np.array(g["Ax"]), np.array(g["bx"]), np.array(g["Au"]), np.array(g["bu"])
    nx, nu = prob.nx, prob.nu
    Ax = np.zeros((2, nx))
    Ax[0, 0], Ax[0, 1] = 0.6, 0.8          # a keep-out plane in the (x, y) plane
    Ax[1, 2] = 1.3                         # a scaled altitude limit
    bx = np.array([0.5 * np.abs(Ax[0] @ x0).max(), 0.5 * np.abs(Ax[1] @ x0).max()])
    Au = np.zeros((2, nu))
    Au[0, 0], Au[0, 1] = 1.0, 1.0          # a coupled limit on two rotors
    Au[1, nu - 1] = -1.1
    bu = 0.3 * np.array([2.0, 1.1]) * np.abs(prob.u_max).max()
    return Ax, bx, Au, bu


def worker(arm, work, batch, iters, inner):
    import numpy as np
    import tinympc_julia_amd as t
    if work == "quadrotor27":
        prob, x0 = t.problems.quadrotor(27), t.problems.quadrotor_x0(batch, seed=1)
    else:
        prob, x0 = t.problems.cartpole(17, u_bound=0.5), t.problems.cartpole_x0(batch, seed=0)
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=batch)
    bs.update_settings(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=iters, check_termination=1)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    Ax, bx, Au, bu = rows_of(work, prob, x0)
    if arm == "shared":
        bs.set_linear_constraints(Ax, bx, Au, bu)
    else:
        bs.set_instance_linear(np.repeat(Ax[:, :, None], batch, axis=2), np.repeat(bx[:, None], batch, axis=1),
                               np.repeat(Au[:, :, None], batch, axis=2), np.repeat(bu[:, None], batch, axis=1))
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

    say(f"# scripts/instance_rows_time.py: one-shot solves on the stream kernel, batch {a.batch}, {a.iters} fixed iterations; kernel ms, "
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
    for work in workloads:
        for arm in ARMS:
            med, spread = summary(got[(work, arm)])
            say(f"{work:11s} {arm:8s}: {got[(work, arm)]} median {med:.5f} spread {100 * spread:.1f} %")
        (sh, s_sh), (il, s_il) = (summary(got[(work, arm)]) for arm in ARMS)
        say(f"{work:11s}: instance / shared {il / sh:.3f} (spreads {100 * s_sh:.1f} % / {100 * s_il:.1f} %; predicted 1.000 beyond the one-off read of the rows)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
