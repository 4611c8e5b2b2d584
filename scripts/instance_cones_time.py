#!/usr/bin/env python3
"""Per-instance cone coefficients on the stream kernel, timed in five arms:

  shared     the rocket's thrust and glide-slope cones shared by the batch: the plain stream kernel's EXT = 1 form     stream4<6,3>
  bounds     the same, with the shared box bounds given per instance: the `ib` form's EXT = 1 text                     stream4<6,3;ib>
  instance   the same cones with a coefficient per instance (tinympc_set_instance_cones), every instance the same
             values: the `ic` form, which is the EXT = 2 text reading bounds, rows and coefficients per instance       stream4<6,3;ic>
  rows       the shared cones beside one state and one input row per instance that never act: the `il` form            stream4<6,3;il>
  rows_inst  the per-instance coefficients beside those rows: the `ic` form doing the `il` arm's arithmetic             stream4<6,3;ic>

so the arithmetic of shared / bounds / instance is identical, and that of rows / rows_inst (the results are bit-identical:
tests/test_instance_cones_gpu.py).  instance / shared is what a caller pays; bounds / shared is the share of the bounds read per
instance; rows_inst / rows is what the coefficients alone cost over the EXT = 2 text they share.  All on the rocket
landing problem at N = 50 with the affine term and the references, one-shot solves of 100 fixed iterations
(TINYMPC_HIP_NO_MFMAT=1 and TINYMPC_HIP_NO_MFMAC=1: the shared arm would otherwise run on a matrix-core kernel — `mfmat`, or for
one-shot solves `mfmar` — which is another algorithm's schedule).

    python scripts/instance_cones_time.py [--batch 65536] [--iters 100] [--runs 3] [--inner 5] [--out profiles/rNN_instance_cones.txt]

A fresh process per run, the arms alternating, `--runs` runs per arm.  A run is `--inner` solves behind a warm-up solve, timed by
the events around the kernel (tinympc_set_profiling); its figure is their mean, in ms.  Per arm: every run, the median, the
spread (max - min) / median; then the ratios of the medians.  The arithmetic predicts no ratio beyond the one-off read of
the coefficients (one float per cone and instance) — what instance / shared shows is the cost of the `ic` form's text: the EXT = 2
kernel (scripts/instance_rows_time.py measures that text on other shapes, instance / shared rows) with its bounds read per instance
at knot stride 0 and a cone's coefficient read from LDS instead of a scalar register.  Nothing more is started after a run that fails.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("shared", "bounds", "instance", "rows", "rows_inst")
CONES = ([0], [3], [0.25], [0], [3], [0.5])       # Acu, qcu, cu, Acx, qcx, cx: thrust pointing, glide slope
NAMES = dict(shared="stream4<6,3>", bounds="stream4<6,3;ib>", instance="stream4<6,3;ic>", rows="stream4<6,3;il>", rows_inst="stream4<6,3;ic>")
FAR = 1.0e6      # a right-hand side no trajectory reaches


def worker(arm, batch, iters, inner):
    import numpy as np
    import tinympc_julia_amd as t
    N = 50
    prob, x0 = t.problems.rocket(N), t.problems.rocket_x0(batch, seed=1)
    xr, ur = t.problems.rocket_refs(N)
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=batch)
    bs.update_settings(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=iters, check_termination=1)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_fdyn(prob.fdyn)
    bs.set_x_ref(xr)
    bs.set_u_ref(ur)
    if arm in ("shared", "bounds", "rows"):
        bs.set_cone_constraints(*CONES)
    else:
        bs.set_instance_cones(CONES[0], CONES[1], np.full((1, batch), CONES[2][0]), CONES[3], CONES[4], np.full((1, batch), CONES[5][0]))
    if arm == "bounds":
        bs.set_instance_bounds(*[np.repeat(a[:, :1], batch, axis=1) for a in (prob.x_min, prob.x_max, prob.u_min, prob.u_max)])
    if arm in ("rows", "rows_inst"):
        Ax, Au = np.zeros((1, prob.nx, batch)), np.zeros((1, prob.nu, batch))
        Ax[0, 2, :], Au[0, 2, :] = 1.0, 1.0
        bs.set_instance_linear(Ax, np.full((1, batch), FAR), Au, np.full((1, batch), FAR))
    bs.set_warm_start(False)
    bs.set_profiling(True)
    bs.set_x0(x0)
    for _ in range(inner + 1):        # (the first solve: code object, buffers, uploads)
        bs.solve()
    ms = bs.kernel_elapsed_ms(last_n=inner)
    launched = bs.last_launch_name
    print(json.dumps(dict(arm=arm, launched=launched, batch=batch, iters=iters, kernel_ms=round(ms, 5),
                          algorithmic_mb=round(bs.algorithmic_bytes() / 1e6, 1))), flush=True)
    bs.close()
    if launched != NAMES[arm]:
        sys.exit(f"{arm}: ran on {launched}, not on {NAMES[arm]}")


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
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", metavar="ARM")
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.batch, a.iters, a.inner)
        return
    lines, got = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# scripts/instance_cones_time.py: rocket N = 50 with the affine term and references, one-shot solves on the stream kernel, batch "
        f"{a.batch}, {a.iters} fixed iterations; kernel ms, a fresh process per run ({a.inner} timed solves behind a warm-up solve), arms alternating")
    env = dict(os.environ, TINYMPC_HIP_NO_MFMAT="1", TINYMPC_HIP_NO_MFMAC="1")
    for rep in range(a.runs):
        for arm in ARMS:
            cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--iters", str(a.iters), "--inner", str(a.inner),
                   "--worker", arm]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:], flush=True)
                sys.exit(f"{arm}: exit status {p.returncode}")    # (nothing more is started after a failure)
            r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            got.setdefault(arm, []).append(r["kernel_ms"])
            say(f"rocket50 run {rep} {arm:9s} {r['launched']:16s} {r['kernel_ms']:.5f} ms   (algorithmic {r['algorithmic_mb']} MB)")
    for arm in ARMS:
        med, spread = summary(got[arm])
        say(f"rocket50 {arm:9s}: {got[arm]} median {med:.5f} spread {100 * spread:.1f} %")
    med = {arm: summary(got[arm])[0] for arm in ARMS}
    say(f"rocket50: instance / shared {med['instance'] / med['shared']:.3f}   bounds / shared {med['bounds'] / med['shared']:.3f}   "
        f"instance / bounds {med['instance'] / med['bounds']:.3f}   rows_inst / rows {med['rows_inst'] / med['rows']:.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
