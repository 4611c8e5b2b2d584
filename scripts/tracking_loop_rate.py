#!/usr/bin/env python3
"""Closed loops that follow a moving reference (set_ref_sequence + mpc_rollout), timed per shape and kernel family in three arms:

  seq     the fused / chained loop with a reference sequence (every step on its own shared references)
  noseq   the same loop without a sequence (the references never move)
  host    the loop stepped by the host: set_x_ref, set_u_ref, set_x0, solve per step, the plant applied on the host to the
          first control of the fp32 solution (what a caller without the sequence does to follow a moving reference)

    python scripts/tracking_loop_rate.py [--shape cartpole|quadrotor|both] [--batch 65536] [--runs 3]
    python scripts/tracking_loop_rate.py --ab LIB_A LIB_B [--shape ...]

cartpole: (4,1,20), 50 steps — the quad kernel's in-kernel loop, and the lean kernel's chain (TINYMPC_HIP_LEAN_WS=1);
quadrotor: (12,4,30), 20 steps — the matrix-core chain (mfma; the shape's quad entry takes no sequence at this horizon).
Tolerances 1e-3, max_iter 10, input bound, warm-started.
The arms alternate, `--runs` times each; a fused run is ten tinympc_mpc_rollout calls, each on a reset workspace (launches +
status, the logs stay on the device), timed with the host clock around the synchronous calls only.  Per arm: ms per step of every run, the
median, and the spread (max - min) / median.
--ab: the loop WITHOUT a sequence on two builds of the library (say, a parent commit's and this tree's), a fresh process per
library and repetition, alternating — the spread of each side is the yardstick for the difference between them.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = dict(cartpole=dict(N=20, steps=50, families=(("quad", {}), ("lean", {"TINYMPC_HIP_LEAN_WS": "1"}))),
              quadrotor=dict(N=30, steps=20, families=(("mfma", {}),)))
KW = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=10, check_termination=1)


def refs(shape, N, steps):
    """the position reference on a ramp in knot + step (as rocket_landing_constraints.jl:107-115 shifts its own)"""
    import numpy as np
    nx, nu = (4, 1) if shape == "cartpole" else (12, 4)
    xs, us = np.zeros((nx, N, steps)), np.zeros((nu, N - 1, steps))
    ik = np.arange(N)[:, None] + np.arange(steps)[None, :]
    if shape == "cartpole":
        xs[0] = 0.005 * ik
    else:
        for row, rate in ((0, 1.0), (1, 0.5), (2, 0.25)):
            xs[row] = 0.002 * rate * ik
            xs[6 + row] = 0.002 * rate / 0.05
    return xs, us


def measure(shape, batch, runs, arms, families, lib):
    import numpy as np
    import tinympc_julia_amd as t
    if lib:
        from tinympc_julia_amd import tinympc as tm
        tm.load_library(lib)
    cfg = SHAPES[shape]
    N, steps = cfg["N"], cfg["steps"]
    prob = (t.problems.cartpole(N, u_bound=0.5), t.problems.quadrotor(N))[shape == "quadrotor"]
    x0 = (t.problems.cartpole_x0(batch, seed=3), t.problems.quadrotor_x0(batch, seed=3))[shape == "quadrotor"]
    xs, us = refs(shape, N, steps)
    out = []
    for fam, env in cfg["families"]:
        if families and fam not in families:
            continue
        for k, v in env.items():
            os.environ[k] = v

        def make(seq):
            bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=batch)
            bs.update_settings(**KW)
            bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
            if seq:
                bs.set_ref_sequence(xs, us)
            else:
                bs.set_x_ref(xs[:, :, 0])
                bs.set_u_ref(us[:, :, 0])
            return bs

        solvers = {a: make(a == "seq") for a in arms}
        for k in env:
            del os.environ[k]
        sf = np.zeros((prob.nx, N, batch), dtype=np.float32, order="F")
        cf = np.zeros((prob.nu, N - 1, batch), dtype=np.float32, order="F")

        def fused(bs, inner=10):
            dt = 0.0
            for _ in range(inner):                            # the same loop `inner` times: only the rollouts are timed
                bs.reset()
                bs.set_x0(x0)
                t0 = time.perf_counter()
                st = bs.lib.tinympc_mpc_rollout(bs.h, steps, ctypes.c_void_p(0))
                dt += time.perf_counter() - t0
                assert st >= 0, "mpc_rollout failed"
            return dt / inner

        def host(bs):
            bs.reset()
            x = x0.copy()
            t0 = time.perf_counter()
            for k in range(steps):
                bs.set_x_ref(xs[:, :, k])
                bs.set_u_ref(us[:, :, k])
                bs.set_x0(x)
                bs.solve()
                bs.get_solution_f32(sf, cf)
                x = prob.A @ x + prob.B @ cf[:, 0, :].astype(np.float64)
            return time.perf_counter() - t0

        times = {a: [] for a in arms}
        for a in arms:                                        # warm-up: code objects, buffers, the first launches
            (host if a == "host" else fused)(solvers[a])
        for _ in range(runs):
            for a in arms:
                times[a].append((host if a == "host" else fused)(solvers[a]) / steps * 1e3)
        for a in arms:
            bs = solvers[a]
            out.append(dict(shape=shape, family=fam, arm=a, kernel=bs.kernel_name, launched=bs.last_launch_name, batch=batch, steps=steps,
                            ms_per_step=[round(v, 4) for v in times[a]]))
            bs.close()
    return out


def summary(ms):
    s = sorted(ms)
    med = s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])
    return med, (s[-1] - s[0]) / med


def report(rows):
    for r in rows:
        med, spread = summary(r["ms_per_step"])
        print(f"{r['shape']:9s} {r['family']:5s} {r['arm']:5s} {r['launched']:18s} {r['batch']} x {r['steps']} steps: "
              f"ms per step {r['ms_per_step']} median {med:.4f} spread {100 * spread:.1f} %", flush=True)
    for key in sorted({(r["shape"], r["family"]) for r in rows}):
        arm = {r["arm"]: summary(r["ms_per_step"])[0] for r in rows if (r["shape"], r["family"]) == key}
        if "seq" in arm and "host" in arm:
            print(f"{key[0]:9s} {key[1]:5s} host-stepped / fused with a sequence = {arm['host'] / arm['seq']:.2f}"
                  + (f"; with a sequence / without = {arm['seq'] / arm['noseq']:.3f}" if "noseq" in arm else ""), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["cartpole", "quadrotor", "both"])
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--arms", default="seq,noseq,host")
    ap.add_argument("--families", default="")
    ap.add_argument("--lib", default="")
    ap.add_argument("--json", action="store_true", help="one JSON line per arm (what --ab reads)")
    ap.add_argument("--ab", nargs=2, metavar=("LIB_A", "LIB_B"))
    a = ap.parse_args()
    shapes = ["cartpole", "quadrotor"] if a.shape == "both" else [a.shape]
    if a.ab:
        got = {}
        for rep in range(a.runs):
            for lib in a.ab:
                cmd = [sys.executable, os.path.abspath(__file__), "--shape", a.shape, "--batch", str(a.batch), "--runs", "3", "--arms", "noseq",
                       "--lib", lib, "--json"] + (["--families", a.families] if a.families else [])
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    print(p.stdout[-2000:], p.stderr[-2000:], flush=True)
                    sys.exit(f"{lib}: exit status {p.returncode}")    # (nothing more is started after a failure)
                for line in p.stdout.splitlines():
                    if line.startswith("{"):
                        r = json.loads(line)
                        got.setdefault((r["shape"], r["family"], lib), []).append(min(r["ms_per_step"]))
                        print(f"rep {rep} {lib}: {r['shape']} {r['family']} {r['launched']} without a sequence, ms per step {r['ms_per_step']}", flush=True)
        for (shape, fam, lib), v in sorted(got.items()):
            med, spread = summary(v)
            print(f"{shape:9s} {fam:5s} {lib}: best of each process {[round(x, 4) for x in v]} median {med:.4f} spread {100 * spread:.1f} %")
        for shape, fam in sorted({k[:2] for k in got}):
            ma, mb = summary(got[(shape, fam, a.ab[0])])[0], summary(got[(shape, fam, a.ab[1])])[0]
            print(f"{shape:9s} {fam:5s} B / A = {mb / ma:.4f}")
        return
    rows = []
    for shape in shapes:
        rows += measure(shape, a.batch, a.runs, a.arms.split(","), a.families.split(",") if a.families else None, a.lib)
    if a.json:
        for r in rows:
            print(json.dumps(r), flush=True)
    else:
        report(rows)


if __name__ == "__main__":
    main()
