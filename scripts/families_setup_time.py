#!/usr/bin/env python3
"""Setup of a per-instance-family solver, timed in two arms:

  host     tinympc_create_families: Riccati per instance in host threads, the pack filled on the host, one upload
  device   tinympc_create_families_device: riccati_families_kernel and fill_family_pack_kernel (csrc/families_setup.hip)

on three workloads — cartpole (4,1) N = 20, rocket (6,3) N = 50, quadrotor (12,4) N = 30 — whose families are the base problem
with A perturbed by 2 %, B by 5 %, Q and R scaled in [0.5, 2] and rho in [0.5, 3] (the recipe of test_per_instance_families_vs_oracle;
tests/families_cases.py: perturbed), at batches 4 096 and 65 536.

    python scripts/families_setup_time.py [--batches 4096,65536] [--runs 3] [--only WORKLOAD] [--out profiles/rNN_families_setup_time.txt]

The figure is WALL time from the create call to the end of the first solve (create, settings, bounds, x0, one solve of 10 fixed
iterations, the status read back), in ms; drawing the families is outside it.  One worker process per workload and batch, under
its own time limit, one at a time (one process on one GPU); in it, behind a warm-up of both arms at 64 instances (code objects,
the runtime's first allocations), the arms alternate, `--runs` runs each.  For the device arm also the kernel times of the two
kernels (events, tinympc_families_setup_ms), the histogram of the sweep counts, and what the Riccati kernel's time means in fp64
operations: an instance's sweep is 2 (3 nx^2 nu + nu^2 nx + 2 nx^3) operations in the matrix products (the replicated nu x nu
solve is not counted), the kernel runs an instance's group until the LAST of its wavefront's four instances is done, so "useful" counts
every instance's own sweeps and "issued" four times the wavefront's longest.  Nothing more is started after a worker that fails.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"cartpole": (4, 1), "rocket": (6, 3), "quadrotor": (12, 4)}
ARMS = ("host", "device")


def worker(work, batch, runs):
    import numpy as np
    import tinympc_julia_amd as t
    from tests import families_cases as fc
    shape = WORKLOADS[work]
    base = fc.base_problem(shape)
    nx, nu = shape
    x0_of = dict(cartpole=t.problems.cartpole_x0, rocket=t.problems.rocket_x0, quadrotor=t.problems.quadrotor_x0)[work]

    def run(arm, fam, x0):
        t0 = time.perf_counter()
        bs = t.BatchSolver.from_families(*fam, base.N, setup=arm)
        bs.update_settings(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=10, check_termination=1)
        bs.set_bound_constraints(base.x_min, base.x_max, base.u_min, base.u_max)
        bs.set_x0(x0)
        bs.solve()
        bs.get_status()
        wall = 1e3 * (time.perf_counter() - t0)
        out = dict(arm=arm, wall_ms=round(wall, 2), launched=bs.last_launch_name)
        if arm == "device":
            ric, fill = bs.families_setup_ms()
            sw = bs.family_cache(sweeps_only=True)["sweeps"].astype(np.int64)
            pad = np.concatenate([sw, np.zeros((-len(sw)) % 4, dtype=np.int64)]).reshape(-1, 4)
            per_sweep = 2.0 * (3 * nx * nx * nu + nu * nu * nx + 2 * nx ** 3)
            hist, edges = np.histogram(sw, bins=[0, 50, 100, 200, 300, 400, 600, 800, 1000, 1001])
            out.update(riccati_ms=round(ric, 4), fill_ms=round(fill, 4), sweeps_mean=round(float(sw.mean()), 1), sweeps_min=int(sw.min()),
                       sweeps_max=int(sw.max()), at_cap=int((sw >= 1000).sum()), hist=hist.tolist(), hist_edges=edges.tolist(),
                       useful_gflops=round(per_sweep * sw.sum() / (ric * 1e6), 1),
                       issued_gflops=round(per_sweep * 4.0 * pad.max(axis=1).sum() / (ric * 1e6), 1),
                       issued_over_useful=round(4.0 * pad.max(axis=1).sum() / sw.sum(), 3))
        bs.close()
        return out

    small = fc.perturbed(base, 64, 7)
    for arm in ARMS:                       # warm-up, not reported
        run(arm, small, x0_of(64, seed=1))
    fam, x0 = fc.perturbed(base, batch, 2026), x0_of(batch, seed=3)
    for rep in range(runs):
        for arm in ARMS:
            print(json.dumps(dict(work=work, batch=batch, rep=rep, **run(arm, fam, x0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,65536")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default="", help="one workload instead of the three")
    ap.add_argument("--out", default="")
    ap.add_argument("--limit", type=int, default=240, help="seconds a worker may take")
    ap.add_argument("--worker", nargs=2, metavar=("WORKLOAD", "BATCH"))
    a = ap.parse_args()
    if a.worker:
        worker(a.worker[0], int(a.worker[1]), a.runs)
        return
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# scripts/families_setup_time.py: wall ms from the create call to the end of the first solve (10 fixed iterations), per-instance families; "
        f"one worker process per workload and batch, arms alternating behind a warm-up, {a.runs} runs each")
    env = dict(os.environ, TINYMPC_HIP_NO_JIT="1")
    for work in [w for w in WORKLOADS if not a.only or w == a.only]:
        for batch in [int(b) for b in a.batches.split(",")]:
            cmd = [sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--worker", work, str(batch)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit, env=env)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:], flush=True)
                sys.exit(f"{work} {batch}: exit status {p.returncode}")    # (nothing more is started after a failure)
            rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
            host = [r["wall_ms"] for r in rows if r["arm"] == "host"]
            dev = [r for r in rows if r["arm"] == "device"]
            dw = [r["wall_ms"] for r in dev]
            nx, nu = WORKLOADS[work]
            say(f"{work} ({nx},{nu}) batch {batch} [{rows[0]['launched']}]")
            say(f"  host   wall ms {host}")
            say(f"  device wall ms {dw}   riccati kernel ms {[r['riccati_ms'] for r in dev]}   fill kernel ms {[r['fill_ms'] for r in dev]}")
            say(f"  every device run below every host run: {max(dw) < min(host)}   slowest device / fastest host {max(dw) / min(host):.4f}   "
                f"median host / median device {sorted(host)[len(host) // 2] / sorted(dw)[len(dw) // 2]:.1f}")
            d = dev[-1]
            say(f"  sweeps: mean {d['sweeps_mean']} min {d['sweeps_min']} max {d['sweeps_max']} at the cap {d['at_cap']}; histogram "
                + " ".join(f"[{int(lo)},{int(hi)}):{n}" for lo, hi, n in zip(d["hist_edges"][:-1], d["hist_edges"][1:], d["hist"]) if n))
            say(f"  riccati kernel: {d['useful_gflops']} useful fp64 GFLOP/s, {d['issued_gflops']} issued (issued / useful {d['issued_over_useful']}: "
                f"a group runs until its wavefront's last instance is done)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
