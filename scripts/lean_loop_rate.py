#!/usr/bin/env python3
"""mpc_rollout of the headline shape — 65 536 cartpoles (4,1,20), 50 steps, tolerance 1e-3, max_iter 10, input bound, warm
started — timed per step in three arms:

  quad    the quad kernel's in-kernel loop                       (no switch)
  chain   the lean kernel's chain of workspace-carrying launches (TINYMPC_HIP_LEAN_WS=1)
  loop    the lean kernel's in-kernel loop, one launch           (TINYMPC_HIP_LEAN_WS=1 TINYMPC_HIP_LEAN_LOOP=1)

with check_termination 1 and 10.

    python scripts/lean_loop_rate.py [--batch 65536] [--steps 50] [--runs 3] [--out profiles/rNN_lean_loop.txt]

A fresh process per run, the arms alternating, `--runs` runs per arm and check.  A run is `--inner` (40) tinympc_mpc_rollout calls behind
a warm-up call, each on a reset workspace (launches + status; the logs stay on the device), timed with the host clock around
the synchronous calls only; its figure is the mean.  Per arm: ms per step of every run, the median, the spread
(max - min) / median; then whether every run of the loop is below every run of the chain / of the quad loop.
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

ARMS = (("quad", {}), ("chain", {"TINYMPC_HIP_LEAN_WS": "1"}), ("loop", {"TINYMPC_HIP_LEAN_WS": "1", "TINYMPC_HIP_LEAN_LOOP": "1"}))


def worker(arm, ct, batch, steps, inner):
    import tinympc_julia_amd as t
    launches = ctypes.CDLL(t.LIB_PATH).tmpc_last_rollout_launches
    launches.restype, launches.argtypes = ctypes.c_int, [ctypes.c_void_p]
    prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(batch, seed=3)
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=batch)
    bs.update_settings(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=10, check_termination=ct)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    dt = 0.0
    for k in range(inner + 1):                                # (the first call: code objects, buffers, the first launches)
        bs.reset()
        bs.set_x0(x0)
        t0 = time.perf_counter()
        st = bs.lib.tinympc_mpc_rollout(bs.h, steps, ctypes.c_void_p(0))
        if k:
            dt += time.perf_counter() - t0
        assert st >= 0, "mpc_rollout failed"
    print(json.dumps(dict(arm=arm, ct=ct, launched=bs.last_launch_name, launches=launches(bs.h), batch=batch, steps=steps,
                          ms_per_step=round(dt / inner / steps * 1e3, 5))), flush=True)
    bs.close()


def summary(ms):
    s = sorted(ms)
    med = s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])
    return med, (s[-1] - s[0]) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--inner", type=int, default=40)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", nargs=2, metavar=("ARM", "CHECK"))
    a = ap.parse_args()
    if a.worker:
        worker(a.worker[0], int(a.worker[1]), a.batch, a.steps, a.inner)
        return
    lines, got = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# scripts/lean_loop_rate.py: mpc_rollout, cartpole (4,1,20), batch {a.batch}, {a.steps} steps, tolerance 1e-3, max_iter 10, warm started; "
        f"ms per step, a fresh process per run ({a.inner} timed calls behind a warm-up call), arms alternating")
    for ct in (1, 10):
        for rep in range(a.runs):
            for arm, env in ARMS:
                e = {k: v for k, v in os.environ.items() if k not in ("TINYMPC_HIP_LEAN_WS", "TINYMPC_HIP_LEAN_LOOP")}
                e.update(env)
                cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--steps", str(a.steps), "--inner", str(a.inner),
                       "--worker", arm, str(ct)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=e)
                if p.returncode != 0:
                    print(p.stdout[-2000:], p.stderr[-2000:], flush=True)
                    sys.exit(f"{arm} check {ct}: exit status {p.returncode}")    # (nothing more is started after a failure)
                r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
                got.setdefault((ct, arm), []).append(r["ms_per_step"])
                say(f"check {ct:2d} run {rep} {arm:5s} {r['launched']:16s} {r['launches']:3d} launch(es): {r['ms_per_step']:.5f}")
    for ct in (1, 10):
        for arm, _ in ARMS:
            med, spread = summary(got[(ct, arm)])
            say(f"check {ct:2d} {arm:5s}: {got[(ct, arm)]} median {med:.5f} spread {100 * spread:.1f} %")
        lo, ch, qu = got[(ct, "loop")], got[(ct, "chain")], got[(ct, "quad")]
        say(f"check {ct:2d}: every run of the loop below every run of the chain: {max(lo) < min(ch)} (loop / chain, medians: {summary(lo)[0] / summary(ch)[0]:.3f}); "
            f"below every run of the quad loop: {max(lo) < min(qu)} (loop / quad: {summary(lo)[0] / summary(qu)[0]:.3f})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
