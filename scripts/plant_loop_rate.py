#!/usr/bin/env python3
"""The closed loop against a plant of its own — every instance its own A_p, B_p and its own disturbance — timed per step in
three arms:

  host    the loop a caller steps itself: set_x0_f32 -> solve -> get_controls_f32 per step, the per-instance plant and the
          disturbance applied in numpy (batched matmul, fp64)
  own     set_plant + set_disturbance, then mpc_rollout: the chain of kept-workspace launches with plant_step_kernel
  model   for context only: mpc_rollout on the model plant, the loop the shape takes today (no plant, no disturbance)

on two workloads, warm started, tolerance 1e-3, max_iter 10, check_termination 1 (those of profiles/r10_tracking_loop.txt):

  cartpole    (4, 1, 20), input bound, 50 steps
  quadrotor   (12, 4, 30), 20 steps

    python scripts/plant_loop_rate.py [--batch 65536] [--runs 3] [--inner 3] [--only WORKLOAD] [--out profiles/rNN_plant_loop.txt]

Plant: A_p = A o (1 + 0.02 U), B_p = B o (1 + 0.1 U) per instance, U uniform in [-1, 1]; disturbance uniform within 1 % of each
state's scale in x0.  A fresh process per run, the arms alternating, `--runs` runs per arm and workload.  A run is `--inner`
loops behind a warm-up loop, each from a reset workspace and the same x0, timed with the host clock to the point where the
loop's results are on the host or (mpc_rollout) the call has returned, which it does after synchronising; its figure is the mean
per step.  Per arm: ms per step of every run, the median, the spread (max - min) / median; then the one criterion — every run of
`own` below every run of `host` — and own / model of the medians, the price of leaving the fused loop: reported, not judged.
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

SWITCHES = ("TINYMPC_HIP_STREAM_MPC", "TINYMPC_HIP_STREAM_LOOP", "TINYMPC_HIP_LEAN_WS", "TINYMPC_HIP_LEAN_LOOP", "TINYMPC_HIP_NO_MFMAT",
            "TINYMPC_HIP_STREAM_F64", "TINYMPC_HIP_NO_JIT")
ARMS = ("host", "own", "model")
WORKLOADS = (("cartpole", 50), ("quadrotor", 20))


def make(work, batch, steps):
    import numpy as np
    import tinympc_julia_amd as t
    if work == "cartpole":
        prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(batch, seed=2)
    else:
        prob, x0 = t.problems.quadrotor(30), t.problems.quadrotor_x0(batch, seed=1)
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=batch)
    bs.update_settings(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=10, check_termination=1)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(True)
    rng = np.random.default_rng(18)
    nx, nu = prob.nx, prob.nu
    Ap = prob.A[None] * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, (batch, nx, nx)))      # [b] row-major blocks: the host arm's matmul layout
    Bp = prob.B[None] * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, (batch, nx, nu)))
    w = 0.01 * np.abs(x0).max(axis=1)[None, None, :] * rng.uniform(-1.0, 1.0, (steps, batch, nx))
    return t, bs, prob, np.asfortranarray(x0), Ap, Bp, w


def worker(arm, work, batch, steps, inner):
    import numpy as np
    t, bs, prob, x0, Ap, Bp, w = make(work, batch, steps)
    nx, nu, N = prob.nx, prob.nu, prob.N
    launches = ctypes.CDLL(t.LIB_PATH).tmpc_last_rollout_launches
    launches.restype, launches.argtypes = ctypes.c_int, [ctypes.c_void_p]
    c_fp = ctypes.POINTER(ctypes.c_float)
    if arm == "own":
        bs.set_plant(np.transpose(Ap, (1, 2, 0)), np.transpose(Bp, (1, 2, 0)))
        bs.set_disturbance(np.transpose(w, (2, 0, 1)))
    u_all = np.zeros((batch, N - 1, nu), dtype=np.float32)                           # (nu, N-1, B) column-major
    x32 = np.zeros((batch, nx), dtype=np.float32)                                    # (nx, B) column-major
    dt = 0.0
    for k in range(inner + 1):                                # (the first loop: code objects, buffers, the first launches)
        bs.reset()
        bs.set_x0(x0)
        t0 = time.perf_counter()
        if arm == "host":
            x = np.ascontiguousarray(x0.T)
            for s in range(steps):
                x32[...] = x
                assert bs.lib.tinympc_set_x0_f32(bs.h, x32.ctypes.data_as(c_fp), batch) == 0
                assert bs.lib.tinympc_solve(bs.h) >= 0
                assert bs.lib.tinympc_get_controls_f32(bs.h, u_all.ctypes.data_as(c_fp)) == 0
                u0 = u_all[:, 0, :].astype(np.float64)
                x = (Ap @ x[:, :, None])[:, :, 0] + (Bp @ u0[:, :, None])[:, :, 0] + w[s]
        else:
            st = bs.lib.tinympc_mpc_rollout(bs.h, steps, ctypes.c_void_p(0))
            assert st >= 0, "mpc_rollout failed"
        if k:
            dt += time.perf_counter() - t0
    print(json.dumps(dict(arm=arm, work=work, launched=bs.last_launch_name, launches=launches(bs.h) if arm != "host" else steps, batch=batch,
                          steps=steps, ms_per_step=round(dt / inner / steps * 1e3, 5))), flush=True)
    bs.close()


def summary(ms):
    s = sorted(ms)
    med = s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])
    return med, (s[-1] - s[0]) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--only", default="", help="one workload instead of the two")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", nargs=3, metavar=("ARM", "WORKLOAD", "STEPS"))
    a = ap.parse_args()
    if a.worker:
        worker(a.worker[0], a.worker[1], a.batch, int(a.worker[2]), a.inner)
        return
    lines, got = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# scripts/plant_loop_rate.py: closed loops against a per-instance plant and disturbance, batch {a.batch}, tolerance 1e-3, max_iter 10, "
        f"warm started; ms per step, a fresh process per run ({a.inner} timed loops behind a warm-up loop), arms alternating")
    workloads = [wl for wl in WORKLOADS if not a.only or wl[0] == a.only]
    for work, steps in workloads:
        for rep in range(a.runs):
            for arm in ARMS:
                e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
                cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--inner", str(a.inner), "--worker", arm, work, str(steps)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=e)
                if p.returncode != 0:
                    print(p.stdout[-2000:], p.stderr[-2000:], flush=True)
                    sys.exit(f"{work} {arm}: exit status {p.returncode}")    # (nothing more is started after a failure)
                r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
                got.setdefault((work, arm), []).append(r["ms_per_step"])
                say(f"{work:9s} {steps:3d} steps run {rep} {arm:5s} {r['launched']:18s} {r['launches']:3d} launch(es): {r['ms_per_step']:.5f}")
    for work, _ in workloads:
        for arm in ARMS:
            med, spread = summary(got[(work, arm)])
            say(f"{work:9s} {arm:5s}: {got[(work, arm)]} median {med:.5f} spread {100 * spread:.1f} %")
        ho, ow, mo = got[(work, "host")], got[(work, "own")], got[(work, "model")]
        say(f"{work:9s}: every run of the own-plant chain below every run of the host-stepped loop: {max(ow) < min(ho)} (host / own, medians: "
            f"{summary(ho)[0] / summary(ow)[0]:.2f}); own / model, medians: {summary(ow)[0] / summary(mo)[0]:.2f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
