#!/usr/bin/env python3
"""The closed loop under seeded noise — a Monte-Carlo sweep's inner loop — timed per step in these arms:

  hostdrawn  the only way before set_process_noise: rng.standard_normal . G in numpy, [batch][steps][nx] doubles, set_disturbance,
             mpc_rollout; timed from the draw to the end of the loop
  device     set_process_noise once, then mpc_rollout: plant_step_kernel<true> draws on the device; timed from the setter's call
             (a seed per loop, as a sweep would set one) to the end of the loop
  resident   the rollout alone with the disturbance already resident (set before the clock starts): device - resident per step
             is what the generator costs over reading an uploaded row
  both       process and measurement noise on the device, the next step's measurement drawn by the plant-step kernel
  split      the same under TINYMPC_HIP_NOISE_SPLIT=1: measure_kernel ahead of every launch (the A/B of the two forms)
  hostboth   the loop a caller steps itself with both noises: per step a measurement draw in numpy, set_x0_f32 -> solve ->
             get_controls_f32, the plant step and the process draw in numpy (fp64)

on two workloads, warm started, tolerance 1e-3, max_iter 10, check_termination 1 (those of profiles/r18_plant_loop.txt):

  cartpole    (4, 1, 20), input bound, 50 steps
  quadrotor   (12, 4, 30), 20 steps

    python scripts/noise_loop_rate.py [--batch 65536] [--runs 3] [--inner 3] [--only WORKLOAD] [--out profiles/rNN_noise_loop.txt]

G = diag(0.003 scale_r), scale_r the largest |x0| of the row over the batch.  A fresh process per run, the arms alternating,
`--runs` runs per arm and workload.  A run is `--inner` loops behind a warm-up loop, each from a reset workspace, the same x0
and cursor 0, timed with the host clock; its figure is the mean per step.  Per arm: ms per step of every run, the median, the
spread (max - min) / median; then the one criterion — every run of `device` below every run of `hostdrawn` — and, reported and
not judged: device - resident (the generator's price per step), both against split, both against hostboth.  Nothing more is
started after a run that fails.
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
            "TINYMPC_HIP_STREAM_F64", "TINYMPC_HIP_NO_JIT", "TINYMPC_HIP_NOISE_SPLIT")
ARMS = ("hostdrawn", "device", "resident", "both", "split", "hostboth")
WORKLOADS = (("cartpole", 50), ("quadrotor", 20))


def make(work, batch):
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
    return t, bs, prob, np.asfortranarray(x0), 0.003 * np.abs(x0).max(axis=1)


def worker(arm, work, batch, steps, inner):
    import numpy as np
    t, bs, prob, x0, sig = make(work, batch)
    nx, nu, N = prob.nx, prob.nu, prob.N
    launches = ctypes.CDLL(t.LIB_PATH).tmpc_last_rollout_launches
    launches.restype, launches.argtypes = ctypes.c_int, [ctypes.c_void_p]
    c_fp = ctypes.POINTER(ctypes.c_float)
    rng = np.random.default_rng(20)
    u_all = np.zeros((batch, N - 1, nu), dtype=np.float32)                           # (nu, N-1, B) column-major
    x32 = np.zeros((batch, nx), dtype=np.float32)                                    # (nx, B) column-major
    if arm == "resident":
        bs.set_disturbance(np.asfortranarray((rng.standard_normal((batch, steps, nx)) * sig).transpose(2, 1, 0)))
    dt = 0.0
    for k in range(inner + 1):                                # (the first loop: code objects, buffers, the first launches)
        bs.reset()
        bs.set_x0(x0)
        if arm in ("device", "both", "split"):
            bs.set_noise_cursor(0)
        t0 = time.perf_counter()
        if arm == "hostdrawn":
            w = rng.standard_normal((batch, steps, nx)) * sig                        # [batch][steps][nx], the library's layout
            assert bs.lib.tinympc_set_disturbance(bs.h, w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), steps, 1) == 0
        elif arm == "device":
            bs.set_process_noise(sig, 1000 + k)
        elif arm in ("both", "split"):
            bs.set_process_noise(sig, 1000 + k)
            bs.set_measurement_noise(sig, 2000 + k)
        if arm == "hostboth":
            x = np.ascontiguousarray(x0.T)
            for s in range(steps):
                x32[...] = x + rng.standard_normal((batch, nx)) * sig
                assert bs.lib.tinympc_set_x0_f32(bs.h, x32.ctypes.data_as(c_fp), batch) == 0
                assert bs.lib.tinympc_solve(bs.h) >= 0
                assert bs.lib.tinympc_get_controls_f32(bs.h, u_all.ctypes.data_as(c_fp)) == 0
                u0 = u_all[:, 0, :].astype(np.float64)
                x = x @ prob.A.T + u0 @ prob.B.T + rng.standard_normal((batch, nx)) * sig
        else:
            st = bs.lib.tinympc_mpc_rollout(bs.h, steps, ctypes.c_void_p(0))
            assert st >= 0, "mpc_rollout failed"
        if k:
            dt += time.perf_counter() - t0
    if arm in ("device", "both", "split"):
        assert bs.noise_cursor() == steps and bs.noise_mode() == (1 if arm == "device" else 5)
    print(json.dumps(dict(arm=arm, work=work, launched=bs.last_launch_name, launches=launches(bs.h) if arm != "hostboth" else steps, batch=batch,
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

    say(f"# scripts/noise_loop_rate.py: closed loops under seeded noise, batch {a.batch}, tolerance 1e-3, max_iter 10, warm started; ms per step, "
        f"a fresh process per run ({a.inner} timed loops behind a warm-up loop), arms alternating")
    workloads = [wl for wl in WORKLOADS if not a.only or wl[0] == a.only]
    for work, steps in workloads:
        for rep in range(a.runs):
            for arm in ARMS:
                e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
                if arm == "split":
                    e["TINYMPC_HIP_NOISE_SPLIT"] = "1"
                cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--inner", str(a.inner), "--worker", arm, work, str(steps)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=400, env=e)
                if p.returncode != 0:
                    print(p.stdout[-2000:], p.stderr[-2000:], flush=True)
                    sys.exit(f"{work} {arm}: exit status {p.returncode}")    # (nothing more is started after a failure)
                r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
                got.setdefault((work, arm), []).append(r["ms_per_step"])
                say(f"{work:9s} {steps:3d} steps run {rep} {arm:9s} {r['launched']:18s} {r['launches']:3d} launch(es): {r['ms_per_step']:.5f}")
    for work, steps in workloads:
        med = {}
        for arm in ARMS:
            med[arm], spread = summary(got[(work, arm)])
            say(f"{work:9s} {arm:9s}: {got[(work, arm)]} median {med[arm]:.5f} spread {100 * spread:.1f} %")
        ho, de = got[(work, "hostdrawn")], got[(work, "device")]
        say(f"{work:9s}: every run of the device arm below every run of the host-drawn arm: {max(de) < min(ho)} (hostdrawn / device, medians: "
            f"{med['hostdrawn'] / med['device']:.2f}); the generator's price, device - resident of the medians: "
            f"{1e3 * (med['device'] - med['resident']):.1f} us per step")
        say(f"{work:9s}: both noises, the next measurement drawn by the plant-step kernel {med['both']:.5f}, by a kernel of its own {med['split']:.5f} "
            f"({1e3 * (med['split'] - med['both']):+.1f} us per step); the host-stepped loop {med['hostboth']:.5f} ({med['hostboth'] / med['both']:.1f}x)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
