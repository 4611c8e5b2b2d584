#!/usr/bin/env python3
"""The closed loop under output feedback — both noises, measured outputs y = C x + v, a fixed-gain state estimator — timed per step
in these arms:

  host     the only way before set_estimator: the loop a caller steps itself, the draws from get_noise (both kinds, fetched inside
           the clock as a sweep would fetch them), the estimator in batched numpy (fp64), per step set_x0_f32 -> solve ->
           get_controls_f32, the plant step in numpy
  device   set_estimator once, then mpc_rollout: estimator_step_kernel on the chain, predict and the next step's correct fused
  split    the same under TINYMPC_HIP_ESTIMATOR_SPLIT=1: predict and correct as two launches a step (the A/B of the two forms)
  noest    the same chain with both noises and no estimator (the solves from float32(x + v)): device - noest per step is the
           estimator's price

on two workloads, warm started, tolerance 1e-3, max_iter 10, check_termination 1 (those of profiles/r20_noise_loop.txt):

  cartpole    (4, 1, 20), input bound, ny = 2 (cart position, pole angle), 50 steps
  quadrotor   (12, 4, 30), ny = 6 (the pose rows), 20 steps

    python scripts/estimator_loop_rate.py [--batch 65536] [--runs 3] [--inner 3] [--only WORKLOAD] [--out profiles/rNN_estimator_loop.txt]

G_w = G_v = diag(0.003 scale_r), scale_r the largest |x0| of the row over the batch; L = kalman_gain(A, C, G_w, G_v); the initial
estimate is x0.  A fresh process per run, the arms alternating, `--runs` runs per arm and workload.  A run is `--inner` loops behind a
warm-up loop, each from a reset workspace, the same x0, cursor 0 and a re-armed estimate, timed with the host clock; its figure is
the mean per step.  Per arm: ms per step of every run, the median, the spread (max - min) / median; then the one criterion — every
run of `device` below every run of `host` — and, reported and not judged: device - noest (the estimator's price per step) and
split - device, each beside the spreads of its two arms.  Nothing more is started after a run that fails.
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
            "TINYMPC_HIP_STREAM_F64", "TINYMPC_HIP_NO_JIT", "TINYMPC_HIP_NOISE_SPLIT", "TINYMPC_HIP_ESTIMATOR_SPLIT")
ARMS = ("host", "device", "split", "noest")
WORKLOADS = (("cartpole", 50), ("quadrotor", 20))


def make(work, batch):
    import numpy as np
    import tinympc_julia_amd as t
    if work == "cartpole":
        prob, x0, rows = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(batch, seed=2), [0, 2]
    else:
        prob, x0, rows = t.problems.quadrotor(30), t.problems.quadrotor_x0(batch, seed=1), [0, 1, 2, 3, 4, 5]
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=batch)
    bs.update_settings(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=10, check_termination=1)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(True)
    sig = 0.003 * np.abs(x0).max(axis=1)
    C = np.eye(prob.nx)[rows]
    return t, bs, prob, np.asfortranarray(x0), sig, C, t.kalman_gain(prob.A, C, sig, sig)


def worker(arm, work, batch, steps, inner):
    import numpy as np
    t, bs, prob, x0, sig, C, L = make(work, batch)
    nx, nu, N, ny = prob.nx, prob.nu, prob.N, C.shape[0]
    launches = ctypes.CDLL(t.LIB_PATH).tmpc_last_rollout_launches
    launches.restype, launches.argtypes = ctypes.c_int, [ctypes.c_void_p]
    c_fp = ctypes.POINTER(ctypes.c_float)
    u_all = np.zeros((batch, N - 1, nu), dtype=np.float32)                           # (nu, N-1, B) column-major
    x32 = np.zeros((batch, nx), dtype=np.float32)                                    # (nx, B) column-major
    bs.set_process_noise(sig, 1000)
    bs.set_measurement_noise(sig, 2000)
    if arm in ("device", "split"):
        bs.set_estimator(C, L)
    dt = 0.0
    for k in range(inner + 1):                                # (the first loop: code objects, buffers, the first launches)
        bs.reset()
        bs.set_x0(x0)
        bs.set_noise_cursor(0)
        if arm in ("device", "split"):
            bs.set_estimator_state(None)
        t0 = time.perf_counter()
        if arm == "host":
            nw, nv = bs.get_noise(0, 0, steps).T, bs.get_noise(1, 0, steps).T       # (B, steps, nx) views of the library's layout
            x = np.ascontiguousarray(x0.T)
            xh = x.copy()
            for s in range(steps):
                y = x @ C.T + nv[:, s, :ny]
                xh = xh + (y - xh @ C.T) @ L.T
                x32[...] = xh
                assert bs.lib.tinympc_set_x0_f32(bs.h, x32.ctypes.data_as(c_fp), batch) == 0
                assert bs.lib.tinympc_solve(bs.h) >= 0
                assert bs.lib.tinympc_get_controls_f32(bs.h, u_all.ctypes.data_as(c_fp)) == 0
                u0 = u_all[:, 0, :].astype(np.float64)
                x = x @ prob.A.T + u0 @ prob.B.T + nw[:, s, :]
                xh = xh @ prob.A.T + u0 @ prob.B.T
        else:
            st = bs.lib.tinympc_mpc_rollout(bs.h, steps, ctypes.c_void_p(0))
            assert st >= 0, "mpc_rollout failed"
            assert bs.lib.tinympc_solve_status(bs.h) >= 0                            # (waits for the chain: the clock covers its run)
        if k:
            dt += time.perf_counter() - t0
    if arm != "host":
        assert bs.noise_cursor() == steps and bs.noise_mode() == 5 and bs.estimator_mode() == (0 if arm == "noest" else 1)
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

    say(f"# scripts/estimator_loop_rate.py: closed loops under output feedback, batch {a.batch}, tolerance 1e-3, max_iter 10, warm started; ms per step, "
        f"a fresh process per run ({a.inner} timed loops behind a warm-up loop), arms alternating")
    workloads = [wl for wl in WORKLOADS if not a.only or wl[0] == a.only]
    for work, steps in workloads:
        for rep in range(a.runs):
            for arm in ARMS:
                e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
                if arm == "split":
                    e["TINYMPC_HIP_ESTIMATOR_SPLIT"] = "1"
                cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--inner", str(a.inner), "--worker", arm, work, str(steps)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=400, env=e)
                if p.returncode != 0:
                    print(p.stdout[-2000:], p.stderr[-2000:], flush=True)
                    sys.exit(f"{work} {arm}: exit status {p.returncode}")    # (nothing more is started after a failure)
                r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
                got.setdefault((work, arm), []).append(r["ms_per_step"])
                say(f"{work:9s} {steps:3d} steps run {rep} {arm:7s} {r['launched']:18s} {r['launches']:3d} launch(es): {r['ms_per_step']:.5f}")
    for work, steps in workloads:
        med, spread = {}, {}
        for arm in ARMS:
            med[arm], spread[arm] = summary(got[(work, arm)])
            say(f"{work:9s} {arm:7s}: {got[(work, arm)]} median {med[arm]:.5f} spread {100 * spread[arm]:.1f} %")
        ho, de = got[(work, "host")], got[(work, "device")]
        us = lambda arm: 1e3 * spread[arm] * med[arm]      # noqa: E731  (an arm's max - min, in us)
        say(f"{work:9s}: every run of the device arm below every run of the host arm: {max(de) < min(ho)} (host / device, medians: "
            f"{med['host'] / med['device']:.2f})")
        say(f"{work:9s}: the estimator's price, device - noest of the medians: {1e3 * (med['device'] - med['noest']):+.1f} us per step "
            f"(the arms' own max - min: {us('device'):.1f} / {us('noest'):.1f} us)")
        say(f"{work:9s}: predict and correct as two launches, split - device of the medians: {1e3 * (med['split'] - med['device']):+.1f} us per step "
            f"(the arms' own max - min: {us('split'):.1f} / {us('device'):.1f} us)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
