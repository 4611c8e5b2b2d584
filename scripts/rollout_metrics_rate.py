#!/usr/bin/env python3
"""What a Monte-Carlo sweep takes out of a closed loop — per-instance cost, errors, violations, saturation and iteration
statistics and their batch summary — timed per rollout in four arms:

  none     the rollout alone
  fold     set_rollout_metrics once (before the clock), then per loop mpc_rollout alone: the route and rollout_metrics_kernel behind
           it, nothing read back — fold - none is the kernel by itself
  device   set_rollout_metrics once (before the clock), then per loop: mpc_rollout, whose stream carries rollout_metrics_kernel
           behind the route, and get_rollout_summary (the fixed-order fold and 44 doubles to the host)
  host     the only way before: mpc_rollout, get_mpc_log ([batch][steps][nx] and [nu] floats widened to fp64, the iteration
           counts), then the same eleven statistics per instance and their summary in numpy

on two workloads, warm started, tolerance 1e-3, max_iter 10, check_termination 1 (those of profiles/r20_noise_loop.txt):

  cartpole    (4, 1, 20), input bound, 50 steps, its fused loop (one launch)
  quadrotor   (12, 4, 30), 20 steps, the matrix-core chain

    python scripts/rollout_metrics_rate.py [--batch 65536] [--runs 3] [--inner 3] [--only WORKLOAD] [--out profiles/rNN_rollout_metrics.txt]

Weights: the diagonals of Q and R; the safe set: x within +-0.5 of the largest |x0| of each row, u the solver's input bounds
(cartpole) or +-0.4 (quadrotor).  A fresh process per run, the arms alternating, `--runs` runs per arm and workload.  A run is
`--inner` loops behind a warm-up loop, each from a reset workspace, reset accumulators and the same x0, timed with the host clock;
its figure is the mean per ROLLOUT in ms.  Per arm: every run, the median, the spread (max - min) / median; then the one
criterion — every run of `device` below every run of `host` — and, reported and not judged: device - none (the fold's and the
summary's price per rollout) with the log bytes the fold reads divided by that time, and fold - none (the kernel by itself).  The device and host arms' summaries are
printed side by side from the last loop.  Nothing more is started after a run that fails.
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
            "TINYMPC_HIP_STREAM_F64", "TINYMPC_HIP_NO_JIT", "TINYMPC_HIP_NOISE_SPLIT", "TINYMPC_HIP_GROUP")
ARMS = ("none", "fold", "device", "host")
WORKLOADS = (("cartpole", 50), ("quadrotor", 20))


def make(work, batch):
    import numpy as np
    import tinympc_julia_amd as t
    if work == "cartpole":
        prob, x0 = t.problems.cartpole(20, u_bound=0.5), t.problems.cartpole_x0(batch, seed=2)
        u_lim = prob.u_max[:, 0].copy()
    else:
        prob, x0 = t.problems.quadrotor(30), t.problems.quadrotor_x0(batch, seed=1)
        u_lim = np.full(prob.nu, 0.4)
    bs = t.BatchSolver(prob.A, prob.B, prob.Q, prob.R, prob.rho, prob.N, batch=batch)
    bs.update_settings(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=10, check_termination=1)
    bs.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    bs.set_warm_start(True)
    x_lim = 0.5 * np.abs(x0).max(axis=1)
    cfg = dict(qw=np.diag(prob.Q).copy(), rw=np.diag(prob.R).copy(), x_lo=-x_lim, x_hi=x_lim, u_lo=-u_lim, u_hi=u_lim)
    return t, bs, prob, np.asfortranarray(x0), cfg


def host_metrics(np, x, u, it, cfg):
    """the eleven slots per instance from the log as get_mpc_log gives it — x [B][steps][nx], u [B][steps][nu] fp64, it [B][steps]
    signed — vectorised over the batch, and their summary [11][4] (no references here: the targets are zero)"""
    B, steps = it.shape
    m = np.zeros((B, 11))
    err = np.abs(x).max(axis=2)
    viol = np.maximum(np.maximum(x - cfg["x_hi"], cfg["x_lo"] - x).max(axis=2), 0.0)
    out = ((x > cfg["x_hi"]) | (x < cfg["x_lo"])).any(axis=2)
    sat = ((u >= cfg["u_hi"]) | (u <= cfg["u_lo"])).any(axis=2)
    m[:, 0] = steps
    m[:, 1] = (x * x * cfg["qw"]).sum(axis=(1, 2))
    m[:, 2] = (u * u * cfg["rw"]).sum(axis=(1, 2))
    m[:, 3], m[:, 4], m[:, 5] = err.max(axis=1), err[:, -1], viol.max(axis=1)
    m[:, 6] = out.sum(axis=1)
    m[:, 7] = np.where(out.any(axis=1), out.argmax(axis=1) + 1, 0)
    m[:, 8] = sat.sum(axis=1)
    m[:, 9], m[:, 10] = np.abs(it).sum(axis=1), (it < 0).sum(axis=1)
    return m, np.stack([m.sum(axis=0), m.min(axis=0), m.max(axis=0), (m > 0).sum(axis=0).astype(np.float64)], axis=1)


def worker(arm, work, batch, steps, inner):
    import numpy as np
    t, bs, prob, x0, cfg = make(work, batch)
    nx, nu = prob.nx, prob.nu
    launches = ctypes.CDLL(t.LIB_PATH).tmpc_last_rollout_launches
    launches.restype, launches.argtypes = ctypes.c_int, [ctypes.c_void_p]
    c_dp, c_ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    xl, ul, il = np.zeros((batch, steps, nx)), np.zeros((batch, steps, nu)), np.zeros((batch, steps), dtype=np.int32)
    summary = np.zeros((11, 4))
    if arm in ("fold", "device"):
        bs.set_rollout_metrics(True, **cfg)
    dt = 0.0
    for k in range(inner + 1):                                # (the first loop: code objects, buffers, the first launches)
        bs.reset()
        bs.set_x0(x0)
        if arm in ("fold", "device"):
            bs.reset_rollout_metrics()
        t0 = time.perf_counter()
        st = bs.lib.tinympc_mpc_rollout(bs.h, steps, ctypes.c_void_p(0))
        assert st >= 0, "mpc_rollout failed"
        if arm == "device":
            assert bs.lib.tinympc_get_rollout_summary(bs.h, summary.ctypes.data_as(c_dp)) == 0
        elif arm == "host":
            assert bs.lib.tinympc_get_mpc_log(bs.h, xl.ctypes.data_as(c_dp), ul.ctypes.data_as(c_dp), il.ctypes.data_as(c_ip)) == 0
            summary = host_metrics(np, xl, ul, il, cfg)[1]
        if k:
            dt += time.perf_counter() - t0
    print(json.dumps(dict(arm=arm, work=work, launched=bs.last_launch_name, launches=launches(bs.h), batch=batch, steps=steps,
                          ms_per_rollout=round(dt / inner * 1e3, 4), log_bytes=batch * steps * (nx + nu + 1) * 4,
                          summary=[[float(v) for v in row] for row in summary])), flush=True)
    bs.close()


def median_spread(ms):
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
    lines, got, last = [], {}, {}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# scripts/rollout_metrics_rate.py: closed loops with their metrics, batch {a.batch}, tolerance 1e-3, max_iter 10, warm started; ms per rollout, "
        f"a fresh process per run ({a.inner} timed loops behind a warm-up loop), arms alternating")
    workloads = [wl for wl in WORKLOADS if not a.only or wl[0] == a.only]
    for work, steps in workloads:
        for rep in range(a.runs):
            for arm in ARMS:
                e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
                cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--inner", str(a.inner), "--worker", arm, work, str(steps)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=400, env=e)
                if p.returncode != 0:
                    print(p.stdout[-2000:], p.stderr[-2000:], flush=True)
                    sys.exit(f"{work} {arm}: exit status {p.returncode}")    # (nothing more is started after a failure)
                r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
                got.setdefault((work, arm), []).append(r["ms_per_rollout"])
                last[(work, arm)] = r
                say(f"{work:9s} {steps:3d} steps run {rep} {arm:6s} {r['launched']:18s} {r['launches']:3d} launch(es): {r['ms_per_rollout']:.4f}")
    for work, steps in workloads:
        med = {}
        for arm in ARMS:
            med[arm], spread = median_spread(got[(work, arm)])
            say(f"{work:9s} {arm:6s}: {got[(work, arm)]} median {med[arm]:.4f} spread {100 * spread:.1f} %")
        ho, de = got[(work, "host")], got[(work, "device")]
        price, kernel = med["device"] - med["none"], med["fold"] - med["none"]
        nbytes = last[(work, "device")]["log_bytes"]
        say(f"{work:9s}: every run of the device arm below every run of the host arm: {max(de) < min(ho)} (host / device, medians: {med['host'] / med['device']:.2f})")
        say(f"{work:9s}: the fold's and the summary's price, device - none of the medians: {1e3 * price:.1f} us per rollout; the log it reads: "
            f"{nbytes / 1e6:.1f} MB" + (f", {nbytes / (price * 1e-3) / 1e9:.0f} GB/s over that time" if price > 0 else " (no positive difference to divide by)"))
        say(f"{work:9s}: the fold kernel by itself, fold - none of the medians: {1e3 * kernel:.1f} us per rollout" +
            (f", {nbytes / (kernel * 1e-3) / 1e9:.0f} GB/s of log" if kernel > 0 else " (inside the spread)"))
        sd, sh = last[(work, "device")]["summary"], last[(work, "host")]["summary"]
        for k, name in enumerate(("steps", "cost_x", "cost_u", "peak_err", "final_err", "x_viol_max", "x_viol_steps", "first_viol", "u_sat_steps", "iters", "maxiter_steps")):
            say(f"{work:9s}   {name:13s} device sum {sd[k][0]:.9g} min {sd[k][1]:.6g} max {sd[k][2]:.6g} count {sd[k][3]:.0f} | host sum {sh[k][0]:.9g} min {sh[k][1]:.6g} "
                f"max {sh[k][2]:.6g} count {sh[k][3]:.0f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
