"""Idle time between consecutive launches of the headline kernel, from rocprofv3 --kernel-trace CSVs (one run of
bench.py --gpus 1 --steps 20 --warmup 5 under the profiler): gap = start[i + 1] - end[i] over launches that follow each other
without a host synchronisation in between (gaps above 50 us are the host's: warm-up solves are synchronised one by one), and
the kernel's own duration.  usage: trace_gaps.py DIR_OR_CSV [kernel-name substring, default admm_lean_kernel]"""
import csv, glob, os, sys
import numpy as np
src = sys.argv[1]
want = sys.argv[2] if len(sys.argv) > 2 else "admm_lean_kernel"
files = [src] if os.path.isfile(src) else sorted(glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True))
for f in files:
    rows = [r for r in csv.DictReader(open(f)) if want in r["Kernel_Name"]]
    if len(rows) < 3:
        continue
    t0 = np.array([int(r["Start_Timestamp"]) for r in rows], dtype=np.int64)
    t1 = np.array([int(r["End_Timestamp"]) for r in rows], dtype=np.int64)
    o = np.argsort(t0)
    t0, t1 = t0[o], t1[o]
    gap = (t0[1:] - t1[:-1]) * 1e-3
    dur = (t1 - t0) * 1e-3
    q = gap[gap < 50.0]                                          # queued back to back
    tail = gap[-19:]                                             # the 20 timed steps are the last launches of the run
    print(f"{os.path.basename(f)}: {len(rows)} launches of {want}; duration median {np.median(dur):.2f} us (min {dur.min():.2f}, max {dur.max():.2f}; last 20: {np.median(dur[-20:]):.2f});")
    print(f"  gap between launches queued back to back ({len(q)} of {len(gap)} below 50 us): median {np.median(q):.2f} us, min {q.min():.2f}, max {q.max():.2f}; "
          f"the last 19 gaps (the timed steps): median {np.median(tail):.2f}, min {tail.min():.2f}, max {tail.max():.2f}; "
          f"start to start over them {np.median(np.diff(t0[-20:])) * 1e-3:.2f} us")
