"""TEST INFRASTRUCTURE ONLY — writes tests/golden/G10_cartpole_tracking_loop.json from the compiled reference snapshot
(oracle.cpu_oracle.CpuSolver("ref", ...); CPU only, run where the snapshot is built):

    python scripts/make_golden_tracking.py

The cartpole example's closed loop (examples/cartpole_example_mpc.jl:35-51) with an input bound and a reference that moves
every step, the way the rocket example shifts its own (examples/rocket_landing_constraints.jl:107-115): before the solve
of step k the caller sets x_ref[:, i] with the cart position on a ramp in i + k (and a small input reference that moves
with it), then solves warm-started and applies the first control to the model.

Layout as G5 (settings, x0, per step x0 / iter / solved / u / status ...), plus the reference sequence itself:
x_ref_seq (nx, N, steps) and u_ref_seq (nu, N-1, steps), flattened column-major like every other array of the fixtures.
"""
import json
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

from oracle import make_golden as mg  # noqa: E402  (the fixtures' own helpers: one layout, one flattening)

NAME = "G10_cartpole_tracking_loop"
N, STEPS = 10, 12
SETTINGS = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=30, check_termination=1)
X0 = [0.3, 0.0, 0.05, 0.0]
U_BOUND = 0.5
RAMP = 0.005         # cart position reference per knot and per step


def tracking_refs(nx, nu, N, steps, ramp=RAMP):
    """x_ref_seq (nx, N, steps), u_ref_seq (nu, N-1, steps): knot i of step k (both 0-based) asks for the cart at
    ramp * (i + k) and for a small input that fades along the same ramp"""
    xs, us = np.zeros((nx, N, steps)), np.zeros((nu, N - 1, steps))
    for k in range(steps):
        for i in range(N):
            xs[0, i, k] = ramp * (i + k)
            if i < N - 1:
                us[0, i, k] = 0.05 - 0.002 * (i + k)
    return xs, us


def case_tracking():
    prob = mg.P.cartpole(N, u_bound=U_BOUND)
    xs, us = tracking_refs(prob.nx, prob.nu, N, STEPS)
    s = mg._mk(prob, SETTINGS)
    x = np.array(X0, dtype=np.float64)
    seq = []
    for k in range(STEPS):
        s.set_x0(x)
        s.set_x_ref(xs[:, :, k])
        s.set_u_ref(us[:, :, k])
        st = s.solve()
        o = mg._sol(s, st)
        o["x0"] = mg._l(x)
        seq.append(o)
        x = prob.A @ x + prob.B @ np.array(o["u"][: prob.nu])
    s.close()
    return dict(case=NAME, note="cartpole_example_mpc.jl:35-51 with an input bound and set_x_ref / set_u_ref of a moving "
                                "reference before every solve (as rocket_landing_constraints.jl:107-115 shifts its own)",
                problem=mg._prob_dict(prob), settings=SETTINGS, x0=mg._l(X0), x_ref_seq=mg._l(xs), u_ref_seq=mg._l(us),
                steps=seq)


def main():
    mg.build(port=False, ref=True)
    c = case_tracking()
    path = os.path.join(mg.OUT, NAME + ".json")
    with open(path, "w") as f:
        json.dump(c, f)
    its = [(o["iter"], o["solved"]) for o in c["steps"]]
    sat = [abs(abs(o["u"][0]) - U_BOUND) < 1e-12 for o in c["steps"]]
    print(f"{NAME}: {os.path.getsize(path)} bytes; (iter, solved) per step {its}; first control on the bound: {sat}")


if __name__ == "__main__":
    main()
