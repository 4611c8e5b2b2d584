# A batch of quadrotors following ONE moving position reference: the receding-horizon loop of the reference's examples
# (set_x0 -> set_x_ref of the step -> solve -> apply the first control: examples/cartpole_example_mpc.jl:35-51, with the
# reference shift of examples/rocket_landing_constraints.jl:107-115) through set_ref_sequence + mpc_rollout, the plant stepped on
# the device between the launches.  Problem data: examples/quadrotor_hover_codegen.jl:26-58.
# (Julia is not installed in the build image: this script is written against julia/TinyMPC.jl and has not been executed;
# the same calls run in tests/test_ref_sequence_gpu.py::test_chain_on_mfma through the Python mirror.)
include(joinpath(@__DIR__, "..", "TinyMPC.jl"))
using .TinyMPC
using LinearAlgebra, Random

const NSTATES, NINPUTS, NHORIZON = 12, 4, 30
A = [1.0 0 0 0 0.024525 0 0.05 0 0 0 0.0002044 0;
     0 1.0 0 -0.024525 0 0 0 0.05 0 -0.0002044 0 0;
     0 0 1.0 0 0 0 0 0 0.05 0 0 0;
     0 0 0 1.0 0 0 0 0 0 0.025 0 0;
     0 0 0 0 1.0 0 0 0 0 0 0.025 0;
     0 0 0 0 0 1.0 0 0 0 0 0 0.025;
     0 0 0 0 0.981 0 1.0 0 0 0 0.0122625 0;
     0 0 0 -0.981 0 0 0 1.0 0 -0.0122625 0 0;
     0 0 0 0 0 0 0 0 1.0 0 0 0;
     0 0 0 0 0 0 0 0 0 1.0 0 0;
     0 0 0 0 0 0 0 0 0 0 1.0 0;
     0 0 0 0 0 0 0 0 0 0 0 1.0]
B = [-0.0007069 0.0007773 0.0007091 -0.0007795;
     0.0007034 0.0007747 -0.0007042 -0.0007739;
     0.0052554 0.0052554 0.0052554 0.0052554;
     -0.1720966 -0.1895213 0.1722891 0.1893288;
     -0.1729419 0.190174 0.1734809 -0.1907131;
     0.0123423 -0.0045148 -0.0174024 0.0095748;
     -0.056552 0.0621869 0.0567283 -0.0623632;
     0.0562756 0.0619735 -0.0563386 -0.0619105;
     0.2102143 0.2102143 0.2102143 0.2102143;
     -13.7677303 -15.1617018 13.7831318 15.1463003;
     -13.8353509 15.2139209 13.8784751 -15.2570451;
     0.9873856 -0.361182 -1.392188 0.7659845]
Q = diagm([100.0, 100.0, 100.0, 4.0, 4.0, 400.0, 4.0, 4.0, 4.0, 2.0408163, 2.0408163, 4.0])
R = diagm(fill(4.0, 4))

batch, steps = 65536, 200
solver = TinyMPCSolver()
setup(solver, A, B, zeros(NSTATES), Q, R, 5.0, NSTATES, NINPUTS, NHORIZON; batch=batch, max_iter=10, abs_pri_tol=1e-3, abs_dua_tol=1e-3)
set_bound_constraints(solver, fill(-1e17, NSTATES, NHORIZON), fill(1e17, NSTATES, NHORIZON),
                      fill(-0.5, NINPUTS, NHORIZON - 1), fill(0.5, NINPUTS, NHORIZON - 1))     # the workspace persists (default)

# one trajectory for the whole batch: a circle of radius 0.5 m flown in 10 s (the model's step is 0.05 s), climbing 2 cm/s;
# knot i of step k looks (i + k - 2) model steps ahead of the start — the shift every receding-horizon caller performs
dt, radius, omega, climb = 0.05, 0.5, 2pi / 10.0, 0.02
x_ref_seq = zeros(NSTATES, NHORIZON, steps); u_ref_seq = zeros(NINPUTS, NHORIZON - 1, steps)
for k in 1:steps, i in 1:NHORIZON
    s = (i + k - 2) * dt
    x_ref_seq[1:3, i, k] = [radius * (cos(omega * s) - 1), radius * sin(omega * s), climb * s]                 # position
    x_ref_seq[7:9, i, k] = [-radius * omega * sin(omega * s), radius * omega * cos(omega * s), climb]          # velocity
end
set_ref_sequence(solver, x_ref_seq, u_ref_seq)      # step 1's references become the solver's own

Random.seed!(1)
x0 = zeros(NSTATES, batch)
x0[1:3, :] = 0.1 .* (2 .* rand(3, batch) .- 1)      # every quadrotor starts up to 10 cm off the trajectory's first point
set_x0(solver, x0)
log = mpc_rollout(solver, steps)                    # 200 steps x 65 536 quadrotors; kernel_name() says which family ran them
err = [norm(log.x[1:3, steps, b] - x_ref_seq[1:3, 2, steps]) for b in 1:batch]     # plant after the last step against the knot it was steered to
println("kernel ", kernel_name(), ": tracking error after ", steps, " steps, mean ", sum(err) / batch, " m, worst ", maximum(err),
        " m; mean ADMM iterations per step: ", sum(abs.(log.iter)) / length(log.iter))
