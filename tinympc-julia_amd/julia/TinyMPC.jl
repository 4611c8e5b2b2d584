module TinyMPC

# Julia host side of the MI355X batched TinyMPC engine.
#
# Keeps the surface of the reference module (reference: src/TinyMPC.jl:3-6,34-292):
#   TinyMPCSolver / setup / set_x0 / set_x_ref / set_u_ref / set_bound_constraints /
#   update_settings / set_cache_terms / solve / get_solution
# and reaches the solver the same way — `ccall((:sym, libpath), Int32, ...)` by symbol name into a
# C-ABI shared library — but the library is libtinympc_hip.so (include/tinympc_hip.h) instead of
# libtinympc_jl built from src/bindings.cpp.  A batch dimension is added:
#   setup(...; batch=B)
#   set_x0(solver, x0)        x0 :: Vector (broadcast) or Matrix (nx, B)
#   set_x_ref(solver, xref)   Matrix (nx, N) shared, or Array{Float64,3} (nx, N, B)
#   get_solution(solver)      states (nx, N) for B == 1 (the reference's shape), else (nx, N, B)
#   get_status(solver)        per-instance iter / solved / residuals
#
# NOTE: the Julia toolchain is absent from the image this repository is built and tested in, so this
# file has not been executed there; the C-ABI it binds is exercised call-for-call by the Python
# mirror (tinympc-julia_amd/tinympc.py) in tests/.  INTEGRATION.md shows the two-line change that
# makes the reference's own src/TinyMPC.jl use this library without adopting this module.

export TinyMPCSolver, setup, solve, get_solution, get_solution!, pin_host!, unpin_host!, get_status, set_x0, set_x_ref, set_u_ref, set_ref_sequence, mpc_rollout, set_plant, set_disturbance, plant_mode, set_ref_trajectory, set_ref_cursor, ref_cursor, set_process_noise, set_measurement_noise, set_noise_cursor, noise_cursor, noise_mode, get_noise, host_noise, set_estimator, set_estimator_state, estimator_mode, get_estimator_state, host_estimator_step, kalman_gain, set_rollout_metrics, reset_rollout_metrics, get_rollout_metrics, get_rollout_summary, METRIC_NAMES, set_instance_bounds, set_instance_linear, set_instance_cones!, setup_families, set_families!, family_cache, families_setup_mode,
       set_bound_constraints, set_linear_constraints, set_equality_constraints, set_cone_constraints, update_settings,
       set_cache_terms, set_batch_size, set_gpus, get_gpus, set_warm_start, set_precision, kernel_name, reset_workspace, print_problem_data,
       compute_sensitivity_autograd, set_sensitivity, get_adaptive_rho

using LinearAlgebra, Libdl, Printf

const _lib = Ref{String}(joinpath(dirname(@__DIR__), "lib", "libtinympc_hip." * Libdl.dlext))
_lib_path() = _lib[]
set_library_path!(p::AbstractString) = (_lib[] = String(p))
_ensure_loaded() = isfile(_lib_path()) || error("TinyMPC library not found: $(_lib_path())")
_last_error() = unsafe_string(ccall((:tinympc_last_error, _lib_path()), Cstring, ()))

mutable struct TinyMPCSolver
    nx::Int
    nu::Int
    N::Int
    batch::Int
    rho::Float64
    is_setup::Bool
    A::Matrix{Float64}
    B::Matrix{Float64}
    Q::Matrix{Float64}
    R::Matrix{Float64}
    TinyMPCSolver() = new(0, 0, 0, 1, 0.0, false, zeros(0, 0), zeros(0, 0), zeros(0, 0), zeros(0, 0))
end

# ---- small helpers ---------------------------------------------------------------------------
# every matrix crosses the boundary as (pointer, rows, cols), column-major Float64 — Julia's own layout
_mat(a::AbstractMatrix{Float64}) = Matrix(a)
_mat(a::AbstractVector{Float64}) = reshape(collect(a), length(a), 1)
_mat(a::AbstractArray{Float64,3}) = reshape(Array(a), size(a, 1), size(a, 2) * size(a, 3))  # (rows, knots*batch)
_flag(b::Bool) = Int32(b ? 1 : 0)
_need(solver) = solver.is_setup || error("Solver not setup")
_ok(status, what) = status == 0 ? status : error("$what ($(_last_error()))")

"""
    setup(solver, A, B, f, Q, R, rho, nx, nu, N; batch=1, kwargs...)

Same call as the reference (src/TinyMPC.jl:55-112) plus `batch`.  The infinite-horizon Riccati
precompute runs on the host in Float64 inside the library; a non-zero `f` (affine dynamics) is honoured
but its parity with the upstream solver is unpinned (DESIGN.md §6).  Settings are then
pushed with every `en_*` flag false, exactly like the reference (src/TinyMPC.jl:89-104).
"""
function setup(solver::TinyMPCSolver, A::Matrix{Float64}, B::Matrix{Float64}, f::Vector{Float64},
               Q::Matrix{Float64}, R::Matrix{Float64}, rho::Float64, nx::Int, nu::Int, N::Int;
               batch::Int=1, verbose::Bool=false, abs_pri_tol::Float64=1e-3, abs_dua_tol::Float64=1e-3,
               max_iter::Int=100, check_termination::Bool=true, adaptive_rho::Bool=false,
               adaptive_rho_min::Float64=0.1, adaptive_rho_max::Float64=10.0,
               adaptive_rho_clipping::Bool=true)
    _ensure_loaded()
    solver.nx, solver.nu, solver.N, solver.rho, solver.batch = nx, nu, N, rho, batch
    solver.A, solver.B, solver.Q, solver.R = copy(A), copy(B), copy(Q), copy(R)
    fm = _mat(f)
    status = ccall((:setup_solver, _lib_path()), Int32,
                   (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32,
                    Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Float64, Int32, Int32, Int32, Int32),
                   A, size(A, 1), size(A, 2), B, size(B, 1), size(B, 2), fm, size(fm, 1), size(fm, 2),
                   Q, size(Q, 1), size(Q, 2), R, size(R, 1), size(R, 2), rho, nx, nu, N, _flag(verbose))
    status == 0 || error("Setup failed with status: $status ($(_last_error()))")
    batch == 1 || _ok(ccall((:set_batch_size, _lib_path()), Int32, (Int32,), batch), "Failed to set batch size")
    solver.is_setup = true
    update_settings(solver; abs_pri_tol=abs_pri_tol, abs_dua_tol=abs_dua_tol, max_iter=max_iter,
                    check_termination=check_termination, adaptive_rho=adaptive_rho,
                    adaptive_rho_min=adaptive_rho_min, adaptive_rho_max=adaptive_rho_max,
                    adaptive_rho_enable_clipping=adaptive_rho_clipping, verbose=verbose)
    verbose && @printf("TinyMPC solver setup successful (nx=%d, nu=%d, N=%d, batch=%d)\n", nx, nu, N, batch)
    return status
end

function set_batch_size(solver::TinyMPCSolver, batch::Int)
    _need(solver)
    _ok(ccall((:set_batch_size, _lib_path()), Int32, (Int32,), batch), "Failed to set batch size")
    solver.batch = batch
    return 0
end

# One problem family PER INSTANCE: a parameter sweep, a fleet of unlike vehicles, a Monte-Carlo run over model error.  A (nx, nx,
# batch), B (nx, nu, batch), Q (nx, nx, batch), R (nu, nu, batch), rho (batch,); every instance gets its own Riccati cache — computed
# on the host, or with on_device=true by a kernel (the same recursion; the route for large batches).  Replaces setup(): settings are
# pushed with every en_* flag false, bounds, references and the closed loop behave as on a single-family solver.  Needs (nx, nu)
# in the stream kernel's grid (nx in {2,3,4,6,8,10,12}, nu <= 4); the batch is fixed.  solver.A / B / Q / R hold instance 1's.
# (Written against the C-ABI like the rest of this file, not executed here.)
function setup_families(solver::TinyMPCSolver, A::Array{Float64,3}, B::Array{Float64,3}, Q::Array{Float64,3}, R::Array{Float64,3},
                        rho::Vector{Float64}, N::Int; on_device::Bool=false, verbose::Bool=false, abs_pri_tol::Float64=1e-3,
                        abs_dua_tol::Float64=1e-3, max_iter::Int=100, check_termination::Bool=true)
    _ensure_loaded()
    nx, nu, batch = size(A, 1), size(B, 2), size(A, 3)
    Am, Bm, Qm, Rm = _mat(A), _mat(B), _mat(Q), _mat(R)
    status = ccall((:setup_families, _lib_path()), Int32,
                   (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32,
                    Ptr{Float64}, Int32, Int32, Int32, Int32, Int32, Int32, Int32),
                   Am, size(Am, 1), size(Am, 2), Bm, size(Bm, 1), size(Bm, 2), Qm, size(Qm, 1), size(Qm, 2), Rm, size(Rm, 1), size(Rm, 2),
                   rho, length(rho), nx, nu, N, batch, _flag(on_device), _flag(verbose))
    status == 0 || error("Setup failed with status: $status ($(_last_error()))")
    solver.nx, solver.nu, solver.N, solver.rho, solver.batch = nx, nu, N, rho[1], batch
    solver.A, solver.B, solver.Q, solver.R = A[:, :, 1], B[:, :, 1], Q[:, :, 1], R[:, :, 1]
    solver.is_setup = true
    update_settings(solver; abs_pri_tol=abs_pri_tol, abs_dua_tol=abs_dua_tol, max_iter=max_iter, check_termination=check_termination,
                    verbose=verbose)
    return status
end

# Replaces EVERY instance's family on a family solver: re-linearisation along a trajectory, gain scheduling, a sweep over rho.  A
# and B come together, so do Q and R; what is nothing is kept.  The caches are recomputed on the device; settings, bounds, rows,
# cones, references, the closed loop's configuration and the warm-start workspace are kept.  Fails, the solver unchanged, where
# some instance's R + B'PB is singular (the error names the first such instance and their count).
function set_families!(solver::TinyMPCSolver; A::Union{Array{Float64,3},Nothing}=nothing, B::Union{Array{Float64,3},Nothing}=nothing,
                       Q::Union{Array{Float64,3},Nothing}=nothing, R::Union{Array{Float64,3},Nothing}=nothing,
                       rho::Union{Vector{Float64},Nothing}=nothing)
    _need(solver)
    ((A === nothing) != (B === nothing) || (Q === nothing) != (R === nothing)) && error("set_families!: A and B come together, and so do Q and R")
    want = Dict(:A => (solver.nx, solver.nx), :B => (solver.nx, solver.nu), :Q => (solver.nx, solver.nx), :R => (solver.nu, solver.nu))
    for (name, m) in ((:A, A), (:B, B), (:Q, Q), (:R, R))
        m === nothing || size(m) == (want[name]..., solver.batch) || error("set_families!: $name must be $((want[name]..., solver.batch))")
    end
    rho === nothing || length(rho) == solver.batch || error("set_families!: rho must have one entry per instance")
    p(m) = m === nothing ? Ptr{Float64}(C_NULL) : pointer(m)
    GC.@preserve A B Q R rho begin
        _ok(ccall((:set_families, _lib_path()), Int32, (Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                  p(A), p(B), p(Q), p(R), p(rho)), "Failed to set the families")
    end
    if A !== nothing
        solver.A, solver.B = A[:, :, 1], B[:, :, 1]
    end
    if Q !== nothing
        solver.Q, solver.R = Q[:, :, 1], R[:, :, 1]
    end
    rho === nothing || (solver.rho = rho[1])
    return 0
end

# the Riccati caches of instances first .. first + count - 1 (1-based) of a family solver, whichever way it was set up:
# (Kinf (nu, nx, n), Pinf (nx, nx, n), Quu_inv (nu, nu, n), AmBKt (nx, nx, n), sweeps (n,) — 1000: the instance stopped at the cap)
function family_cache(solver::TinyMPCSolver; first::Integer=1, count::Union{Integer,Nothing}=nothing)
    _need(solver)
    n = count === nothing ? solver.batch - first + 1 : Int(count)
    K, P = zeros(solver.nu, solver.nx, n), zeros(solver.nx, solver.nx, n)
    Qi, Am = zeros(solver.nu, solver.nu, n), zeros(solver.nx, solver.nx, n)
    sweeps = zeros(Int32, n)
    _ok(ccall((:get_family_cache, _lib_path()), Int32, (Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
              first - 1, n, K, P, Qi, Am, sweeps), "Failed to get the family caches")
    return (Kinf=K, Pinf=P, Quu_inv=Qi, AmBKt=Am, sweeps=sweeps)
end

# 0: not a family solver, 1: families set up on the host, 2: on the device
function families_setup_mode(solver::TinyMPCSolver)
    _need(solver)
    m = ccall((:families_setup_mode, _lib_path()), Int32, ())
    m < 0 && error("families_setup_mode failed ($(_last_error()))")
    return Int(m)
end

# Spread the solver's batch over GPUs 0 .. n-1 of the node in contiguous shards (n = 1: back to one device).  Every
# other call is unchanged and acts on the whole batch; solve() returns 0 iff every instance on every GPU converged
# (the status block is folded over RCCL).  include/tinympc_hip.h section 3, INTEGRATION.md section 4.
function set_gpus(solver::TinyMPCSolver, n::Integer)
    _need(solver)
    _ok(ccall((:set_gpus, _lib_path()), Int32, (Int32,), Int32(n)), "Failed to set the number of GPUs")
    return 0
end
get_gpus() = Int(ccall((:get_gpus, _lib_path()), Int32, ()))

# on = false: every solve() starts from the zero workspace and keeps none (one-shot solves: the benchmark regime, served by
# the on-chip kernels); true (default): the reference's semantics, the workspace persists between solves
# Arithmetic of the solver: 0 = fp64 recurrences over fp32 state (default, 1e-5 of the reference), 1 = all fp32 (faster on
# shapes without a matrix-core kernel, does not hold 1e-5 on every instance), 2 = fp64 end to end like the reference
# (types.hpp:15) — for validation against the CPU solver; slow.  mpc_rollout fails at precision 2 unless the library's
# TINYMPC_HIP_STREAM_MPC=1 is in the environment at setup (see mpc_rollout).
function set_precision(solver::TinyMPCSolver, precision::Integer)
    _need(solver)
    _ok(ccall((:set_precision, _lib_path()), Int32, (Int32,), precision), "Failed to set precision")
end

function set_warm_start(solver::TinyMPCSolver, on::Bool)
    _need(solver)
    _ok(ccall((:set_warm_start, _lib_path()), Int32, (Int32,), on ? 1 : 0), "Failed to set warm start")
    return 0
end
kernel_name() = unsafe_string(ccall((:get_kernel_name, _lib_path()), Cstring, ()))
# 0: no cones or cones shared by the batch, 1: a coefficient per instance (set_instance_cones!)
cone_mode() = Int(ccall((:get_cone_mode, _lib_path()), Int32, ()))

# x0: Vector (length nx, broadcast to the batch) or Matrix (nx, batch)
function set_x0(solver::TinyMPCSolver, x0::AbstractVecOrMat{Float64}; verbose::Bool=false)
    _need(solver)
    m = _mat(x0)
    _ok(ccall((:set_x0, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32, Int32),
              m, size(m, 1), size(m, 2), _flag(verbose)), "Failed to set initial state")
end

# Float32 host arrays: the device buffers are fp32, so this is a plain copy (the Float64 method narrows 65 536 x nx values on
# the host first).  x0: (nx,) broadcast to the batch, or (nx, batch)
function set_x0(solver::TinyMPCSolver, x0::AbstractVecOrMat{Float32}; verbose::Bool=false)
    _need(solver)
    m = x0 isa AbstractVector ? reshape(collect(x0), :, 1) : Matrix{Float32}(x0)
    _ok(ccall((:set_x0_f32, _lib_path()), Int32, (Ptr{Float32}, Int32, Int32, Int32),
              m, size(m, 1), size(m, 2), _flag(verbose)), "Failed to set initial state")
end

# x_ref: Matrix (nx, N) shared by the batch, or Array{Float64,3} (nx, N, batch)
function set_x_ref(solver::TinyMPCSolver, x_ref::AbstractArray{Float64}; verbose::Bool=false)
    _need(solver)
    m = _mat(x_ref)
    _ok(ccall((:set_x_ref, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32, Int32),
              m, size(m, 1), size(m, 2), _flag(verbose)), "Failed to set state reference")
end

# u_ref: Matrix (nu, N-1) shared by the batch, or Array{Float64,3} (nu, N-1, batch)
function set_u_ref(solver::TinyMPCSolver, u_ref::AbstractArray{Float64}; verbose::Bool=false)
    _need(solver)
    m = _mat(u_ref)
    _ok(ccall((:set_u_ref, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32, Int32),
              m, size(m, 1), size(m, 2), _flag(verbose)), "Failed to set input reference")
end

# Returns 0 (every instance converged), 1 (some instance hit max_iter) or -1; never throws on it,
# like the reference (src/TinyMPC.jl:143-148).
function solve(solver::TinyMPCSolver; verbose::Bool=false)
    _need(solver)
    return ccall((:solve_mpc, _lib_path()), Int32, (Int32,), _flag(verbose))
end

function get_solution(solver::TinyMPCSolver)
    _need(solver)
    nx, nu, N, B = solver.nx, solver.nu, solver.N, solver.batch
    xs, us = zeros(nx * N * B), zeros(nu * (N - 1) * B)
    xr, xc, ur, uc = Ref{Int32}(), Ref{Int32}(), Ref{Int32}(), Ref{Int32}()
    s1 = ccall((:get_states, _lib_path()), Int32, (Ptr{Float64}, Ref{Int32}, Ref{Int32}), xs, xr, xc)
    s2 = ccall((:get_controls, _lib_path()), Int32, (Ptr{Float64}, Ref{Int32}, Ref{Int32}), us, ur, uc)
    (s1 != 0 || s2 != 0) && error("Failed to get solution ($(_last_error()))")
    B == 1 && return (states=reshape(xs, nx, N), controls=reshape(us, nu, N - 1))   # the reference's shapes
    return (states=reshape(xs, nx, N, B), controls=reshape(us, nu, N - 1, B))
end

# The solution into the caller's own Float32 arrays (nx, N, batch) / (nu, N-1, batch): no allocation, no fp32 -> fp64
# widening on the host — the per-solve round trip of a closed loop that keeps Float32 state.
# (Device-resident callers skip the copies altogether: `device_buffers(solver)` returns the fp32 device pointers of x0,
# the references, states, controls and the status arrays; with AMDGPU.jl wrap them with
# `unsafe_wrap(ROCArray, convert(Ptr{Float32}, ptr), dims)`, fill x0 on the device, and call `solve_async` / `solve`.)
function get_solution!(states::Array{Float32,3}, controls::Array{Float32,3}, solver::TinyMPCSolver)
    _need(solver)
    nx, nu, N, B = solver.nx, solver.nu, solver.N, solver.batch
    (size(states) == (nx, N, B) && size(controls) == (nu, N - 1, B)) || error("get_solution!: states (nx, N, batch), controls (nu, N-1, batch)")
    xr, xc, ur, uc = Ref{Int32}(), Ref{Int32}(), Ref{Int32}(), Ref{Int32}()
    s1 = ccall((:get_states_f32, _lib_path()), Int32, (Ptr{Float32}, Ref{Int32}, Ref{Int32}), states, xr, xc)
    s2 = ccall((:get_controls_f32, _lib_path()), Int32, (Ptr{Float32}, Ref{Int32}, Ref{Int32}), controls, ur, uc)
    (s1 != 0 || s2 != 0) && error("Failed to get solution ($(_last_error()))")
    return (states=states, controls=controls)
end

# Page-lock an array that is reused with `get_solution!` / the Float32 `set_x0` (the copies then DMA straight into it).  The
# library never pins caller memory by itself: call `unpin_host!` before the array can be garbage-collected, e.g.
#   pin_host!(solver, states); try ... finally unpin_host!(solver, states) end
function pin_host!(solver::TinyMPCSolver, a::Array{Float32})
    _need(solver)
    _ok(ccall((:pin_host_buffer, _lib_path()), Int32, (Ptr{Cvoid}, Csize_t), a, sizeof(a)), "Failed to pin host array")
end
function unpin_host!(solver::TinyMPCSolver, a::Array{Float32})
    _need(solver)
    _ok(ccall((:unpin_host_buffer, _lib_path()), Int32, (Ptr{Cvoid},), a), "Failed to unpin host array")
end

# Per-instance iteration count, solved flag and residuals (pri_state, dua_state, pri_input, dua_input)
function get_status(solver::TinyMPCSolver)
    _need(solver)
    B = solver.batch
    iter, solved, res = zeros(Int32, B), zeros(Int32, B), zeros(4, B)
    _ok(ccall((:get_status, _lib_path()), Int32, (Ptr{Int32}, Ptr{Int32}, Ptr{Float64}), iter, solved, res),
        "Failed to get status")
    return (iter=iter, solved=solved, residuals=res)
end

# Shared references of every step of the next fused closed loops: x_ref_seq (nx, N, steps), u_ref_seq (nu, N-1, steps) —
# what the loop of examples/rocket_landing_constraints.jl:107-115 passes to set_x_ref / set_u_ref step by step.
# Supported wherever mpc_rollout is: inside the launch on the transposed-sets kernel (rocket shapes) and on the lanes-per-instance
# kernels at horizons up to 20 (cartpole shapes; quadrotor N = 20 with TINYMPC_HIP_MFMA_ONESHOT_ONLY=1), launch by launch on the chained loops
# (quadrotor shapes on the matrix-core kernel; the lean kernel's with TINYMPC_HIP_LEAN_WS=1 — with a sequence also when
# TINYMPC_HIP_LEAN_LOOP=1 asks for that kernel's in-kernel loop, which takes constant references only).  mpc_rollout fails, naming the
# condition, with fewer sequence steps than loop steps, per-instance references, adaptive rho, precision 2, a lanes-per-instance
# entry with a horizon above 20, shapes without a
# closed loop (stream / generic kernels) — precision 2 and those shapes unless TINYMPC_HIP_STREAM_MPC=1 gives them their
# chained loop (mpc_rollout below); a sharded solver (set_gpus > 1) takes no sequence.
# (julia/examples/rocket_landing_batch_closed_loop.jl, julia/examples/quadrotor_batch_tracking.jl)
function set_ref_sequence(solver::TinyMPCSolver, x_ref_seq::Array{Float64,3}, u_ref_seq::Array{Float64,3})
    _need(solver)
    steps = size(x_ref_seq, 3)
    (size(x_ref_seq) == (solver.nx, solver.N, steps) && size(u_ref_seq) == (solver.nu, solver.N - 1, steps)) ||
        error("set_ref_sequence: x_ref_seq (nx, N, steps), u_ref_seq (nu, N-1, steps)")
    _ok(ccall((:set_ref_sequence, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Int32),
              x_ref_seq, solver.nx, solver.N * steps, u_ref_seq, solver.nu, (solver.N - 1) * steps, steps),
        "Failed to set the reference sequence")
end

# `steps` closed-loop MPC steps in ONE launch: solve -> u0 = controls[:, 1] -> x0 = A x0 + B u0 + f -> next solve, the
# warm-start workspace staying on chip (the host loops of cartpole_example_mpc.jl:35-51, rocket_landing_constraints.jl:97-134).
# Returns (status of the last solve, x (nx, steps, batch) plant states, u (nu, steps, batch) applied controls,
# iter (steps, batch) ADMM iterations per step, negative where the step hit max_iter).
# Problems that run on the stream / generic kernels (other horizons, linear rows, per-instance families, precision 2, ...)
# have no closed loop by default and fail here.  TINYMPC_HIP_STREAM_MPC=1 in the environment at setup runs it as a chain of
# `steps` warm launches with the fp64 plant step between them; TINYMPC_HIP_STREAM_LOOP=1 beside it as one launch of the
# stream kernel's in-kernel loop where one is built (the same results, bit for bit).  Both are off by default.
function mpc_rollout(solver::TinyMPCSolver, steps::Integer)
    _need(solver)
    nx, nu, B = solver.nx, solver.nu, solver.batch
    x, u, it = zeros(nx, steps, B), zeros(nu, steps, B), zeros(Int32, steps, B)
    st = ccall((:mpc_rollout, _lib_path()), Int32, (Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}), steps, x, u, it)
    st < 0 && error("mpc_rollout failed ($(_last_error()))")
    if ccall((:estimator_mode, _lib_path()), Int32, ()) > 0      # an estimator: what every solve started from, and the measured outputs
        ny = ccall((:estimator_outputs, _lib_path()), Int32, ())
        xhat, yout = zeros(nx, steps, B), zeros(ny, steps, B)
        _ok(ccall((:get_mpc_estimate, _lib_path()), Int32, (Ptr{Float64},), xhat), "Failed to get the estimates")
        _ok(ccall((:get_mpc_outputs, _lib_path()), Int32, (Ptr{Float64},), yout), "Failed to get the measured outputs")
        return (status=st, x=x, u=u, iter=it, xhat=xhat, yout=yout)
    end
    if ccall((:noise_mode, _lib_path()), Int32, ()) >= 4     # measurement noise installed: what every step's solve started from
        y = zeros(nx, steps, B)
        _ok(ccall((:get_mpc_measured, _lib_path()), Int32, (Ptr{Float64},), y), "Failed to get the measured states")
        return (status=st, x=x, u=u, iter=it, y=y)
    end
    return (status=st, x=x, u=u, iter=it)
end

# The plant mpc_rollout steps when it is not the controller's model, x+ = f_p + A_p x + B_p u0 (+ w) in fp64 — Monte-Carlo over
# disturbances, a fleet whose true parameters differ from the model, robustness sweeps.  A (nx, nx), B (nx, nu), f (nx,) shared by
# the batch, or A (nx, nx, batch), B (nx, nu, batch), f (nx, batch) one plant per instance; f = nothing is zero;
# set_plant(solver, nothing, nothing) drops it.  mpc_rollout then runs as a chain of `steps` ordinary kept-workspace launches with the
# plant step between them, on whatever kernel such a solve takes (every shape and precision, no environment switch).  Not with
# adaptive rho, not on a sharded solver (set_gpus > 1).  (Written against the C-ABI like the rest of this file, not executed here.)
function set_plant(solver::TinyMPCSolver, A::Union{Array{Float64},Nothing}, B::Union{Array{Float64},Nothing},
                   f::Union{Array{Float64},Nothing}=nothing)
    _need(solver)
    if A === nothing && B === nothing
        return _ok(ccall((:set_plant, _lib_path()), Int32,
                         (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32),
                         C_NULL, 0, 0, C_NULL, 0, 0, C_NULL, 0, 0), "Failed to drop the plant")
    end
    (A === nothing || B === nothing) && error("set_plant: A and B, or nothing and nothing")
    per = ndims(A) == 3 ? 1 : 0
    _ok(ccall((:set_plant, _lib_path()), Int32,
              (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32),
              A, size(A, 1), div(length(A), size(A, 1)), B, size(B, 1), div(length(B), size(B, 1)),
              f === nothing ? C_NULL : f, f === nothing ? 0 : length(f), per), "Failed to set the plant")
end

# Additive disturbance of every step of the next closed loops: w (nx, steps) shared, or (nx, steps, batch) per instance (the layout
# of mpc_rollout's x); every mpc_rollout reads it from its first column; nothing drops it.  Without set_plant it disturbs the model.
function set_disturbance(solver::TinyMPCSolver, w::Union{Array{Float64},Nothing})
    _need(solver)
    w === nothing && return _ok(ccall((:set_disturbance, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32, Int32), C_NULL, 0, 0, 0),
                                "Failed to drop the disturbance")
    _ok(ccall((:set_disturbance, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32, Int32),
              w, size(w, 1), div(length(w), size(w, 1)), ndims(w) == 3 ? 1 : 0), "Failed to set the disturbance")
end

# 0 model, 1 shared plant, 2 per-instance plant; + 4 shared disturbance, + 8 per-instance disturbance
function plant_mode(solver::TinyMPCSolver)
    _need(solver)
    m = ccall((:plant_mode, _lib_path()), Int32, ())
    m < 0 && error("plant_mode failed ($(_last_error()))")
    return Int(m)
end

# Seeded process and measurement noise, drawn on the device: Monte-Carlo sweeps of mpc_rollout with nothing drawn on the host or
# uploaded.  A draw is a pure function of (seed, kind, instance, step): Philox4x32-10 and Box-Muller give nx standard normals xi, the
# noise vector is G xi (include/tinympc_hip.h states the rule; the covariance is G G').  G (nx, nx) shared, (nx, nx, batch) one
# factor per instance, a vector (nx,) is diag(sigma); nothing drops that kind.  With the noise cursor c (0-based) and loop step s,
# t = c + s: measurement noise — the solve of step s starts from Float32(x_t + G_v xi_v[b][t]), the fp64 plant state x_t is never
# contaminated; process noise — the plant step ends with + G_w xi_w[b][t], after the uploaded disturbance if any.  mpc_rollout
# then runs as the chain of `steps` kept-workspace launches (every shape and precision, no environment switch), leaves the cursor
# at c + steps, and returns y (nx, steps, batch), what every solve started from, while measurement noise is installed.  One cursor
# serves both kinds; a newly installed noise leaves it alone.  Not with adaptive rho, not on a sharded solver (set_gpus > 1).
# (Written against the C-ABI like the rest of this file, not executed here.)
_noise_factor(G::Array{Float64}) = ndims(G) == 1 ? [i == j ? G[i] : 0.0 for i in eachindex(G), j in eachindex(G)] : G

function set_process_noise(solver::TinyMPCSolver, G::Union{Array{Float64},Nothing}, seed::Integer=0)
    _need(solver)
    G === nothing && return _ok(ccall((:set_process_noise, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32, Int32, UInt64), C_NULL, 0, 0, 0, 0),
                                "Failed to drop the process noise")
    M = _noise_factor(G)
    _ok(ccall((:set_process_noise, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32, Int32, UInt64),
              M, size(M, 1), div(length(M), size(M, 1)), ndims(M) == 3 ? 1 : 0, UInt64(seed)), "Failed to set the process noise")
end

function set_measurement_noise(solver::TinyMPCSolver, G::Union{Array{Float64},Nothing}, seed::Integer=0)
    _need(solver)
    G === nothing && return _ok(ccall((:set_measurement_noise, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32, Int32, UInt64), C_NULL, 0, 0, 0, 0),
                                "Failed to drop the measurement noise")
    M = _noise_factor(G)
    _ok(ccall((:set_measurement_noise, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32, Int32, UInt64),
              M, size(M, 1), div(length(M), size(M, 1)), ndims(M) == 3 ? 1 : 0, UInt64(seed)), "Failed to set the measurement noise")
end

# the noise cursor (0-based step index of the next loop's first draw): 0 for a new solver, `steps` further on after every
# mpc_rollout of a solver with noise; a negative cursor is refused
function set_noise_cursor(solver::TinyMPCSolver, t::Integer)
    _need(solver)
    _ok(ccall((:set_noise_cursor, _lib_path()), Int32, (Int32,), t), "Failed to set the noise cursor")
end

function noise_cursor(solver::TinyMPCSolver)
    _need(solver)
    c = ccall((:noise_cursor, _lib_path()), Int32, ())
    c < 0 && error("noise_cursor failed ($(_last_error()))")
    return Int(c)
end

# 1 shared / 2 per-instance process factor; + 4 shared / + 8 per-instance measurement factor
function noise_mode(solver::TinyMPCSolver)
    _need(solver)
    m = ccall((:noise_mode, _lib_path()), Int32, ())
    m < 0 && error("noise_mode failed ($(_last_error()))")
    return Int(m)
end

# the realised noise vectors G xi of kind `which` (0 process, 1 measurement) at the steps t0 .. t0 + steps - 1, computed on the
# device by the loop's own device function: (nx, steps, batch)
function get_noise(solver::TinyMPCSolver, which::Integer, t0::Integer, steps::Integer)
    _need(solver)
    buf = zeros(solver.nx, steps, solver.batch)
    _ok(ccall((:get_noise, _lib_path()), Int32, (Int32, Int32, Int32, Ptr{Float64}), which, t0, steps, buf), "Failed to get the noise")
    return buf
end

# the draw rule on the host (no device needed): G (nx, nx), or nothing for the identity; b and t 0-based
function host_noise(seed::Integer, which::Integer, b::Integer, t::Integer, nx::Integer, G::Union{Matrix{Float64},Nothing}=nothing)
    out = zeros(nx)
    rc = ccall((:tinympc_host_noise, _lib_path()), Int32, (UInt64, Int32, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}),
               UInt64(seed), which, b, t, nx, G === nothing ? C_NULL : G, out)
    rc != 0 && error("host_noise failed ($(_last_error()))")
    return out
end

# Output feedback through a fixed-gain state estimator stepped on the device: the loop measures y = C x + v (ny <= nx outputs, v the
# first ny rows of the measurement noise where installed), corrects xhat = xhat- + L (y - C xhat-), solves from Float32(xhat) and
# predicts xhat-+ = f + A xhat + B u with the MODEL (include/tinympc_hip.h states the rule).  C (ny, nx) and L (nx, ny) shared, or
# (ny, nx, batch) and (nx, ny, batch); set_estimator(solver, nothing, nothing) drops it.  mpc_rollout then is the own-plant chain, returns
# xhat (nx, steps, batch) — what every solve started from — and yout (ny, steps, batch), and no y.  Between rollouts the solver keeps
# xhat- of the next step; set_x0 moves the plant, not the estimate.  Not with adaptive rho, not on a sharded solver.
# (Written against the C-ABI like the rest of this file, not executed here.)
function set_estimator(solver::TinyMPCSolver, C::Union{Array{Float64},Nothing}, L::Union{Array{Float64},Nothing})
    _need(solver)
    if C === nothing && L === nothing
        return _ok(ccall((:set_estimator, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Int32), C_NULL, 0, 0, C_NULL, 0, 0, 0),
                   "Failed to drop the estimator")
    end
    (C === nothing || L === nothing) && error("set_estimator: expected both C (ny, nx) and L (nx, ny), or neither to drop the estimator")
    _ok(ccall((:set_estimator, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Int32),
              C, size(C, 1), div(length(C), size(C, 1)), L, size(L, 1), div(length(L), size(L, 1)), ndims(C) == 3 ? 1 : 0), "Failed to set the estimator")
end

# xhat- of the next step: (nx,) shared or (nx, batch); nothing re-arms it (the next mpc_rollout takes xhat-_0 = x0)
function set_estimator_state(solver::TinyMPCSolver, xhat::Union{Array{Float64},Nothing})
    _need(solver)
    xhat === nothing && return _ok(ccall((:set_estimator_state, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32), C_NULL, 0, 0), "Failed to re-arm the estimate")
    _ok(ccall((:set_estimator_state, _lib_path()), Int32, (Ptr{Float64}, Int32, Int32), xhat, size(xhat, 1), div(length(xhat), size(xhat, 1))),
        "Failed to set the estimate")
end

# 0: no estimator, 1: shared C and L, 2: per instance
function estimator_mode(solver::TinyMPCSolver)
    _need(solver)
    m = ccall((:estimator_mode, _lib_path()), Int32, ())
    m < 0 && error("estimator_mode failed ($(_last_error()))")
    return Int(m)
end

# the current xhat- of the next step, (nx, batch)
function get_estimator_state(solver::TinyMPCSolver)
    _need(solver)
    buf = zeros(solver.nx, solver.batch)
    _ok(ccall((:get_estimator_state, _lib_path()), Int32, (Ptr{Float64},), buf), "Failed to get the estimate")
    return buf
end

# the rule on the host for one instance (no device needed): predict (A, B, f or nothing, u) and / or correct (C, L, the true state x,
# v or nothing); returns (xhat, y), y nothing without the correct
function host_estimator_step(xhat::Vector{Float64}; A=nothing, B=nothing, f=nothing, u=nothing, C=nothing, L=nothing, x=nothing, v=nothing,
                             predict::Bool=true, correct::Bool=true)
    nx = length(xhat)
    nu = B === nothing ? 1 : size(B, 2)
    ny = C === nothing ? 1 : size(C, 1)
    out, y = copy(xhat), zeros(ny)
    p(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    rc = GC.@preserve A B f u C L x v out y ccall((:tinympc_host_estimator_step, _lib_path()), Int32,
               (Int32, Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Ptr{Float64}), nx, nu, ny, predict ? 1 : 0, correct ? 1 : 0, p(A), p(B), p(f), p(C), p(L), p(u), p(x), p(v), pointer(out), pointer(y))
    rc != 0 && error("host_estimator_step failed ($(_last_error()))")
    return out, (correct ? y : nothing)
end

# the steady-state Kalman gain L (nx, ny) of the model (A, C) under the factors of set_process_noise / set_measurement_noise:
# W = Gw Gw', V = Gv[1:ny, :] Gv[1:ny, :]' (the filter Riccati recursion from P = W, host only)
function kalman_gain(A::Matrix{Float64}, C::Matrix{Float64}, Gw::Matrix{Float64}, Gv::Matrix{Float64})
    nx, ny = size(A, 1), size(C, 1)
    W, V = Gw * Gw', Gv[1:ny, :] * Gv[1:ny, :]'
    L, P = zeros(nx, ny), zeros(nx, nx)
    rc = ccall((:tinympc_host_kalman_gain, _lib_path()), Int32, (Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}),
               A, C, W, V, nx, ny, L, P)
    rc != 0 && error("kalman_gain failed ($(_last_error()))")
    return L
end

# Per-instance metrics of the closed loop, folded on the device: while enabled every mpc_rollout is followed on its stream by one
# kernel that reads the log it wrote and updates 11 fp64 slots per instance (METRIC_NAMES; include/tinympc_hip.h states the rule):
# they accumulate over rollouts until reset_rollout_metrics, so a long run is a sequence of short rollouts on a fixed-size log and
# only the statistics leave the device.  qw (nx), rw (nu): non-negative weights, nothing = the diagonal of Q / R; x_lo, x_hi (nx),
# u_lo, u_hi (nu): the metric's own safe set, nothing = that side never counts.  enable = false drops configuration and
# accumulators.  get_rollout_metrics: (11, batch); get_rollout_summary: (4, 11) — per slot the sum, minimum, maximum and number of
# instances > 0 (the C arrays [batch][11] and [11][4] seen column-major).  Not on a sharded solver (set_gpus > 1).
# (Written against the C-ABI like the rest of this file, not executed here.)
const METRIC_NAMES = (:steps, :cost_x, :cost_u, :peak_err, :final_err, :x_viol_max, :x_viol_steps, :first_viol, :u_sat_steps, :iters, :maxiter_steps)
_vec_or_null(v::Union{Vector{Float64},Nothing}) = v === nothing ? C_NULL : v

function set_rollout_metrics(solver::TinyMPCSolver, enable::Bool=true; qw::Union{Vector{Float64},Nothing}=nothing, rw::Union{Vector{Float64},Nothing}=nothing,
                             x_lo::Union{Vector{Float64},Nothing}=nothing, x_hi::Union{Vector{Float64},Nothing}=nothing,
                             u_lo::Union{Vector{Float64},Nothing}=nothing, u_hi::Union{Vector{Float64},Nothing}=nothing)
    _need(solver)
    for (v, n, name) in ((x_lo, solver.nx, "x_lo"), (x_hi, solver.nx, "x_hi"), (u_lo, solver.nu, "u_lo"), (u_hi, solver.nu, "u_hi"))
        v === nothing || length(v) == n || error("set_rollout_metrics: expected $n values of $name")
    end
    _ok(ccall((:set_rollout_metrics, _lib_path()), Int32,
              (Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
              enable ? 1 : 0, _vec_or_null(qw), qw === nothing ? 0 : length(qw), _vec_or_null(rw), rw === nothing ? 0 : length(rw),
              _vec_or_null(x_lo), _vec_or_null(x_hi), _vec_or_null(u_lo), _vec_or_null(u_hi)), "Failed to set the rollout metrics")
end

function reset_rollout_metrics(solver::TinyMPCSolver)
    _need(solver)
    _ok(ccall((:reset_rollout_metrics, _lib_path()), Int32, ()), "Failed to reset the rollout metrics")
end

function get_rollout_metrics(solver::TinyMPCSolver)
    _need(solver)
    buf = zeros(length(METRIC_NAMES), solver.batch)
    _ok(ccall((:get_rollout_metrics, _lib_path()), Int32, (Ptr{Float64},), buf), "Failed to get the rollout metrics")
    return buf
end

function get_rollout_summary(solver::TinyMPCSolver)
    _need(solver)
    buf = zeros(4, length(METRIC_NAMES))
    _ok(ccall((:get_rollout_summary, _lib_path()), Int32, (Ptr{Float64},), buf), "Failed to get the rollout summary")
    return buf
end

# A reference trajectory, windowed on the device: every instance tracks a moving target of its own through mpc_rollout, and nothing
# is uploaded per step.  x_traj (nx, Lx) and u_traj (nu, Lu) shared by the batch, or (nx, Lx, batch) and (nu, Lu, batch) one
# trajectory per instance (the shapes of mpc_rollout's x and u: one run's log can be another run's trajectory), both shared or both
# per instance; u_traj = nothing is zero input references; set_ref_trajectory(solver, nothing) drops it and leaves the window at the
# cursor as ordinary references.  With the cursor c (0-based) the references of a solve are the rows min(c + k, L - 1) of the
# trajectory, k = 0 .. N-1 (N-2 for u): the pattern of examples/rocket_landing_constraints.jl:107-115, which shifts x_ref by one
# knot per step, with the last row held beyond the end.  solve reads the window at the cursor; mpc_rollout(steps) the windows at
# c .. c+steps-1, as a chain of `steps` ordinary kept-workspace launches (every shape and precision, no environment switch), and
# leaves c + steps.  set_x_ref / set_u_ref / set_ref_sequence replace it; it replaces a sequence.  Not with adaptive rho, not on a
# sharded solver (set_gpus > 1).  (Written against the C-ABI like the rest of this file, not executed here.)
function set_ref_trajectory(solver::TinyMPCSolver, x_traj::Union{Array{Float64},Nothing}, u_traj::Union{Array{Float64},Nothing}=nothing;
                            verbose::Bool=false)
    _need(solver)
    sig = (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Int32, Int32)
    x_traj === nothing && return _ok(ccall((:set_ref_trajectory, _lib_path()), Int32, sig, C_NULL, 0, 0, C_NULL, 0, 0, 0, verbose ? 1 : 0),
                                     "Failed to drop the reference trajectory")
    (u_traj === nothing || ndims(u_traj) == ndims(x_traj)) ||
        error("set_ref_trajectory: x_traj and u_traj are both shared (nx, Lx) / (nu, Lu) or both per instance (nx, Lx, batch) / (nu, Lu, batch)")
    per = ndims(x_traj) == 3 ? 1 : 0
    _ok(ccall((:set_ref_trajectory, _lib_path()), Int32, sig,
              x_traj, size(x_traj, 1), div(length(x_traj), max(1, size(x_traj, 1))),
              u_traj === nothing ? C_NULL : u_traj, u_traj === nothing ? 0 : size(u_traj, 1),
              u_traj === nothing ? 0 : div(length(u_traj), max(1, size(u_traj, 1))), per, verbose ? 1 : 0),
        "Failed to set the reference trajectory")
end

# the cursor (0-based row of the trajectory the next window starts at): 0 for a new trajectory, `steps` further on after every
# mpc_rollout; a negative cursor is refused
function set_ref_cursor(solver::TinyMPCSolver, cursor::Integer)
    _need(solver)
    _ok(ccall((:set_ref_cursor, _lib_path()), Int32, (Int32,), cursor), "Failed to set the reference cursor")
end

function ref_cursor(solver::TinyMPCSolver)
    _need(solver)
    c = ccall((:ref_cursor, _lib_path()), Int32, ())
    c < 0 && error("ref_cursor failed ($(_last_error()))")
    return Int(c)
end

function reset_workspace(solver::TinyMPCSolver)
    _need(solver)
    _ok(ccall((:reset_workspace, _lib_path()), Int32, ()), "Failed to reset workspace")
end

# Like the reference (src/TinyMPC.jl:181-211) every field is sent with its keyword default, so a later
# call resets en_*_bound to false and the tolerances to 1e-3.
function update_settings(solver::TinyMPCSolver;
                         abs_pri_tol::Float64=1e-3, abs_dua_tol::Float64=1e-3, max_iter::Int=100,
                         check_termination::Bool=true, en_state_bound::Bool=false, en_input_bound::Bool=false,
                         en_state_soc::Bool=false, en_input_soc::Bool=false, en_state_linear::Bool=false,
                         en_input_linear::Bool=false, adaptive_rho::Bool=false, adaptive_rho_min::Float64=0.1,
                         adaptive_rho_max::Float64=10.0, adaptive_rho_enable_clipping::Bool=true,
                         verbose::Bool=false)
    _ok(ccall((:update_settings, _lib_path()), Int32,
              (Float64, Float64, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32,
               Int32, Float64, Float64, Int32, Int32),
              abs_pri_tol, abs_dua_tol, max_iter, _flag(check_termination), _flag(en_state_bound),
              _flag(en_input_bound), _flag(en_state_soc), _flag(en_input_soc), _flag(en_state_linear),
              _flag(en_input_linear), _flag(adaptive_rho), adaptive_rho_min, adaptive_rho_max,
              _flag(adaptive_rho_enable_clipping), _flag(verbose)), "Failed to update settings")
end

# per-knot bounds (nx, N) / (nu, N-1), shared by the batch; the library enables both bound flags
function set_bound_constraints(solver::TinyMPCSolver, x_min::Matrix{Float64}, x_max::Matrix{Float64},
                               u_min::Matrix{Float64}, u_max::Matrix{Float64}; verbose::Bool=false)
    _ok(ccall((:set_bound_constraints, _lib_path()), Int32,
              (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32,
               Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Int32),
              x_min, size(x_min, 1), size(x_min, 2), x_max, size(x_max, 1), size(x_max, 2),
              u_min, size(u_min, 1), size(u_min, 2), u_max, size(u_max, 1), size(u_max, 2), _flag(verbose)),
        "Failed to set bound constraints")
end

# bounds PER INSTANCE AND KNOT, (nx, N, batch) / (nu, N-1, batch) with batch > 1: the batch dimension rides on the column
# counts, as for set_x_ref.  The solver then runs on the `ib` form of the stream or the generic kernel (kernel_name());
# the shared method above returns it to shared bounds.  Not with adaptive rho; mpc_rollout only under TINYMPC_HIP_STREAM_MPC.
function set_bound_constraints(solver::TinyMPCSolver, x_min::Array{Float64,3}, x_max::Array{Float64,3},
                               u_min::Array{Float64,3}, u_max::Array{Float64,3}; verbose::Bool=false)
    _need(solver)
    ms = map(_mat, (x_min, x_max, u_min, u_max))
    _ok(ccall((:set_bound_constraints, _lib_path()), Int32,
              (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32,
               Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Int32),
              ms[1], size(ms[1], 1), size(ms[1], 2), ms[2], size(ms[2], 1), size(ms[2], 2),
              ms[3], size(ms[3], 1), size(ms[3], 2), ms[4], size(ms[4], 1), size(ms[4], 2), _flag(verbose)),
        "Failed to set per-instance bound constraints")
end

# per-instance bounds: (nx, N, batch) / (nu, N-1, batch) as above, or (nx, batch) / (nu, batch) — one column per instance,
# constant over the horizon (repeated over the knots here: the process-global entry points take the per-knot layout)
function set_instance_bounds(solver::TinyMPCSolver, x_min::Array{Float64,3}, x_max::Array{Float64,3},
                             u_min::Array{Float64,3}, u_max::Array{Float64,3}; verbose::Bool=false)
    set_bound_constraints(solver, x_min, x_max, u_min, u_max; verbose=verbose)
end
function set_instance_bounds(solver::TinyMPCSolver, x_min::Matrix{Float64}, x_max::Matrix{Float64},
                             u_min::Matrix{Float64}, u_max::Matrix{Float64}; verbose::Bool=false)
    _need(solver)
    over(a, knots) = repeat(reshape(a, size(a, 1), 1, size(a, 2)), 1, knots, 1)
    set_bound_constraints(solver, over(x_min, solver.N), over(x_max, solver.N), over(u_min, solver.N - 1),
                          over(u_max, solver.N - 1); verbose=verbose)
end

# Linear inequalities Alin_x x <= blin_x, Alin_u u <= blin_u at every knot (at most 8 rows per side); equalities as
# two opposite rows each.  Cones: per-knot second-order cones, inputs first,
# 0-based first row `Ac`, dimension `qc`, slope `c` (last row of the block is the axis); parity unpinned.
function set_linear_constraints(solver::TinyMPCSolver, Alin_x::Matrix{Float64}, blin_x::Vector{Float64},
                                Alin_u::Matrix{Float64}, blin_u::Vector{Float64}; verbose::Bool=false)
    _ok(ccall((:set_linear_constraints, _lib_path()), Int32,
              (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32),
              Alin_x, size(Alin_x, 1), size(Alin_x, 2), blin_x, length(blin_x),
              Alin_u, size(Alin_u, 1), size(Alin_u, 2), blin_u, length(blin_u), _flag(verbose)),
        "Failed to set linear constraints")
end

# linear rows PER INSTANCE, batch > 1: Alin_x (rows, nx, batch) with blin_x (rows, batch), Alin_u (rows, nu, batch) with blin_u
# (rows, batch); an empty side is zeros(0, n, batch) with zeros(0, batch); an all-zero row of an instance is a row that
# instance does not have.  The batch dimension rides on the widths of the process-global entry point, as for
# set_bound_constraints.  The solver then runs on the `il` form of the stream or the generic kernel (kernel_name()); the
# shared method above returns it to shared rows.  Not with adaptive rho; mpc_rollout only as a chain of launches.
# (Written and not executed, like the rest of this file: no Julia on the build machine.)
function set_instance_linear(solver::TinyMPCSolver, Alin_x::Array{Float64,3}, blin_x::Matrix{Float64},
                             Alin_u::Array{Float64,3}, blin_u::Matrix{Float64}; verbose::Bool=false)
    _need(solver)
    Ax, Au = _mat(Alin_x), _mat(Alin_u)
    bx, bu = vec(blin_x), vec(blin_u)
    _ok(ccall((:set_linear_constraints, _lib_path()), Int32,
              (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32),
              Ax, size(Ax, 1), size(Ax, 2), bx, length(bx),
              Au, size(Au, 1), size(Au, 2), bu, length(bu), _flag(verbose)),
        "Failed to set per-instance linear constraints")
end

function set_equality_constraints(solver::TinyMPCSolver, Aeq_x::Matrix{Float64}, beq_x::Vector{Float64};
                                  Aeq_u::Matrix{Float64}=zeros(0, solver.nu), beq_u::Vector{Float64}=zeros(Float64, 0))
    return set_linear_constraints(solver, vcat(Aeq_x, -Aeq_x), vcat(beq_x, -beq_x), vcat(Aeq_u, -Aeq_u), vcat(beq_u, -beq_u))
end

function set_cone_constraints(solver::TinyMPCSolver, Acu::Vector{Int32}, qcu::Vector{Int32}, cu::Vector{Float64},
                              Acx::Vector{Int32}, qcx::Vector{Int32}, cx::Vector{Float64}; verbose::Bool=false)
    _ok(ccall((:set_cone_constraints, _lib_path()), Int32,
              (Ptr{Int32}, Int32, Ptr{Int32}, Int32, Ptr{Float64}, Int32,
               Ptr{Int32}, Int32, Ptr{Int32}, Int32, Ptr{Float64}, Int32, Int32),
              Acu, length(Acu), qcu, length(qcu), cu, length(cu),
              Acx, length(Acx), qcx, length(qcx), cx, length(cx), _flag(verbose)),
        "Failed to set cone constraints")
end

# cone coefficients PER INSTANCE over one layout, batch > 1: Acu, qcu (n_u) with cu (n_u, batch), Acx, qcx (n_x) with cx (n_x, batch);
# an empty side is Int32[] with zeros(0, batch); Inf is a cone that instance does not have.  The batch dimension rides on the
# widths of the process-global entry point, [batch][cone] in memory, as for set_instance_linear.  The solver then runs on the
# `ic` form of the stream or the generic kernel (kernel_name()); the shared method above returns it to shared cones.  Not with
# adaptive rho; mpc_rollout only as a chain of launches.
# (Written and not executed, like the rest of this file: no Julia on the build machine.)
function set_instance_cones!(solver::TinyMPCSolver, Acu::Vector{Int32}, qcu::Vector{Int32}, cu::Matrix{Float64},
                             Acx::Vector{Int32}, qcx::Vector{Int32}, cx::Matrix{Float64}; verbose::Bool=false)
    _need(solver)
    cuv, cxv = vec(cu), vec(cx)    # column-major (cone, batch) is [batch][cone] in memory
    _ok(ccall((:set_cone_constraints, _lib_path()), Int32,
              (Ptr{Int32}, Int32, Ptr{Int32}, Int32, Ptr{Float64}, Int32,
               Ptr{Int32}, Int32, Ptr{Int32}, Int32, Ptr{Float64}, Int32, Int32),
              Acu, length(Acu), qcu, length(qcu), cuv, length(cuv),
              Acx, length(Acx), qcx, length(qcx), cxv, length(cxv), _flag(verbose)),
        "Failed to set per-instance cone constraints")
end

function set_cache_terms(solver::TinyMPCSolver, Kinf::Matrix{Float64}, Pinf::Matrix{Float64},
                         Quu_inv::Matrix{Float64}, AmBKt::Matrix{Float64}; verbose::Bool=false)
    _need(solver)
    _ok(ccall((:set_cache_terms, _lib_path()), Int32,
              (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32,
               Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Int32),
              Kinf, size(Kinf, 1), size(Kinf, 2), Pinf, size(Pinf, 1), size(Pinf, 2),
              Quu_inv, size(Quu_inv, 1), size(Quu_inv, 2), AmBKt, size(AmBKt, 1), size(AmBKt, 2), _flag(verbose)),
        "Failed to set cache terms")
end

# LQR gains of the rho-regularised problem the sensitivities are differenced on (reference TinyMPC.jl:326-352):
# rho enters once, P starts at Q + rho I, a 1e-8 ridge in the gain solve only, at most 5000 sweeps.
function _lqr_gains(A, B, Q, R, rho)
    nx, nu = size(A, 1), size(B, 2)
    Qr = Q + rho * Matrix{Float64}(I, nx, nx)
    Rr = R + rho * Matrix{Float64}(I, nu, nu)
    P = copy(Qr)
    K = zeros(nu, nx)
    for sweep in 1:5000
        Kold = K
        K = (Rr + B' * P * B + 1e-8 * Matrix{Float64}(I, nu, nu)) \ (B' * P * A)
        P = Qr + A' * P * (A - B * K)
        (sweep > 1 && norm(K - Kold) < 1e-10) && break
    end
    return K, P, inv(Rr + B' * P * B), Matrix((A - B * K)')
end

"""
    compute_sensitivity_autograd(solver) -> (dK, dP, dC1, dC2)

Forward differences (h = 1e-6) of the cache terms in rho, as the reference's function of the same name
(TinyMPC.jl:301-323).  `update_settings(adaptive_rho=true)` without `set_sensitivity` makes the library do the same.
"""
function compute_sensitivity_autograd(solver::TinyMPCSolver)
    _need(solver)
    h = 1e-6
    g0 = _lqr_gains(solver.A, solver.B, solver.Q, solver.R, solver.rho)
    g1 = _lqr_gains(solver.A, solver.B, solver.Q, solver.R, solver.rho + h)
    return ntuple(i -> (g1[i] - g0[i]) / h, 4)
end

# What codegen_with_sensitivity (reference TinyMPC.jl:374-394) bakes into generated code, for the live solver.
function set_sensitivity(solver::TinyMPCSolver, dK::Matrix{Float64}, dP::Matrix{Float64},
                         dC1::Matrix{Float64}, dC2::Matrix{Float64}; verbose::Bool=false)
    _need(solver)
    _ok(ccall((:set_sensitivity, _lib_path()), Int32,
              (Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32,
               Ptr{Float64}, Int32, Int32, Ptr{Float64}, Int32, Int32, Int32),
              dK, size(dK, 1), size(dK, 2), dP, size(dP, 1), size(dP, 2),
              dC1, size(dC1, 1), size(dC1, 2), dC2, size(dC2, 1), size(dC2, 2), _flag(verbose)),
        "Failed to set sensitivity matrices")
end

# rho of every instance after adaptation
function get_adaptive_rho(solver::TinyMPCSolver)
    _need(solver)
    rho = zeros(Float64, solver.batch)
    n = Ref{Int32}(0)
    _ok(ccall((:get_adaptive_rho, _lib_path()), Int32, (Ptr{Float64}, Ptr{Int32}), rho, n), "Failed to get adaptive rho")
    return rho
end

function print_problem_data(solver::TinyMPCSolver; verbose::Bool=false)
    _need(solver)
    ccall((:print_problem_data, _lib_path()), Int32, (Int32,), _flag(verbose))
end

cleanup() = try; ccall((:cleanup_solver, _lib_path()), Cvoid, ()); catch; end
atexit(cleanup)

end # module
