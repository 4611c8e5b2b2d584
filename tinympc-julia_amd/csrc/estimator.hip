// Output feedback through a fixed-gain state estimator stepped on the device (tinympc_set_estimator; the rule: estimator.h):
// the kernel the chain (Solver::rollout_chain, solver.hip) launches around its solves and plant steps, and the solver's side —
// set, drop, the state between rollouts, the logs.  No solve kernel knows of it.
#include "solver.h"
#include "estimator.h"
#include "noise.h"

#include <string>

namespace tmpc {

#define HIP_TRY(expr)                       \
    do {                                    \
        if (!hip_ok((expr), #expr)) return -1; \
    } while (0)

struct EstimatorStep {
    double *xhat;            // [batch][nx]: read whole by every row of an instance, then written
    const float *xhat0;      // not null: xhat- is (double)xhat0[b][r] — the caller's x0, the first rollout of an estimate not yet live
    float *x0;               // [batch][nx]: takes (float)xhat_t, what the solve starts from (CORRECT)
    const double *x0d;       // [batch][nx]: the true plant state (CORRECT)
    const float *uout;       // [batch][nu (N - 1)]: the solution whose first control was applied (PREDICT)
    const double *model;     // [A | B | f], instance b's at model + b * model_stride (PREDICT)
    const double *C, *L;     // instance b's at C + b * c_stride, L + b * c_stride (0: shared)
    const double *Gv;        // the measurement noise factor, instance b's at Gv + b * gv_stride; null: v = 0 and no add
    long model_stride, c_stride, gv_stride;
    unsigned long long seed_v;
    float *xlog, *ylog;      // [batch][steps][nx] (float)xhat_t, [batch][steps][ny] (float)y_t
    int nx, nu, ny, N, steps, step, t;   // step: the log row; t = noise cursor + step: the draw
    long batch;
};

// One launch of the rule, plant_step_kernel's layout: 256 / nx instances per workgroup, lane (instance, r) owns row r.
//   PREDICT  row r of xhat- = f + A xhat + B u0 from d_xhat (all of the instance's rows) and the solution; else xhat- is d_xhat's
//            row (or x0's, xhat0);
//   CORRECT  the lanes r < ceil(nx / 2) draw the instance's pairs of xi_v[b][t] into LDS (noise_block_row's scheme; only where Gv
//            is given), xhat- goes to LDS; behind the barrier the lanes r < ny form y[r] = C x + v[r] and the innovation
//            e[r] = y[r] - C xhat- into LDS, behind a second barrier every lane takes its row of xhat- + L e.
// Every lane of the workgroup reaches both barriers (the ragged last workgroup's and the 256 % nx idle lanes included: nothing
// returns before them, and their conditions are kernel arguments), and the first one is also where every row has read d_xhat
// before any row writes it.
template <bool PREDICT, bool CORRECT>
__global__ void __launch_bounds__(256) estimator_step_kernel(EstimatorStep a) {
    __shared__ double xm[256], xi[CORRECT ? 256 : 1], inn[CORRECT ? 256 : 1];
    const int nx = a.nx, per_block = 256 / nx, lane = (int)threadIdx.x, g = lane / nx, r = lane - g * nx;
    const long b = (long)blockIdx.x * per_block + g;
    const bool on = g < per_block && b < a.batch;
    double *mine_x = xm + g * nx;
    double xr = 0.0;
    if (on) {
        if constexpr (PREDICT)
            xr = estimator_predict_row(a.model + b * a.model_stride, nx, a.nu, r, a.xhat + b * nx, a.uout + b * (long)a.nu * (a.N - 1));
        else
            xr = a.xhat0 ? (double)a.xhat0[b * nx + r] : a.xhat[b * nx + r];
    }
    if constexpr (CORRECT) {
        if (on) {
            mine_x[r] = xr;
            if (a.Gv && 2 * r < nx) {
                double even, odd;
                noise_pair(a.seed_v, NOISE_MEASUREMENT, (uint64_t)b, (unsigned)a.t, (uint32_t)r, even, odd);
                xi[g * nx + 2 * r] = even;
                if (2 * r + 1 < nx) xi[g * nx + 2 * r + 1] = odd;
            }
        }
    }
    __syncthreads();   // (every row has read d_xhat; xhat- and the draws are in LDS)
    if constexpr (CORRECT) {
        const int ny = a.ny;
        if (on && r < ny) {
            const double *C = a.C + b * a.c_stride;
            double y = estimator_output_row(C, nx, ny, r, a.x0d + b * nx);
            if (a.Gv) y = y + noise_row(a.Gv + b * a.gv_stride, nx, r, xi + g * nx);
            inn[g * nx + r] = y - estimator_output_row(C, nx, ny, r, mine_x);
            a.ylog[(b * a.steps + a.step) * ny + r] = (float)y;
        }
        __syncthreads();
        if (on) xr = estimator_correct_row(a.L + b * a.c_stride, nx, ny, r, xr, inn + g * nx);
    }
    if (!on) return;
    a.xhat[b * nx + r] = xr;
    if constexpr (CORRECT) {
        a.x0[b * nx + r] = (float)xr;
        a.xlog[(b * a.steps + a.step) * nx + r] = (float)xr;
    }
}

// ---- the solver's side ----
int Solver::estimator_step(hipStream_t stream, bool predict, bool correct, int mpc_steps, int step) {
    const long per_block = 256 / nx;
    const bool measured = noise_kind[NOISE_MEASUREMENT] != 0;
    EstimatorStep a{};
    a.xhat = d_xhat;
    a.xhat0 = (!predict && !xhat_live) ? d_x0 : nullptr;
    a.x0 = d_x0, a.x0d = d_x0d, a.uout = d_uout;
    a.model = plant_kind ? d_model : d_plant;
    a.model_stride = model_stride();
    a.C = d_est_C, a.L = d_est_L;
    a.c_stride = est_kind == 2 ? (long)nx * est_ny : 0L;
    a.Gv = measured ? d_noise_G[NOISE_MEASUREMENT] : nullptr;
    a.gv_stride = noise_kind[NOISE_MEASUREMENT] == 2 ? (long)nx * nx : 0L;
    a.seed_v = noise_seed[NOISE_MEASUREMENT];
    a.xlog = d_mpc_y, a.ylog = d_mpc_yout;
    a.nx = nx, a.nu = nu, a.ny = est_ny, a.N = N, a.steps = mpc_steps, a.step = step, a.t = noise_cursor + step;
    a.batch = batch;
    const unsigned groups = (unsigned)((batch + per_block - 1) / per_block);
    if (predict && correct)
        estimator_step_kernel<true, true><<<groups, 256, 0, stream>>>(a);
    else if (predict)
        estimator_step_kernel<true, false><<<groups, 256, 0, stream>>>(a);
    else
        estimator_step_kernel<false, true><<<groups, 256, 0, stream>>>(a);
    if (correct) xhat_live = true;   // (d_xhat holds the estimate from here on)
    return 0;
}

// the logs of a loop of mpc_steps: (float)xhat_t in d_mpc_y (the buffer measurement noise logs into without an estimator), (float)y_t
int Solver::ensure_estimator_logs(int mpc_steps) {
    if (mpc_y_cap < mpc_steps) {
        if (d_mpc_y.alloc((size_t)batch * mpc_steps * nx)) return -1;
        mpc_y_cap = mpc_steps;
    }
    if (mpc_yout_cap < mpc_steps) {
        if (d_mpc_yout.alloc((size_t)batch * mpc_steps * est_ny)) return -1;
        mpc_yout_cap = mpc_steps;
    }
    mpc_y_steps = mpc_yout_steps = mpc_steps;
    return 0;
}

void Solver::drop_estimator() {
    if (!estimating() && !d_xhat) return;
    (void)wait_last_launch();   // (a chain still running reads and writes them)
    est_kind = est_ny = 0;
    est_C.clear(), est_L.clear();
    d_est_C.free();
    d_est_L.free();
    d_xhat.free();
    d_model.free();
    d_mpc_yout.free();
    mpc_yout_cap = mpc_yout_steps = 0;
    if (!noise_kind[NOISE_MEASUREMENT]) {   // (the estimate's log is not a measurement log)
        d_mpc_y.free();
        mpc_y_cap = 0;
    }
    mpc_y_steps = 0;
    xhat_live = false;
    plant_dirty = true;
}

// C ny x nx and L nx x ny, column-major fp64, shared or [batch] of each; C null drops the estimator.  Installing (or replacing)
// one re-arms the estimate: the next rollout takes xhat-_0 from x0 unless set_estimator_state installs another.
int Solver::set_estimator(const double *C, int ny, const double *L, int per_instance) {
    HIP_TRY(hipSetDevice(device));
    if (!C && !L) {
        drop_estimator();
        return 0;
    }
    if (!C || !L) {
        set_error("set_estimator: expected both C (ny x nx) and L (nx x ny), or neither to drop the estimator");
        return -1;
    }
    if (ny < 1 || ny > nx) {
        set_error("set_estimator: ny = " + std::to_string(ny) + " outputs; expected 1 <= ny <= nx = " + std::to_string(nx));
        return -1;
    }
    if (nx > 256) {
        set_error("set_estimator: the estimator's kernel holds an instance's rows in one workgroup, nx <= 256");
        return -1;
    }
    if (wait_last_launch()) return -1;   // (a chain still running reads the matrices)
    const size_t n = (per_instance ? (size_t)batch : 1) * (size_t)nx * ny;
    est_C.assign(C, C + n);
    est_L.assign(L, L + n);
    if (d_est_C.upload(est_C) || d_est_L.upload(est_L)) return -1;
    if (!d_xhat && d_xhat.alloc((size_t)batch * nx)) return -1;
    if (ny != est_ny) {   // (the output log's row length)
        d_mpc_yout.free();
        mpc_yout_cap = mpc_yout_steps = 0;
    }
    est_kind = per_instance ? 2 : 1, est_ny = ny;
    xhat_live = false;
    mpc_y_steps = 0;      // (what d_mpc_y holds is no estimate log)
    plant_dirty = true;   // (the model's image beside an installed plant: ensure_plant)
    return 0;
}

// xhat- of the next step: nx (shared) or [batch][nx] fp64; null re-arms xhat- = x0 at the next rollout
int Solver::set_estimator_state(const double *xhat, int per_instance) {
    if (!estimating()) {
        set_error("set_estimator_state: no estimator is installed (set_estimator)");
        return -1;
    }
    if (!xhat) {
        xhat_live = false;
        return 0;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    std::vector<double> h((size_t)batch * nx);
    for (size_t b = 0; b < (size_t)batch; ++b)
        for (int r = 0; r < nx; ++r) h[b * nx + r] = xhat[(per_instance ? b * nx : 0) + r];
    HIP_TRY(hipMemcpy(d_xhat, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    xhat_live = true;
    return 0;
}

// the current xhat- [batch][nx] fp64: what the next step's correct starts from (not live: (double)x0, what the next rollout takes)
int Solver::get_estimator_state(double *xhat) {
    if (!estimating() || !xhat) {
        set_error("get_estimator_state: no estimator is installed (set_estimator), or a null buffer");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    if (xhat_live) {
        HIP_TRY(hipMemcpy(xhat, d_xhat, (size_t)batch * nx * sizeof(double), hipMemcpyDeviceToHost));
        return 0;
    }
    std::vector<float> h((size_t)batch * nx);
    HIP_TRY(hipMemcpy(h.data(), d_x0, h.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h.size(); ++i) xhat[i] = (double)h[i];
    return 0;
}

// what every step's solve of the last loop started from, (float)xhat_t, [batch][steps][nx]
int Solver::get_mpc_estimate(double *xhat) {
    if (!estimating() || mpc_steps_last <= 0 || mpc_y_steps != mpc_steps_last || !xhat) {
        set_error("get_mpc_estimate: no mpc_rollout with an estimator has run (set_estimator, then mpc_rollout)");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    return d2h_double(d_mpc_y, xhat, (size_t)batch * mpc_steps_last * nx);
}

// the measured outputs of the last loop, (float)y_t, [batch][steps][ny]
int Solver::get_mpc_outputs(double *y) {
    if (!estimating() || mpc_steps_last <= 0 || mpc_yout_steps != mpc_steps_last || !y) {
        set_error("get_mpc_outputs: no mpc_rollout with an estimator has run (set_estimator, then mpc_rollout)");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    return d2h_double(d_mpc_yout, y, (size_t)batch * mpc_steps_last * est_ny);
}

}  // namespace tmpc
