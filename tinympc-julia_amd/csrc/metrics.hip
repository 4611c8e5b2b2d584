// Per-instance closed-loop metrics folded on the device (tinympc_set_rollout_metrics; the rule: metrics.h): a pass BEHIND a
// rollout over the log every route writes in one layout (d_mpc_x [batch][steps][nx], d_mpc_u, d_mpc_iter), accumulated per
// instance across rollouts, and the batch summary of the accumulators.  No solve kernel knows of it.
#include "solver.h"
#include "metrics.h"

#include <algorithm>
#include <climits>
#include <string>

namespace tmpc {

#define HIP_TRY(expr)                       \
    do {                                    \
        if (!hip_ok((expr), #expr)) return -1; \
    } while (0)

// Where the target of (instance b, loop step s) lies: row r at base[b * inst_stride + min(offset + s * step_stride, last) + r],
// base null: zero.  One form for
//   a reference trajectory at cursor c: x: offset (c + 1) nx, step_stride nx, last (Lx - 1) nx; u: offset c nu, step_stride nu, last (Lu - 1) nu;
//   a reference sequence: step_stride one step's slice, offset nx (knot 1) / 0 (knot 0), no clamp;
//   constant references: step_stride 0, the same offsets; inst_stride 0 wherever the batch shares them.
struct MetricTarget {
    const float *base;
    long inst_stride, step_stride, offset, last;
};

constexpr int METRIC_THREADS = 256;

// One rollout's log folded into the accumulators, metrics [batch][METRIC_COUNT] fp64, read-modify-write.
// L lanes per instance (a power of two up to 64, METRIC_THREADS / L instances per workgroup); lane l takes the steps l, l + L, ...
// whole: consecutive lanes read consecutive steps, an instance's log is contiguous and so are consecutive instances', so at
// every trip a wavefront reads 64 / L spans of L nx floats (and of L nu floats, L ints), adjacent where L >= steps — each
// byte of the log once, no index split by division anywhere.  The L partial spans combine by an xor butterfly inside the
// group (sums and maxima in that fixed order; the first step out by a minimum; the last step's error from the lane that holds
// it), the rollout's eleven slots go to LDS, and after the barrier (which every lane reaches) the workgroup combines its
// METRIC_THREADS / L * 11 slots with the accumulators as one contiguous read and write, a thread per (instance, slot).
template <int L>
__global__ void __launch_bounds__(METRIC_THREADS)
rollout_metrics_kernel(double *metrics, const float *xlog, const float *ulog, const int *ilog, MetricTarget tx, MetricTarget tu, MetricConfig cfg,
                       int nx, int nu, int steps, long batch) {
    constexpr int PER = METRIC_THREADS / L;
    __shared__ double part[PER * METRIC_COUNT], had[PER];   // the rollout's slots; the steps folded before it
    const int g = (int)threadIdx.x / L, l = (int)threadIdx.x % L;
    const long b0 = (long)blockIdx.x * PER, b = b0 + g;
    const bool on = b < batch;
    double cost_x = 0.0, cost_u = 0.0, peak = 0.0, fin = 0.0, viol = 0.0, iters = 0.0;
    int out_steps = 0, sat_steps = 0, maxit_steps = 0, first = INT_MAX;
    if (on) {
        const float *xb = xlog + b * steps * nx, *ub = ulog + b * steps * nu;
        const int *ib = ilog + b * steps;
        const float *xt = tx.base ? tx.base + b * tx.inst_stride : nullptr, *ut = tu.base ? tu.base + b * tu.inst_stride : nullptr;
        for (int s = l; s < steps; s += L) {
            const long ox = tx.offset + s * tx.step_stride, ou = tu.offset + s * tu.step_stride;
            const MetricStep m = metric_step(nx, nu, xb + (long)s * nx, ub + (long)s * nu, xt ? xt + (ox < tx.last ? ox : tx.last) : nullptr,
                                             ut ? ut + (ou < tu.last ? ou : tu.last) : nullptr, cfg);
            const int it = ib[s];
            cost_x += m.cost_x;
            cost_u += m.cost_u;
            peak = m.err > peak ? m.err : peak;
            viol = m.viol > viol ? m.viol : viol;
            if (s == steps - 1) fin = m.err;
            if (m.out) ++out_steps, first = s < first ? s : first;
            sat_steps += m.sat ? 1 : 0;
            iters += it < 0 ? -(double)it : (double)it;
            maxit_steps += it < 0 ? 1 : 0;
        }
    }
#pragma unroll
    for (int d = 1; d < L; d <<= 1) {   // (groups are aligned runs of L lanes of one wavefront: every partner is in the group)
        cost_x += __shfl_xor(cost_x, d);
        cost_u += __shfl_xor(cost_u, d);
        iters += __shfl_xor(iters, d);
        const double p = __shfl_xor(peak, d), v = __shfl_xor(viol, d), f = __shfl_xor(fin, d);
        peak = p > peak ? p : peak;
        viol = v > viol ? v : viol;
        fin = f > fin ? f : fin;   // (one lane holds the last step's error, the others 0, and an error is >= 0)
        out_steps += __shfl_xor(out_steps, d);
        sat_steps += __shfl_xor(sat_steps, d);
        maxit_steps += __shfl_xor(maxit_steps, d);
        const int q = __shfl_xor(first, d);
        first = q < first ? q : first;
    }
    if (l == 0) {
        double *p = part + g * METRIC_COUNT;
        p[METRIC_STEPS] = (double)steps;
        p[METRIC_COST_X] = cost_x;
        p[METRIC_COST_U] = cost_u;
        p[METRIC_PEAK_ERR] = peak;
        p[METRIC_FINAL_ERR] = fin;
        p[METRIC_X_VIOL_MAX] = viol;
        p[METRIC_X_VIOL_STEPS] = (double)out_steps;
        p[METRIC_FIRST_VIOL] = first == INT_MAX ? 0.0 : (double)first + 1.0;
        p[METRIC_U_SAT_STEPS] = (double)sat_steps;
        p[METRIC_ITERS] = iters;
        p[METRIC_MAXITER_STEPS] = (double)maxit_steps;
    }
    if ((int)threadIdx.x < PER && b0 + threadIdx.x < batch) had[threadIdx.x] = metrics[(b0 + threadIdx.x) * METRIC_COUNT];   // (read before any thread writes it)
    __syncthreads();
    const long left = batch - b0;
    const int count = (int)(left < PER ? left : PER) * METRIC_COUNT;
    double *acc = metrics + b0 * METRIC_COUNT;
    for (int j = (int)threadIdx.x; j < count; j += METRIC_THREADS) {
        const int i = j / METRIC_COUNT, k = j - i * METRIC_COUNT;   // (a division by a constant: a multiply and a shift)
        acc[j] = metric_combine(k, acc[j], part[j], had[i], (double)steps);
    }
}

// The batch summary, [METRIC_COUNT][4] = per slot the sum, the minimum, the maximum and the number of instances whose value
// is > 0, in a FIXED order and without atomics, so that it is the same bits from run to run: every thread folds the instances
// METRIC_THREADS * gridDim.x apart in ascending order, a wavefront combines by an xor butterfly, thread t < 44 of the workgroup
// combines the workgroup's wavefronts in ascending order into partials[workgroup][44]; metrics_summary_final_kernel — one
// workgroup — combines the partials in ascending order.
constexpr int METRIC_SUMMARY = METRIC_COUNT * 4, METRIC_SUMMARY_GROUPS = 128;

__device__ inline double metric_summary_combine(int q, double a, double b) {   // q: 0 sum, 1 min, 2 max, 3 count
    return q == 1 ? (b < a ? b : a) : (q == 2 ? (b > a ? b : a) : a + b);
}

__global__ void __launch_bounds__(METRIC_THREADS) metrics_summary_kernel(double *partials, const double *metrics, long batch) {
    constexpr int WAVES = METRIC_THREADS / 64;
    __shared__ double red[WAVES * METRIC_SUMMARY];
    double v[METRIC_SUMMARY];
#pragma unroll
    for (int k = 0; k < METRIC_COUNT; ++k) v[4 * k] = 0.0, v[4 * k + 1] = INFINITY, v[4 * k + 2] = -INFINITY, v[4 * k + 3] = 0.0;
    for (long i = (long)blockIdx.x * METRIC_THREADS + threadIdx.x; i < batch; i += (long)gridDim.x * METRIC_THREADS) {
#pragma unroll
        for (int k = 0; k < METRIC_COUNT; ++k) {
            const double m = metrics[i * METRIC_COUNT + k];
            v[4 * k] += m;
            v[4 * k + 1] = m < v[4 * k + 1] ? m : v[4 * k + 1];
            v[4 * k + 2] = m > v[4 * k + 2] ? m : v[4 * k + 2];
            v[4 * k + 3] += m > 0.0 ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int e = 0; e < METRIC_SUMMARY; ++e) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) v[e] = metric_summary_combine(e & 3, v[e], __shfl_xor(v[e], d));
    }
    const int wave = (int)threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int e = 0; e < METRIC_SUMMARY; ++e) red[wave * METRIC_SUMMARY + e] = v[e];
    }
    __syncthreads();
    if (threadIdx.x < METRIC_SUMMARY) {
        const int e = (int)threadIdx.x;
        double a = red[e];
        for (int w = 1; w < WAVES; ++w) a = metric_summary_combine(e & 3, a, red[w * METRIC_SUMMARY + e]);
        partials[(long)blockIdx.x * METRIC_SUMMARY + e] = a;
    }
}

__global__ void metrics_summary_final_kernel(double *summary, const double *partials, int groups) {
    const int e = (int)threadIdx.x;
    if (e >= METRIC_SUMMARY) return;
    double a = partials[e];
    for (int w = 1; w < groups; ++w) a = metric_summary_combine(e & 3, a, partials[(long)w * METRIC_SUMMARY + e]);
    summary[e] = a;
}

// ---- host side ----
void Solver::drop_rollout_metrics() {
    if (!metrics_on && !d_metrics) return;
    (void)wait_last_launch();   // (a fold still running reads and writes them)
    metrics_on = false;
    d_metrics.free();
    d_metric_cfg.free();
    d_metric_part.free();
    metric_limits = 0;
}

// enable: installs or replaces the configuration and zeroes the accumulators; else drops both.  The configuration on the device:
// [qw nx | rw nu | x_lo nx | x_hi nx | u_lo nu | u_hi nu] fp64, a null limit array left out of the kernel's MetricConfig.
int Solver::set_rollout_metrics(int enable, const double *qw, const double *rw, const double *x_lo, const double *x_hi, const double *u_lo,
                                const double *u_hi) {
    if (!enable) {
        drop_rollout_metrics();
        return 0;
    }
    if ((!qw || !rw) && hetero) {
        set_error("set_rollout_metrics: a per-instance-family solver has no one Q and R to take the weights from (qw / rw null): give qw (nx) and rw (nu)");
        return -1;
    }
    std::vector<double> h((size_t)3 * nx + 3 * nu, 0.0);
    double *hq = h.data(), *hr = hq + nx, *hxl = hr + nu, *hxh = hxl + nx, *hul = hxh + nx, *huh = hul + nu;
    for (int r = 0; r < nx; ++r) hq[r] = qw ? qw[r] : Q(r, r);
    for (int a = 0; a < nu; ++a) hr[a] = rw ? rw[a] : R(a, a);
    for (size_t i = 0; i < (size_t)nx + nu; ++i)
        if (!(h[i] >= 0.0)) {
            set_error("set_rollout_metrics: a weight is negative (or not a number); qw (nx) and rw (nu) are non-negative");
            return -1;
        }
    for (int r = 0; r < nx; ++r) {
        if (x_lo) hxl[r] = x_lo[r];
        if (x_hi) hxh[r] = x_hi[r];
        if (x_lo && x_hi && !(x_lo[r] <= x_hi[r])) {
            set_error("set_rollout_metrics: x_lo > x_hi in row " + std::to_string(r));
            return -1;
        }
    }
    for (int a = 0; a < nu; ++a) {
        if (u_lo) hul[a] = u_lo[a];
        if (u_hi) huh[a] = u_hi[a];
        if (u_lo && u_hi && !(u_lo[a] <= u_hi[a])) {
            set_error("set_rollout_metrics: u_lo > u_hi in row " + std::to_string(a));
            return -1;
        }
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;   // (a fold still running reads the configuration)
    const size_t n = (size_t)batch * METRIC_COUNT;
    // all three or none: !d_metrics means that none of them exists
    if (!d_metrics && (d_metrics.alloc(n) || d_metric_cfg.alloc(h.size()) || d_metric_part.alloc((size_t)(METRIC_SUMMARY_GROUPS + 1) * METRIC_SUMMARY))) {
        d_metrics.free(), d_metric_cfg.free(), d_metric_part.free();
        return -1;
    }
    HIP_TRY(hipMemcpy(d_metric_cfg, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    if (d_metrics.zero()) return -1;
    metric_limits = (x_lo ? 1 : 0) | (x_hi ? 2 : 0) | (u_lo ? 4 : 0) | (u_hi ? 8 : 0);
    metrics_on = true;
    return 0;
}

int Solver::reset_rollout_metrics() {
    if (!metrics_on) {
        set_error("reset_rollout_metrics: metrics are not enabled (set_rollout_metrics)");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    return d_metrics.zero();
}

// The fold of the rollout just enqueued on `stream`, behind it; cursor0: the reference cursor the rollout started from.  The
// targets are the references the rollout's solves used, read where the solver keeps them: the trajectory itself, the
// sequence, or the installed reference arrays in their mode (upload_refs ran in plan_rollout).
int Solver::fold_rollout_metrics(hipStream_t stream, int mpc_steps, int cursor0) {
    MetricTarget tx{nullptr, 0, 0, 0, LONG_MAX}, tu = tx;
    if (traj_kind) {
        tx = {d_xtraj, traj_kind == 2 ? (long)traj_Lx * nx : 0L, (long)nx, ((long)cursor0 + 1) * nx, ((long)traj_Lx - 1) * nx};
        if (traj_Lu > 0) tu = {d_utraj, traj_kind == 2 ? (long)traj_Lu * nu : 0L, (long)nu, (long)cursor0 * nu, ((long)traj_Lu - 1) * nu};
    } else if (ref_seq_steps > 0) {
        tx = {d_xref_seq, 0L, (long)ex(), (long)nx, LONG_MAX};
        tu = {d_uref_seq, 0L, (long)eu(), 0L, LONG_MAX};
    } else if (ref_mode != REF_ZERO) {
        const bool per = ref_mode == REF_PER_INSTANCE;
        tx = {d_xref, per ? (long)ex() : 0L, 0L, (long)nx, LONG_MAX};
        tu = {d_uref, per ? (long)eu() : 0L, 0L, 0L, LONG_MAX};
    }
    const double *c = d_metric_cfg;
    const MetricConfig cfg{c, c + nx, (metric_limits & 1) ? c + nx + nu : nullptr, (metric_limits & 2) ? c + 2 * nx + nu : nullptr,
                           (metric_limits & 4) ? c + 3 * nx + nu : nullptr, (metric_limits & 8) ? c + 3 * nx + 2 * nu : nullptr};
    // lanes per instance: the power of two that holds the steps, 8 at the most (a longer loop takes more trips)
    const int lanes = mpc_steps >= 5 ? 8 : (mpc_steps >= 3 ? 4 : mpc_steps);
    const long per = METRIC_THREADS / lanes, groups = (batch + per - 1) / per;
    auto kernel = lanes == 8 ? rollout_metrics_kernel<8> : (lanes == 4 ? rollout_metrics_kernel<4> : (lanes == 2 ? rollout_metrics_kernel<2> : rollout_metrics_kernel<1>));
    kernel<<<(unsigned)groups, METRIC_THREADS, 0, stream>>>(d_metrics, d_mpc_x, d_mpc_u, d_mpc_iter, tx, tu, cfg, nx, nu, mpc_steps, (long)batch);
    HIP_TRY(hipGetLastError());
    return record_done(stream);
}

int Solver::get_rollout_metrics(double *per_instance) {
    if (!metrics_on || !per_instance) {
        set_error("get_rollout_metrics: metrics are not enabled (set_rollout_metrics), or a null buffer");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    HIP_TRY(hipMemcpy(per_instance, d_metrics, (size_t)batch * METRIC_COUNT * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int Solver::get_rollout_summary(double *summary) {
    if (!metrics_on || !summary) {
        set_error("get_rollout_summary: metrics are not enabled (set_rollout_metrics), or a null buffer");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    const int groups = (int)std::min<long>(((long)batch + METRIC_THREADS - 1) / METRIC_THREADS, METRIC_SUMMARY_GROUPS);
    double *d_sum = d_metric_part + (size_t)METRIC_SUMMARY_GROUPS * METRIC_SUMMARY;
    metrics_summary_kernel<<<(unsigned)groups, METRIC_THREADS>>>(d_metric_part, d_metrics, (long)batch);
    metrics_summary_final_kernel<<<1, 64>>>(d_sum, d_metric_part, groups);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(summary, d_sum, METRIC_SUMMARY * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace tmpc
