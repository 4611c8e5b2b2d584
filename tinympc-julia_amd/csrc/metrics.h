// THE RULE of the closed loop's per-instance metrics (tinympc_set_rollout_metrics): what one logged step contributes and how
// two spans of steps combine.  One text for the device kernels (metrics.hip) and for the host export
// tinympc_host_rollout_metrics (capi.hip).  Everything is fp64; the logged values and the targets are fp32 widened to fp64.
//
// Step s of instance b: x = its logged state after the step, u = its logged control, it = its signed iteration count (negative:
// the solve hit max_iter), xr / ur = knot 1 of the x references and knot 0 of the u references that step's solve used (null:
// zero).  e = x - xr, v = u - ur.  The step gives
//   cost_x = sum_r qw[r] e[r]^2 and cost_u = sum_a rw[a] v[a]^2, rows ascending from 0.0 (a product and an add, or one fma);
//   err    = max_r |e[r]|;
//   viol   = max_r max(x[r] - x_hi[r], x_lo[r] - x[r], 0), out = any row with x[r] > x_hi[r] or x[r] < x_lo[r];
//   sat    = any row with u[a] >= u_hi[a] or u[a] <= u_lo[a];
// a null limit array is a side that never counts.  The eleven slots of a span of steps, and the combination of an earlier
// span a with a later one b (the accumulators with a rollout, a rollout's partial sums with one another):
//   0 steps         a + b
//   1 cost_x        a + b
//   2 cost_u        a + b
//   3 peak_err      max(a, b)
//   4 final_err     b's where b holds a step, else a's
//   5 x_viol_max    max(a, b)
//   6 x_viol_steps  a + b
//   7 first_viol    a's where a has one, else a.steps + b's where b has one, else 0   (1 + the index of the first step out)
//   8 u_sat_steps   a + b
//   9 iters         a + b     (|it|)
//  10 maxiter_steps a + b     (it < 0)
// Counts are doubles holding integers, exact up to 2^53.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TMPC_METRIC_HD __host__ __device__
#else
#define TMPC_METRIC_HD
#endif

namespace tmpc {

enum {
    METRIC_STEPS = 0, METRIC_COST_X, METRIC_COST_U, METRIC_PEAK_ERR, METRIC_FINAL_ERR, METRIC_X_VIOL_MAX, METRIC_X_VIOL_STEPS,
    METRIC_FIRST_VIOL, METRIC_U_SAT_STEPS, METRIC_ITERS, METRIC_MAXITER_STEPS, METRIC_COUNT
};

// weights and limits, nx / nu doubles each; a null limit array: that side never counts
struct MetricConfig {
    const double *qw, *rw, *x_lo, *x_hi, *u_lo, *u_hi;
};

struct MetricStep {
    double cost_x, cost_u, err, viol;
    bool out, sat;
};

TMPC_METRIC_HD inline MetricStep metric_step(int nx, int nu, const float *x, const float *u, const float *xr, const float *ur, const MetricConfig &c) {
    MetricStep m{0.0, 0.0, 0.0, 0.0, false, false};
    for (int r = 0; r < nx; ++r) {
        const double xv = (double)x[r], e = xv - (xr ? (double)xr[r] : 0.0), ae = fabs(e);
        m.cost_x += c.qw[r] * e * e;
        m.err = ae > m.err ? ae : m.err;
        if (c.x_hi) {
            const double d = xv - c.x_hi[r];
            m.viol = d > m.viol ? d : m.viol;
            m.out = m.out || xv > c.x_hi[r];
        }
        if (c.x_lo) {
            const double d = c.x_lo[r] - xv;
            m.viol = d > m.viol ? d : m.viol;
            m.out = m.out || xv < c.x_lo[r];
        }
    }
    for (int a = 0; a < nu; ++a) {
        const double uv = (double)u[a], v = uv - (ur ? (double)ur[a] : 0.0);
        m.cost_u += c.rw[a] * v * v;
        if (c.u_hi) m.sat = m.sat || uv >= c.u_hi[a];
        if (c.u_lo) m.sat = m.sat || uv <= c.u_lo[a];
    }
    return m;
}

// slot k of (a then b): a, b the slot's two values, a_steps / b_steps slot 0 of the two spans
TMPC_METRIC_HD inline double metric_combine(int k, double a, double b, double a_steps, double b_steps) {
    switch (k) {
    case METRIC_PEAK_ERR:
    case METRIC_X_VIOL_MAX: return a > b ? a : b;
    case METRIC_FINAL_ERR: return b_steps > 0.0 ? b : a;
    case METRIC_FIRST_VIOL: return a != 0.0 ? a : (b != 0.0 ? a_steps + b : 0.0);
    default: return a + b;
    }
}

// the eleven slots of the one-step span
TMPC_METRIC_HD inline void metric_step_slots(const MetricStep &m, int it, double *s) {
    s[METRIC_STEPS] = 1.0;
    s[METRIC_COST_X] = m.cost_x;
    s[METRIC_COST_U] = m.cost_u;
    s[METRIC_PEAK_ERR] = m.err;
    s[METRIC_FINAL_ERR] = m.err;
    s[METRIC_X_VIOL_MAX] = m.viol;
    s[METRIC_X_VIOL_STEPS] = m.out ? 1.0 : 0.0;
    s[METRIC_FIRST_VIOL] = m.out ? 1.0 : 0.0;
    s[METRIC_U_SAT_STEPS] = m.sat ? 1.0 : 0.0;
    s[METRIC_ITERS] = it < 0 ? -(double)it : (double)it;
    s[METRIC_MAXITER_STEPS] = it < 0 ? 1.0 : 0.0;
}

}  // namespace tmpc
