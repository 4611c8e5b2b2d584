// THE RULE of the closed loop's state estimator (tinympc_set_estimator): measured outputs y = C x + v, ny <= nx of them, and a
// fixed-gain observer in current-estimator form (Luenberger / steady-state Kalman), all fp64.  One text for the device kernel
// (estimator.hip) and for the host exports tinympc_host_estimator_step / tinympc_host_kalman_gain (capi.hip).
//
// C ny x nx and L nx x ny, column-major.  Per instance and step t:
//   output   y_t[i]     = (sum_j C[i + j ny] x_t[j]) + v_t[i]: acc = 0, acc = fma(C[i + j ny], x_t[j], acc) for j ascending, then one
//                         add of v_t[i] (no measurement noise: no add); x_t the true fp64 plant state, v_t[i] row i of G_v xi_v[b][t]
//                         (noise.h: noise_row on noise_pair's draws);
//   correct  e[i]       = y_t[i] - (C xhat-_t)[i], the product in the same fma order;
//            xhat_t[r]  = xhat-_t[r], then fma(L[r + i nx], e[i], .) for i ascending;
//   predict  xhat-_{t+1}[r] = f[r], then fma(A[r + j nx], xhat_t[j], .) for j ascending, then fma(B[r + a nx], u_t[a], .) for a
//                         ascending — the MODEL's A, B, f, and the order of the plant step.
// Every product below is an explicit fma and every other operation a single rounding: there is no a * b + c the compiler could
// contract in one caller and not in another.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TMPC_EST_HD __host__ __device__
#else
#define TMPC_EST_HD
#endif

namespace tmpc {

// row i of C x (no noise added)
TMPC_EST_HD inline double estimator_output_row(const double *C, int nx, int ny, int i, const double *x) {
    double acc = 0.0;
    for (int j = 0; j < nx; ++j) acc = fma(C[i + j * ny], x[j], acc);
    return acc;
}

// row r of xhat = xhat- + L e; xm: xhat-[r]
TMPC_EST_HD inline double estimator_correct_row(const double *L, int nx, int ny, int r, double xm, const double *e) {
    for (int i = 0; i < ny; ++i) xm = fma(L[r + i * nx], e[i], xm);
    return xm;
}

// row r of xhat-+ = f + A xhat + B u; model: [A | B | f] column-major; U: float on the device (the solution buffer), double on the host
template <class U>
TMPC_EST_HD inline double estimator_predict_row(const double *model, int nx, int nu, int r, const double *xhat, const U *u) {
    const double *A = model, *B = model + nx * nx;
    double acc = B[nx * nu + r];
    for (int j = 0; j < nx; ++j) acc = fma(A[r + j * nx], xhat[j], acc);
    for (int a = 0; a < nu; ++a) acc = fma(B[r + a * nx], (double)u[a], acc);
    return acc;
}

// One step of the rule for one instance on the host, in the device kernel's order: predict (from xhat and u, with model
// [A | B | f]) and / or correct (with the true state x, and v: ny rows of output noise or null).  xhat: nx in, nx out; y: ny out
// (written where correct).
inline void estimator_step_host(int nx, int nu, int ny, bool predict, bool correct, const double *model, const double *C, const double *L,
                                const double *u, const double *x, const double *v, double *xhat, double *y) {
    std::vector<double> xm(xhat, xhat + nx), e(ny > 0 ? ny : 1);
    if (predict)
        for (int r = 0; r < nx; ++r) xm[r] = estimator_predict_row(model, nx, nu, r, xhat, u);
    if (correct) {
        for (int i = 0; i < ny; ++i) {
            double yi = estimator_output_row(C, nx, ny, i, x);
            if (v) yi = yi + v[i];
            y[i] = yi;
            e[i] = yi - estimator_output_row(C, nx, ny, i, xm.data());
        }
        for (int r = 0; r < nx; ++r) xhat[r] = estimator_correct_row(L, nx, ny, r, xm[r], e.data());
    } else {
        for (int r = 0; r < nx; ++r) xhat[r] = xm[r];
    }
}

// The steady-state gain of the filter Riccati recursion P <- A (P - P C' (C P C' + V)^-1 C P) A' + W from P = W (host only; all
// column-major): iterated until the update is <= 1e-13 of |P|_inf, the ny x ny solves by Cholesky; L = P C' (C P C' + V)^-1 and
// the prediction covariance P.  false with a reason: a non-positive pivot, or no convergence in 100 000 iterations (an
// undetectable pair grows without bound).
inline bool kalman_gain_host(const double *A, const double *C, const double *W, const double *V, int nx, int ny, double *L, double *P,
                             std::string &why) {
    const size_t n = (size_t)nx, m = (size_t)ny;
    std::vector<double> Pk(W, W + n * n), PCt(n * m), S(m * m), K(n * m), M(n * n), AM(n * n), Pn(n * n), t(m);
    // K = P C' S^-1 of a covariance Pc, S = C Pc C' + V factored as G G' (G lower triangular, in place); false on a bad pivot
    auto gain = [&](const std::vector<double> &Pc) {
        for (size_t r = 0; r < n; ++r)
            for (size_t i = 0; i < m; ++i) {
                double a = 0.0;
                for (size_t j = 0; j < n; ++j) a += Pc[r + j * n] * C[i + j * m];
                PCt[r + i * n] = a;
            }
        for (size_t i = 0; i < m; ++i)
            for (size_t k = 0; k < m; ++k) {
                double a = V[i + k * m];
                for (size_t j = 0; j < n; ++j) a += C[i + j * m] * PCt[j + k * n];
                S[i + k * m] = a;
            }
        for (size_t i = 0; i < m; ++i)   // symmetrise, then the lower Cholesky factor in place
            for (size_t k = 0; k < i; ++k) S[i + k * m] = S[k + i * m] = 0.5 * (S[i + k * m] + S[k + i * m]);
        for (size_t k = 0; k < m; ++k) {
            double d = S[k + k * m];
            for (size_t j = 0; j < k; ++j) d -= S[k + j * m] * S[k + j * m];
            if (d <= 0.0) return false;
            d = std::sqrt(d);
            S[k + k * m] = d;
            for (size_t i = k + 1; i < m; ++i) {
                double a = S[i + k * m];
                for (size_t j = 0; j < k; ++j) a -= S[i + j * m] * S[k + j * m];
                S[i + k * m] = a / d;
            }
        }
        // K S = PCt: every row of K solves G G' k' = pct'
        for (size_t r = 0; r < n; ++r) {
            for (size_t i = 0; i < m; ++i) {
                double a = PCt[r + i * n];
                for (size_t j = 0; j < i; ++j) a -= S[i + j * m] * t[j];
                t[i] = a / S[i + i * m];
            }
            for (size_t ii = m; ii-- > 0;) {
                double a = t[ii];
                for (size_t j = ii + 1; j < m; ++j) a -= S[j + ii * m] * t[j];
                t[ii] = a / S[ii + ii * m];
            }
            for (size_t i = 0; i < m; ++i) K[r + i * n] = t[i];
        }
        return true;
    };
    auto norm_inf = [&](const std::vector<double> &X) {
        double best = 0.0;
        for (size_t r = 0; r < n; ++r) {
            double s = 0.0;
            for (size_t j = 0; j < n; ++j) s += std::fabs(X[r + j * n]);
            best = s > best ? s : best;
        }
        return best;
    };
    bool converged = false;
    for (int it = 0; it < 100000 && !converged; ++it) {
        if (!gain(Pk)) {
            why = "a non-positive pivot in the Cholesky factor of C P C' + V at iteration " + std::to_string(it) + " (V has to be positive definite on the measured rows, and the pair (A, C) detectable)";
            return false;
        }
        // M = P - K (C P) = P - K PCt'
        for (size_t r = 0; r < n; ++r)
            for (size_t c = 0; c < n; ++c) {
                double a = Pk[r + c * n];
                for (size_t i = 0; i < m; ++i) a -= K[r + i * n] * PCt[c + i * n];
                M[r + c * n] = a;
            }
        for (size_t r = 0; r < n; ++r)
            for (size_t c = 0; c < n; ++c) {
                double a = 0.0;
                for (size_t j = 0; j < n; ++j) a += A[r + j * n] * M[j + c * n];
                AM[r + c * n] = a;
            }
        for (size_t r = 0; r < n; ++r)
            for (size_t c = 0; c < n; ++c) {
                double a = W[r + c * n];
                for (size_t j = 0; j < n; ++j) a += AM[r + j * n] * A[c + j * n];
                Pn[r + c * n] = a;
            }
        for (size_t r = 0; r < n; ++r)   // (keep it symmetric)
            for (size_t c = 0; c < r; ++c) Pn[r + c * n] = Pn[c + r * n] = 0.5 * (Pn[r + c * n] + Pn[c + r * n]);
        double diff = 0.0;
        for (size_t r = 0; r < n; ++r) {
            double s = 0.0;
            for (size_t j = 0; j < n; ++j) s += std::fabs(Pn[r + j * n] - Pk[r + j * n]);
            diff = s > diff ? s : diff;
        }
        const double scale = norm_inf(Pn);
        if (scale >= 1e300) {   // (checked every iteration, so before anything is infinite)
            why = "the covariance recursion grew past 1e300 at iteration " + std::to_string(it) + " (the pair (A, C) is not detectable)";
            return false;
        }
        converged = diff <= 1e-13 * scale;
        Pk.swap(Pn);
    }
    if (!converged) {
        why = "the filter Riccati recursion did not converge in 100000 iterations (the pair (A, C) is not detectable, or (A, W) has an uncontrollable mode on the unit circle)";
        return false;
    }
    if (!gain(Pk)) {
        why = "a non-positive pivot in the Cholesky factor of C P C' + V at the fixed point";
        return false;
    }
    for (size_t i = 0; i < n * m; ++i) L[i] = K[i];
    if (P)
        for (size_t i = 0; i < n * n; ++i) P[i] = Pk[i];
    return true;
}

}  // namespace tmpc
