// THE RULE of the infinite-horizon Riccati setup (host_setup.cpp: precompute_cache, the reference's tiny_setup +
// tiny_precompute_and_set_cache), stated once for the device kernel (families_setup.hip: riccati_families_kernel) and for the
// host export tinympc_host_family_cache (capi.hip).  fp64 throughout, A nx x nx, B nx x nu, column-major:
//   Qd = diag(Q) + rho, Rd = diag(R) + rho (off-diagonals of Q, R are dropped); the recursion runs on Q1 = Qd + rho, R1 = Rd + rho
//   from P = rho I;
//   sweep    K = (R1 + B'PB)^-1 B'PA by LU with partial pivoting (first row of the largest magnitude; an exactly zero pivot:
//            singular), P' = Q1 + (A'P)(A - BK);
//   exit     max|K - K_prev| < 1e-5 (K_prev = 0 before the first sweep): that sweep's K and P' are kept; otherwise K_prev = K,
//            P = P'.  At most 1000 sweeps: an instance at the cap keeps its last K and P'.  Non-finite values get no special
//            handling: the cap ends every loop;
//   then     Quu_inv = (R1 + B'P'B)^-1 (the same LU on the identity), AmBKt = (A - BK)'.
// Every matrix product is sum_l X(i, l) Y(l, j) from 0.0 with l ascending, the diagonal term added to the finished sum — the
// order of precompute_cache — and no product is contracted with the add behind it (fp contract off in every function below):
// on finite values the rule's results are those of precompute_cache to the last bit, on the host and on the device.  (What
// precompute_cache does beyond it — skipping a product whose right factor is exactly zero — shows only where an intermediate
// is infinite.)
//
// The rule is written per COLUMN j of the nx-wide matrices, over operands every column reads ("shared", column-major): the
// device kernel gives a column to a lane and keeps the shared operands in LDS, the host loops over the columns.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TMPC_RIC_HD __host__ __device__ __forceinline__
#else
#define TMPC_RIC_HD inline
#endif

namespace tmpc {

constexpr int RICCATI_MAX_SWEEPS = 1000;
constexpr double RICCATI_TOL = 1e-5;

template <int NX, int NU>
struct Riccati {
    // the cache image of one instance: element offsets of Kinf (nu x nx), Pinf (nx x nx), Quu_inv (nu x nu), AmBKt (nx x nx),
    // each column-major
    static constexpr int E_K = 0, E_P = NU * NX, E_QI = E_P + NX * NX, E_AT = E_QI + NU * NU, ELEMS = E_AT + NX * NX;

    // column j of B'P from column j of P: out[a] = sum_l B(l, a) Pc[l]
    static TMPC_RIC_HD void btp_col(const double *B, const double (&Pc)[NX], double (&out)[NU]) {
#pragma clang fp contract(off)
#pragma unroll
        for (int a = 0; a < NU; ++a) {
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < NX; ++l) acc = acc + B[l + a * NX] * Pc[l];
            out[a] = acc;
        }
    }

    // S = R1 + (B'P) B, whole (nu x nu): BtP nu x nx shared
    static TMPC_RIC_HD void s_matrix(const double *BtP, const double *B, const double (&R1)[NU], double (&S)[NU][NU]) {
#pragma clang fp contract(off)
#pragma unroll
        for (int a = 0; a < NU; ++a)
#pragma unroll
            for (int c = 0; c < NU; ++c) S[a][c] = 0.0;
#pragma unroll
        for (int l = 0; l < NX; ++l)   // (l outermost: a column of B'P and a row of B live at a time; every sum still runs l ascending)
#pragma unroll
            for (int a = 0; a < NU; ++a)
#pragma unroll
                for (int c = 0; c < NU; ++c) S[a][c] = S[a][c] + BtP[a + l * NU] * B[l + c * NX];
#pragma unroll
        for (int a = 0; a < NU; ++a)
#pragma unroll
            for (int c = 0; c < NU; ++c) S[a][c] = (a == c ? R1[a] : 0.0) + S[a][c];
    }

    // column j of (B'P) A from column j of A
    static TMPC_RIC_HD void rhs_col(const double *BtP, const double (&Ac)[NX], double (&out)[NU]) {
#pragma clang fp contract(off)
#pragma unroll
        for (int a = 0; a < NU; ++a) {
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < NX; ++l) acc = acc + BtP[a + l * NU] * Ac[l];
            out[a] = acc;
        }
    }

    // S X = Rhs for NR columns (rhs[r]: column r, solved in place) by LU with partial pivoting; S is the caller's copy.  The
    // elimination of S does not depend on the columns, and no column on another: solving them one at a time is the same
    // arithmetic.  false: an exactly zero pivot.  Every index is a compile-time constant (the pivot row is brought up by
    // conditional swaps), so nothing here needs an addressable array.
    template <int NR>
    static TMPC_RIC_HD bool lu_solve(double (&S)[NU][NU], double (&rhs)[NR][NU]) {
#pragma clang fp contract(off)
        bool ok = true;
#pragma unroll
        for (int c = 0; c < NU; ++c) {
            int piv = c;
            double best = fabs(S[c][c]);
#pragma unroll
            for (int i = c + 1; i < NU; ++i) {
                const double v = fabs(S[i][c]);
                if (v > best) best = v, piv = i;
            }
#pragma unroll
            for (int i = c + 1; i < NU; ++i) {
                const bool sw = piv == i;
#pragma unroll
                for (int j = 0; j < NU; ++j) {
                    const double t = S[c][j];
                    S[c][j] = sw ? S[i][j] : t;
                    S[i][j] = sw ? t : S[i][j];
                }
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const double t = rhs[r][c];
                    rhs[r][c] = sw ? rhs[r][i] : t;
                    rhs[r][i] = sw ? t : rhs[r][i];
                }
            }
            if (S[c][c] == 0.0) ok = false;
#pragma unroll
            for (int i = c + 1; i < NU; ++i) {
                const double f = S[i][c] / S[c][c];
                if (f != 0.0) {
#pragma unroll
                    for (int j = c; j < NU; ++j) S[i][j] = S[i][j] - f * S[c][j];
#pragma unroll
                    for (int r = 0; r < NR; ++r) rhs[r][i] = rhs[r][i] - f * rhs[r][c];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int i = NU - 1; i >= 0; --i) {
                double acc = rhs[r][i];
#pragma unroll
                for (int l = i + 1; l < NU; ++l) acc = acc - S[i][l] * rhs[r][l];
                rhs[r][i] = acc / S[i][i];
            }
        return ok;
    }

    // column j of A - BK from column j of A and of K
    static TMPC_RIC_HD void ambk_col(const double *B, const double (&Ac)[NX], const double (&Kc)[NU], double (&out)[NX]) {
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            double acc = 0.0;
#pragma unroll
            for (int a = 0; a < NU; ++a) acc = acc + B[i + a * NX] * Kc[a];
            out[i] = Ac[i] - acc;
        }
    }

    // column j of A'P from column j of P: A shared
    static TMPC_RIC_HD void atp_col(const double *A, const double (&Pc)[NX], double (&out)[NX]) {
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < NX; ++l) acc = acc + A[l + i * NX] * Pc[l];
            out[i] = acc;
        }
    }

    // column j of P' = Q1 + (A'P)(A - BK) from column j of A - BK: AtP shared; q1j = Q1[j]
    static TMPC_RIC_HD void pn_col(const double *AtP, const double (&Mc)[NX], int j, double q1j, double (&out)[NX]) {
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < NX; ++l) acc = acc + AtP[i + l * NX] * Mc[l];
            out[i] = (i == j ? q1j : 0.0) + acc;
        }
    }

    // max|K - K_prev| over column j (the exit test takes the largest over the columns)
    static TMPC_RIC_HD double dk_col(const double (&Kc)[NU], const double (&Kp)[NU]) {
        double dk = 0.0;
#pragma unroll
        for (int a = 0; a < NU; ++a) dk = fmax(dk, fabs(Kc[a] - Kp[a]));
        return dk;
    }
};

// The rule for one family on the host.  Qdiag, Rdiag: the diagonals of Q and R as given (rho not yet added).  Kinf nu x nx, Pinf
// nx x nx, Quu_inv nu x nu, AmBKt nx x nx column-major out; *sweeps: the sweeps run (1000: the cap).  Returns 0, or 1: singular
// (*sweeps = -1, the outputs are not meaningful).
template <int NX, int NU>
inline int riccati_host(const double *A, const double *B, const double *Qdiag, const double *Rdiag, double rho, double *Kinf,
                        double *Pinf, double *Quu_inv, double *AmBKt, int *sweeps) {
    using R = Riccati<NX, NU>;
    double Q1[NX], R1[NU], P[NX][NX], Pn[NX][NX], Ac[NX][NX], M[NX][NX], K[NX][NU], Kp[NX][NU], BtP[NU * NX], AtP[NX * NX];
    for (int i = 0; i < NX; ++i) Q1[i] = (Qdiag[i] + rho) + rho;
    for (int a = 0; a < NU; ++a) R1[a] = (Rdiag[a] + rho) + rho;
    for (int j = 0; j < NX; ++j) {
        for (int i = 0; i < NX; ++i) P[j][i] = i == j ? rho : 0.0, Pn[j][i] = 0.0, Ac[j][i] = A[i + j * NX], M[j][i] = 0.0;
        for (int a = 0; a < NU; ++a) K[j][a] = Kp[j][a] = 0.0;
    }
    if (sweeps) *sweeps = -1;
    int it = 0;
    for (; it < RICCATI_MAX_SWEEPS; ++it) {
        for (int j = 0; j < NX; ++j) {
            double c[NU];
            R::btp_col(B, P[j], c);
            for (int a = 0; a < NU; ++a) BtP[a + j * NU] = c[a];
        }
        double S[NU][NU];
        R::s_matrix(BtP, B, R1, S);
        for (int j = 0; j < NX; ++j) R::rhs_col(BtP, Ac[j], K[j]);
        if (!R::template lu_solve<NX>(S, K)) return 1;
        double dk = 0.0;
        for (int j = 0; j < NX; ++j) {
            R::ambk_col(B, Ac[j], K[j], M[j]);
            double c[NX];
            R::atp_col(A, P[j], c);
            for (int i = 0; i < NX; ++i) AtP[i + j * NX] = c[i];
            dk = fmax(dk, R::dk_col(K[j], Kp[j]));
        }
        for (int j = 0; j < NX; ++j) R::pn_col(AtP, M[j], j, Q1[j], Pn[j]);
        if (dk < RICCATI_TOL) {
            ++it;
            break;
        }
        for (int j = 0; j < NX; ++j) {
            for (int a = 0; a < NU; ++a) Kp[j][a] = K[j][a];
            for (int i = 0; i < NX; ++i) P[j][i] = Pn[j][i];
        }
    }
    for (int j = 0; j < NX; ++j) {
        double c[NU];
        R::btp_col(B, Pn[j], c);
        for (int a = 0; a < NU; ++a) BtP[a + j * NU] = c[a];
    }
    double S[NU][NU], I[NU][NU];
    R::s_matrix(BtP, B, R1, S);
    for (int a = 0; a < NU; ++a)
        for (int c = 0; c < NU; ++c) I[a][c] = a == c ? 1.0 : 0.0;
    if (!R::template lu_solve<NU>(S, I)) return 1;
    for (int j = 0; j < NX; ++j) {
        for (int a = 0; a < NU; ++a) Kinf[a + j * NU] = K[j][a];
        for (int i = 0; i < NX; ++i) Pinf[i + j * NX] = Pn[j][i], AmBKt[j + i * NX] = M[j][i];
    }
    for (int c = 0; c < NU; ++c)
        for (int a = 0; a < NU; ++a) Quu_inv[a + c * NU] = I[c][a];
    if (sweeps) *sweeps = it;
    return 0;
}

}  // namespace tmpc
