// Setup of a per-instance-family solver on the device: the Riccati recursion of every instance
// (riccati_families_kernel; the rule: riccati.h) and the stream kernel's per-instance coefficient pack written where the solves
// read it (fill_family_pack_kernel; the element map: fill_streamg_role, streamg_entry.hip.h).
#include <hip/hip_runtime.h>

#include "riccati.h"
#include "solver.h"
#include "streamg_entry.hip.h"

namespace tmpc {

// ---- Riccati ----------------------------------------------------------------------------------------------------------------
// A group of 16 lanes (a DPP row) per instance, four instances per wavefront, one wavefront per workgroup.  Lane j < NX owns
// COLUMN j of every nx-wide matrix (A, P, P', A - BK, K, B'P, A'P) in registers: each product of the sweep then needs one
// operand whole — B, B'P, A, A'P — and those live in LDS, written by their columns' owners and read by the whole group at one
// address (a broadcast read; the four groups' blocks are RIC_STRIDE doubles apart, which puts their reads on different banks).
// The nu x nu system S is built and factored in every lane (replicated: no exchange), each lane solving its own column.  Two
// barriers a sweep (B'P complete; A'P and the columns' |dK| complete) — of a one-wavefront workgroup, so they cost a wait for
// the LDS counter and nothing else.
// An instance leaves the recursion at its own sweep: its group's `run` goes false and from then on its lanes only keep the
// barriers company until the last of the four is done.  Nothing an instance computes depends on anything but its own inputs:
// a group reads its own LDS block and its own registers.
constexpr int RIC_GROUP = 16, RIC_PER_BLOCK = 4, RIC_THREADS = RIC_GROUP * RIC_PER_BLOCK;

template <int NX, int NU>
struct RicLds {
    static constexpr int O_A = 0, O_B = O_A + NX * NX, O_BTP = O_B + NX * NU, O_ATP = O_BTP + NU * NX, O_DK = O_ATP + NX * NX,
                         USED = O_DK + RIC_GROUP;
    static constexpr int STRIDE = (USED + 13) / 16 * 16 + 2;   // = 2 mod 16 doubles: the four groups' broadcast reads four banks apart
};

template <int NX, int NU>
__global__ void __launch_bounds__(RIC_THREADS)
riccati_families_kernel(const double *__restrict__ A, const double *__restrict__ B, const double *__restrict__ Qdiag,
                        const double *__restrict__ Rdiag, const double *__restrict__ rho, int batch, double *__restrict__ img,
                        int *__restrict__ sweeps) {
    static_assert(NX <= RIC_GROUP, "a column per lane of the group");
    using R = Riccati<NX, NU>;
    using L = RicLds<NX, NU>;
    __shared__ double lds[RIC_PER_BLOCK * L::STRIDE];
    const int j = threadIdx.x % RIC_GROUP, g = threadIdx.x / RIC_GROUP;
    const long b = (long)blockIdx.x * RIC_PER_BLOCK + g;
    double *sh = lds + g * L::STRIDE;
    const bool inst = b < batch, col = inst && j < NX;
    const long bb = inst ? b : 0;   // (lanes without an instance or a column load instance 0's and commit nothing)
    const int jj = j < NX ? j : 0;

    // Pc: column j of P going into a sweep and of P' coming out of it (the sweep that ends an instance leaves its P' there, and
    // the next sweep of the others starts from theirs); Kc / Kp: of this sweep's K and the one before; Mc: of A - B K
    double Pc[NX], Mc[NX], Kc[NU], Kp[NU], R1[NU];
    const double r = rho[bb];
    const double q1j = (Qdiag[bb * NX + jj] + r) + r;
#pragma unroll
    for (int a = 0; a < NU; ++a) R1[a] = (Rdiag[bb * NU + a] + r) + r, Kc[a] = 0.0, Kp[a] = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        Pc[i] = i == jj ? r : 0.0, Mc[i] = 0.0;
        if (col) sh[L::O_A + i + j * NX] = A[bb * (NX * NX) + j * NX + i];
    }
    if (inst)
        for (int e = j; e < NX * NU; e += RIC_GROUP) sh[L::O_B + e] = B[bb * (NX * NU) + e];
    sh[L::O_DK + j] = 0.0;   // (the lanes past NX never write theirs again: zeros under the maximum)

    bool run = inst, singular = false;
    int done_at = RICCATI_MAX_SWEEPS;
    for (int it = 0; it < RICCATI_MAX_SWEEPS && __any(run); ++it) {
        if (run && col) {
            double c[NU];
            R::btp_col(sh + L::O_B, Pc, c);
#pragma unroll
            for (int a = 0; a < NU; ++a) sh[L::O_BTP + a + j * NU] = c[a];
        }
        __syncthreads();
        if (run) {
            double S[NU][NU], x[1][NU];
            R::s_matrix(sh + L::O_BTP, sh + L::O_B, R1, S);
            double Ac[NX];   // (column j of A comes from LDS where it is used: held in registers it costs a wavefront per SIMD at nx = 12)
#pragma unroll
            for (int i = 0; i < NX; ++i) Ac[i] = sh[L::O_A + i + jj * NX];
            R::rhs_col(sh + L::O_BTP, Ac, x[0]);
            if (!R::template lu_solve<1>(S, x)) singular = true;   // (S is the same in every lane of the group: so is this)
#pragma unroll
            for (int a = 0; a < NU; ++a) Kc[a] = x[0][a];
            if (col) {
                double c[NX];
                R::atp_col(sh + L::O_A, Pc, c);
#pragma unroll
                for (int i = 0; i < NX; ++i) sh[L::O_ATP + i + j * NX] = c[i];
                sh[L::O_DK + j] = R::dk_col(Kc, Kp);
            }
        }
        __syncthreads();
        if (run) {
            if (singular) {
                run = false;
            } else {
                double Ac[NX];
#pragma unroll
                for (int i = 0; i < NX; ++i) Ac[i] = sh[L::O_A + i + jj * NX];
                R::ambk_col(sh + L::O_B, Ac, Kc, Mc);
                R::pn_col(sh + L::O_ATP, Mc, jj, q1j, Pc);
                double dk = 0.0;
#pragma unroll
                for (int l = 0; l < NX; ++l) dk = fmax(dk, sh[L::O_DK + l]);
                if (dk < RICCATI_TOL) done_at = it + 1, run = false;
#pragma unroll
                for (int a = 0; a < NU; ++a) Kp[a] = Kc[a];
            }
        }
    }
    // Quu_inv = (R1 + B'P'B)^-1: lane a < NU solves column a of the identity
    const bool fin = inst && !singular;
    if (fin && col) {
        double c[NU];
        R::btp_col(sh + L::O_B, Pc, c);
#pragma unroll
        for (int a = 0; a < NU; ++a) sh[L::O_BTP + a + j * NU] = c[a];
    }
    __syncthreads();
    if (!inst) return;
    const size_t Bn = (size_t)batch;
    if (fin) {
        double S[NU][NU], x[1][NU];
        R::s_matrix(sh + L::O_BTP, sh + L::O_B, R1, S);
#pragma unroll
        for (int a = 0; a < NU; ++a) x[0][a] = a == j ? 1.0 : 0.0;
        if (!R::template lu_solve<1>(S, x)) singular = true;
        if (!singular) {
            if (j < NU)
#pragma unroll
                for (int a = 0; a < NU; ++a) img[(size_t)(R::E_QI + a + j * NU) * Bn + b] = x[0][a];
            if (col) {
#pragma unroll
                for (int a = 0; a < NU; ++a) img[(size_t)(R::E_K + a + j * NU) * Bn + b] = Kc[a];
#pragma unroll
                for (int i = 0; i < NX; ++i) {
                    img[(size_t)(R::E_P + i + j * NX) * Bn + b] = Pc[i];
                    img[(size_t)(R::E_AT + j + i * NX) * Bn + b] = Mc[i];
                }
            }
        }
    }
    if (j == 0) sweeps[b] = singular ? -1 : done_at;
}

// ---- pack fill --------------------------------------------------------------------------------------------------------------
// the cache image [element][batch] read as fill_streamg_role reads a Cache
template <int NX, int NU>
struct ImageCacheView {
    using R = Riccati<NX, NU>;
    const double *img;
    size_t Bn, b;
    __device__ double Kinf(int a, int j) const { return img[(size_t)(R::E_K + a + j * NU) * Bn + b]; }
    __device__ double Pinf(int i, int j) const { return img[(size_t)(R::E_P + i + j * NX) * Bn + b]; }
    __device__ double Quu_inv(int a, int c) const { return img[(size_t)(R::E_QI + a + c * NU) * Bn + b]; }
    __device__ double AmBKt(int i, int j) const { return img[(size_t)(R::E_AT + i + j * NX) * Bn + b]; }
};

struct FdynArg {
    double f[16];
};

// One lane per COLUMN of the pack, [element][G * batch + role]: consecutive lanes take consecutive (instance, role) columns, so
// every element's row is written as whole contiguous lines.  The elements no role writes (padding, rows past nx / nu) are
// zeroed by the launcher beforehand, as the host fill zeroes them.  The role-0 lane also writes its instance's column of
// het_aux [diag(Q) + rho | diag(R) + rho | rho][batch] in fp32.
template <int NX, int NU, int G, class RT>
__global__ void __launch_bounds__(256)
fill_family_pack_kernel(const double *__restrict__ img, const double *__restrict__ A, const double *__restrict__ B, FdynArg fd,
                        const double *__restrict__ Qdiag, const double *__restrict__ Rdiag, const double *__restrict__ rho, int batch,
                        RT *__restrict__ coef, float *__restrict__ aux) {
    const size_t Bn = (size_t)batch, B4 = (size_t)G * Bn;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B4) return;
    const size_t b = t / G;
    const int q = (int)(t % G);
    const ImageCacheView<NX, NU> c{img, Bn, b};
    fill_streamg_role<NX, NU, G>(q, A + b * (NX * NX), B + b * (NX * NU), c, fd.f,
                                 [&](int, int idx, double v) { coef[(size_t)idx * B4 + t] = (RT)v; });
    if (q == 0) {
        const double r = rho[b];
        for (int i = 0; i < NX; ++i) aux[(size_t)i * Bn + b] = (float)(Qdiag[b * NX + i] + r);
        for (int a = 0; a < NU; ++a) aux[(size_t)(NX + a) * Bn + b] = (float)(Rdiag[b * NU + a] + r);
        aux[(size_t)(NX + NU) * Bn + b] = (float)r;
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------
namespace {

constexpr int FAM_G = 4;   // lanes per instance of the stream kernel as instantiated (kernels.hip: stream4)

template <int NX, int NU>
hipError_t launch_riccati(const FamilyInputs &in, int batch, double *img, int *sweeps, hipStream_t stream) {
    const int grid = (batch + RIC_PER_BLOCK - 1) / RIC_PER_BLOCK;
    hipLaunchKernelGGL((riccati_families_kernel<NX, NU>), dim3(grid), dim3(RIC_THREADS), 0, stream, in.A, in.B, in.Qdiag, in.Rdiag,
                       in.rho, batch, img, sweeps);
    return hipGetLastError();
}

template <int NX, int NU>
hipError_t launch_fill(const double *img, const FamilyInputs &in, const double *fdyn, int batch, int precision, void *coef, float *aux,
                       hipStream_t stream) {
    using PK = StreamPackG<NX, NU, FAM_G>;
    const size_t cols = (size_t)FAM_G * batch;
    hipError_t e = hipMemsetAsync(coef, 0, (size_t)PK::CP * cols * (precision == 1 ? sizeof(float) : sizeof(double)), stream);
    if (e != hipSuccess) return e;
    FdynArg fd;
    for (int i = 0; i < 16; ++i) fd.f[i] = i < NX ? fdyn[i] : 0.0;
    const int grid = (int)((cols + 255) / 256);
    if (precision == 1)
        hipLaunchKernelGGL((fill_family_pack_kernel<NX, NU, FAM_G, float>), dim3(grid), dim3(256), 0, stream, img, in.A, in.B, fd,
                           in.Qdiag, in.Rdiag, in.rho, batch, (float *)coef, aux);
    else
        hipLaunchKernelGGL((fill_family_pack_kernel<NX, NU, FAM_G, double>), dim3(grid), dim3(256), 0, stream, img, in.A, in.B, fd,
                           in.Qdiag, in.Rdiag, in.rho, batch, (double *)coef, aux);
    return hipGetLastError();
}

struct FamilyShape {
    int nx, nu;
    int pack_elems;
    hipError_t (*riccati)(const FamilyInputs &, int, double *, int *, hipStream_t);
    hipError_t (*fill)(const double *, const FamilyInputs &, const double *, int, int, void *, float *, hipStream_t);
    int (*host)(const double *, const double *, const double *, const double *, double, double *, double *, double *, double *, int *);
};

#define TMPC_FAMILY_SHAPE(NX, NU)                                                                                           \
    {NX, NU, StreamPackG<NX, NU, FAM_G>::CP, &launch_riccati<NX, NU>, &launch_fill<NX, NU>, &riccati_host<NX, NU>}
#define TMPC_FAMILY_SHAPES(NX) TMPC_FAMILY_SHAPE(NX, 1), TMPC_FAMILY_SHAPE(NX, 2), TMPC_FAMILY_SHAPE(NX, 3), TMPC_FAMILY_SHAPE(NX, 4)
// the stream kernel's grid (kernels.hip), which is what tinympc_create_families accepts
const FamilyShape kShapes[] = {TMPC_FAMILY_SHAPES(2), TMPC_FAMILY_SHAPES(3), TMPC_FAMILY_SHAPES(4),  TMPC_FAMILY_SHAPES(6),
                               TMPC_FAMILY_SHAPES(8), TMPC_FAMILY_SHAPES(10), TMPC_FAMILY_SHAPES(12)};

const FamilyShape *find_shape(int nx, int nu) {
    for (const FamilyShape &s : kShapes)
        if (s.nx == nx && s.nu == nu) return &s;
    return nullptr;
}

}  // namespace

bool families_shape_built(int nx, int nu) { return find_shape(nx, nu) != nullptr; }
int families_cache_elems(int nx, int nu) { return nu * nx + nx * nx + nu * nu + nx * nx; }
size_t families_pack_elems(int nx, int nu, int lanes) {
    const FamilyShape *s = find_shape(nx, nu);
    return s && lanes == FAM_G ? (size_t)s->pack_elems : 0;
}

hipError_t families_riccati_launch(int nx, int nu, const FamilyInputs &in, int batch, double *img, int *sweeps, hipStream_t stream) {
    const FamilyShape *s = find_shape(nx, nu);
    return s ? s->riccati(in, batch, img, sweeps, stream) : hipErrorNotSupported;
}

hipError_t families_fill_launch(int nx, int nu, const double *img, const FamilyInputs &in, const double *fdyn, int batch, int precision,
                                void *coef, float *aux, hipStream_t stream) {
    const FamilyShape *s = find_shape(nx, nu);
    return s ? s->fill(img, in, fdyn, batch, precision, coef, aux, stream) : hipErrorNotSupported;
}

int families_host_cache(int nx, int nu, const double *A, const double *B, const double *Qdiag, const double *Rdiag, double rho, double *Kinf,
                        double *Pinf, double *Quu_inv, double *AmBKt, int *sweeps) {
    const FamilyShape *s = find_shape(nx, nu);
    return s ? s->host(A, B, Qdiag, Rdiag, rho, Kinf, Pinf, Quu_inv, AmBKt, sweeps) : -2;
}

}  // namespace tmpc
