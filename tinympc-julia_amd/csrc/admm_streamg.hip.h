// Fused ADMM kernel with a run-time horizon, G = 1, 2 or 4 lanes per instance: "stream<G>".
//
// For shapes / options without an unrolled quad-kernel instantiation (admm_quad.hip.h): any horizon, the
// affine dynamics term, second-order cones, linear inequalities, one problem family per instance.  The knot loops are rolled and the
// per-instance trajectories are streamed through a scratch block in HBM / Infinity Cache, D knots ahead of
// their use; the lane mapping is the quad kernel's (lane q of a group owns state rows [q*RX,(q+1)*RX) and
// input rows [q*RU,(q+1)*RU), mat-vec operands fetched with DPP quad_perm broadcasts).
//   * G trades instruction efficiency against parallelism: one lane per instance executes the fewest
//     instructions per instance but fills the chip only from ~65 536 instances up; four lanes put 4x the
//     wavefronts in flight at ~2x the instructions.  G = 4 is what is instantiated (kernels.hip): measured, 1 and 2
//     lanes are no faster at any batch size, because from ~32 768 instances up all three are bound by the state stream.
//   * scratch layout [array][knot][instance][row] with the real nx / nu rows only: a lane's rows are one
//     contiguous (vector) access, a wavefront's instances one contiguous span, no padding rows travel;
//   * one-shot solves (cold start, workspace not kept: OS) update vnew / znew in place and hand the backward
//     sweep one fused array (vnew - g [+ the cone set's]) instead of four: 10 instead of 14 state-shaped and
//     12 instead of 16 input-shaped float transfers per knot and iteration (6 and 8 when no residual check
//     reads vnew / znew back);
//   * one family for the batch: coefficient rows per lane role in LDS (conflict-free image, as in the
//     quad kernel); one family per instance (HET): the same rows as per-lane columns in HBM;
//   * second-order cones may straddle lanes: squared head norms and the axis value are summed over
//     the group with DPP steps.
#ifndef TMPC_ADMM_STREAMG_HIP_H   // (no #pragma once: the file includes itself four times, at its end, for the loop form's, the per-instance-bounds form's, the per-instance-rows form's and the per-instance-cones form's entry points)
#define TMPC_ADMM_STREAMG_HIP_H
#define TMPC_STREAMG_MPC 0
#define TMPC_STREAMG_IB 0
#define TMPC_STREAMG_IL 0
#define TMPC_STREAMG_IC 0
#include <hip/hip_runtime.h>

#include <cfloat>

#include "admm_generic.hip.h"   // Ws64, the type-generic gmin / gmax / gsqrt / gfma / gupmax
#include "admm_params.h"
#include "admm_quad.hip.h"

namespace tmpc {

// Pack per lane role: the quad kernel's three blocks (QuadShape offsets; N plays no role in them) + the affine block
template <int NX, int NU, int G>
struct StreamPackG {
    using S = QuadShape<NX, NU, 2, G>;
    static constexpr int RX = S::RX, RU = S::RU;
    static constexpr int O_F = S::CP, O_APF = O_F + RX, O_BPF = O_APF + RX;
    static constexpr int O_ATT = S::pad8(O_BPF + RU);   // A^T rows [RX][NXP] (adaptive rho: the dual residual's A' g)
    static constexpr int CP = O_ATT + S::pad8(RX * S::NXP);
    // adaptive rho (ADP): the rows that differ per instance, as this lane's column of a [ADP_LEN][G*batch] matrix
    static constexpr int AO_K = 0, AO_KT = AO_K + RU * S::NXP, AO_PT = AO_KT + RX * S::NUP, ADP_LEN = AO_PT + RX * S::NXP;
    static constexpr int BW = 2 * RX + 2 * RU;  // bounds per knot and role: xmin xmax umin umax
    static constexpr int DW = RX + RU;          // diag(Q)+rho, diag(R)+rho per role
};

// the (wave-uniform) knot index, hidden from loop strength reduction
__device__ __forceinline__ int knot_sgpr(int k) {
    k = __builtin_amdgcn_readfirstlane(k);  // free when the compiler already knows k to be uniform; makes "s" legal when not
    asm volatile("" : "+s"(k));
    return k;
}

// a wave-uniform pointer pinned to SGPRs: accesses become (SGPR base) + (32-bit VGPR offset)
template <class T>
__device__ __forceinline__ T *sgpr_ptr(T *p) {
    const unsigned long long a = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    p = reinterpret_cast<T *>(((unsigned long long)hi << 32) | lo);
    asm("" : "+s"(p));
    return p;
}

// uniform base + 32-bit byte offset of the lane: the (SGPR pair) + (VGPR) addressing mode of global_load/store.
// The explicit global address space keeps these from degrading to flat accesses once the pointer has been
// through sgpr_ptr's asm.
template <class T>
__device__ __forceinline__ auto lane_elem(T *uniform_base, unsigned byte_off) {
    using GC = std::conditional_t<std::is_const<T>::value, const char, char> __attribute__((address_space(1)));
    using GT = T __attribute__((address_space(1)));
    asm("" : "+v"(byte_off));  // keeps the 32->64-bit extension next to the access, where the addressing mode can absorb it
    return (GT *)((GC *)uniform_base + byte_off);
}

// R consecutive floats of one lane as the widest accesses (4-byte aligned; the hardware takes unaligned vectors)
typedef float sg_f2 __attribute__((ext_vector_type(2)));
typedef float sg_f4 __attribute__((ext_vector_type(4)));
typedef sg_f2 sg_f2u __attribute__((aligned(4)));
typedef sg_f4 sg_f4u __attribute__((aligned(4)));
template <int R, int O = 0, int RT_>
__device__ __forceinline__ void load_rows(const float __attribute__((address_space(1))) * p, float (&dst)[RT_]) {
    if constexpr (R >= 4) {
        const sg_f4 v = *(const sg_f4u __attribute__((address_space(1))) *)(p + O);
        dst[O] = v.x, dst[O + 1] = v.y, dst[O + 2] = v.z, dst[O + 3] = v.w;
        load_rows<R - 4, O + 4>(p, dst);
    } else if constexpr (R >= 2) {
        const sg_f2 v = *(const sg_f2u __attribute__((address_space(1))) *)(p + O);
        dst[O] = v.x, dst[O + 1] = v.y;
        load_rows<R - 2, O + 2>(p, dst);
    } else if constexpr (R == 1) {
        dst[O] = p[O];
    }
}
template <int R, int O = 0, int RT_>
__device__ __forceinline__ void store_rows(float __attribute__((address_space(1))) * p, const float (&src)[RT_]) {
    if constexpr (R >= 4) {
        sg_f4 v;
        v.x = src[O], v.y = src[O + 1], v.z = src[O + 2], v.w = src[O + 3];
        *(sg_f4u __attribute__((address_space(1))) *)(p + O) = v;
        store_rows<R - 4, O + 4>(p, src);
    } else if constexpr (R >= 2) {
        sg_f2 v;
        v.x = src[O], v.y = src[O + 1];
        *(sg_f2u __attribute__((address_space(1))) *)(p + O) = v;
        store_rows<R - 2, O + 2>(p, src);
    } else if constexpr (R == 1) {
        p[O] = src[O];
    }
}

// ... and R consecutive doubles (the fp64-state form): 16 bytes where rows pair up, 8 for the odd one (8-byte aligned)
typedef double sg_d2 __attribute__((ext_vector_type(2)));
typedef sg_d2 sg_d2u __attribute__((aligned(8)));
template <int R, int O = 0, int RT_>
__device__ __forceinline__ void load_rows(const double __attribute__((address_space(1))) * p, double (&dst)[RT_]) {
    if constexpr (R >= 2) {
        const sg_d2 v = *(const sg_d2u __attribute__((address_space(1))) *)(p + O);
        dst[O] = v.x, dst[O + 1] = v.y;
        load_rows<R - 2, O + 2>(p, dst);
    } else if constexpr (R == 1) {
        dst[O] = p[O];
    }
}
template <int R, int O = 0, int RT_>
__device__ __forceinline__ void store_rows(double __attribute__((address_space(1))) * p, const double (&src)[RT_]) {
    if constexpr (R >= 2) {
        sg_d2 v;
        v.x = src[O], v.y = src[O + 1];
        *(sg_d2u __attribute__((address_space(1))) *)(p + O) = v;
        store_rows<R - 2, O + 2>(p, src);
    } else if constexpr (R == 1) {
        p[O] = src[O];
    }
}

// Coefficient rows of one lane role in the LDS image (CoefLds's role-interleaved 16-byte chunks), any offset
template <class RT, int G>
struct CoefRole {
    static constexpr int VEC = 16 / (int)sizeof(RT);
    const RT *base;  // s_coef + q * VEC
    int off;
    __device__ __forceinline__ RT operator[](int i) const {
        const int j = off + i;
        return base[(j / VEC) * G * VEC + j % VEC];
    }
    __device__ __forceinline__ CoefRole operator+(int o) const { return CoefRole{base, off + o}; }
};

// One family per instance: element i of this lane's pack is column `lane` of row i of a [CP][G*batch] matrix.
template <class RT>
struct CoefCol {
    const RT *base;  // wave-uniform
    long stride;
    unsigned lane;  // byte offset of this lane's column
    __device__ __forceinline__ RT operator[](int i) const { return *lane_elem(sgpr_ptr(base + i * stride), lane); }
    __device__ __forceinline__ CoefCol operator+(int off) const { return CoefCol{base + off * stride, stride, lane}; }
};

template <int G, class T>
__device__ __forceinline__ T group_sum(T v) {
    if constexpr (G >= 2) v += dpp_quad<0xB1>(v);
    if constexpr (G == 4) v += dpp_quad<0x4E>(v);
    return v;
}

// max over the G lanes of a group, any arithmetic type (the adaptive-rho norms are kept in the kernel's RT)
template <int G, class T>
__device__ __forceinline__ T group_max_t(T v) {
    if constexpr (G >= 2) {
        const T o = __shfl_xor(v, 1, 64);
        v = o > v ? o : v;
    }
    if constexpr (G == 4) {
        const T o = __shfl_xor(v, 2, 64);
        v = o > v ? o : v;
    }
    return v;
}
// max over the group of a state-typed value: the quad kernel's DPP form, for either width
template <int G>
__device__ __forceinline__ float group_max_s(float m) { return group_max<G>(m); }
template <int G>
__device__ __forceinline__ double group_max_s(double m) {
    if constexpr (G >= 2) m = fmax(m, dpp_quad<0xB1>(m));
    if constexpr (G == 4) m = fmax(m, dpp_quad<0x4E>(m));
    return m;
}
template <class T>
__device__ __forceinline__ void upmax_abs(T &m, T v) {
    v = v < (T)0 ? -v : v;
    m = v > m ? v : m;
}

// cone c restricted to this lane's R local rows: bit m of head / axis set when local row m belongs to it
template <int G, int R, class T>
__device__ __forceinline__ void project_soc_group(T (&blk)[R], unsigned head, unsigned axis, T mu) {
    T a2 = (T)0, ax = (T)0;
#pragma unroll
    for (int m = 0; m < R; ++m) {
        if ((head >> m) & 1u) a2 = gfma(blk[m], blk[m], a2);
        if ((axis >> m) & 1u) ax = blk[m];
    }
    a2 = group_sum<G>(a2);
    ax = group_sum<G>(ax);  // exactly one lane contributes
    const T an = gsqrt(a2), u0 = ax * mu;
    const bool zero = an <= -u0, keep = !zero && an <= u0;
    const T sc = zero ? (T)0 : (keep ? (T)1 : (T)0.5 * ((T)1 + u0 / an));
    const T ax_new = zero ? (T)0 : (keep ? ax : sc * (an / mu));
#pragma unroll
    for (int m = 0; m < R; ++m) {
        if ((head >> m) & 1u) blk[m] *= sc;
        if ((axis >> m) & 1u) blk[m] = ax_new;
    }
}

// z <- projection onto {a_k . z <= b_k}, one row after the other; a lane holds its R local entries of each row
// (rows + k * stride), the dot product is summed over the group, so the branch is uniform within it
template <int G, int R, class T>
__device__ __forceinline__ void project_halfspaces_group(T (&z)[R], const float *rows, int stride, int m,
                                                         const float *b, const float *n2) {
    for (int k = 0; k < m; ++k) {
        const float *a = rows + k * stride;
        T dot = (T)0;
#pragma unroll
        for (int j = 0; j < R; ++j) dot = gfma((T)a[j], z[j], dot);
        dot = group_sum<G>(dot);
        if (dot > (T)b[k]) {
            const T t = (dot - (T)b[k]) / (T)n2[k];
#pragma unroll
            for (int j = 0; j < R; ++j) z[j] -= t * (T)a[j];
        }
    }
}

// a workspace array in the state's type: the fp32 array, or its place in the fp64 block (Ws64)
template <class ST>
__device__ __forceinline__ ST *ws_sel(float *f32, double *f64) {
    if constexpr (sizeof(ST) == 8) return f64;
    else return f32;
}

// wavefronts per SIMD the register allocation is held to, and knots of prefetch, per group size (MI355X, rocket
// N=50 with cones: 2..4 wavefronts and depth 1..3 are within 5 % of each other for G = 4; scripts/stream_tune.sh)
template <int G>
struct StreamTune {
    static constexpr int WAVES = G == 4 ? 3 : (G == 2 ? 2 : 1);
    // fp64 state: the knot buffers take twice the registers.  Two wavefronts (256 registers) hold every form but the
    // workspace-keeping ones with cones / linear rows compiled in, whose backward buffer carries w and g of every set:
    // (12, 4) spills 18 / 91 registers there, so those forms are held to one wavefront (the unified 512-register file)
    static constexpr int waves64(int ext, bool os) { return (ext > 0 && !os) ? 1 : 2; }
    // per-instance bounds (IB): four more arrays in every knot buffer.  (4, 1) and (6, 3) hold them at the plain forms' three
    // wavefronts without a spilled register.  (12, 4), whose plain twins already spill there (0 .. 14 registers box-only, 59 ..
    // 148 with cones / linear rows compiled in), spills 10 .. 34 and 82 .. 166: more than its twins in every form, so its IB
    // forms are held to two wavefronts (256 registers), as waves64 holds the fp64-state forms
    static constexpr int waves_ib(int nx) { return nx >= 12 ? 2 : WAVES; }
    static constexpr int DEPTH = G == 4 ? 1 : (G == 2 ? 2 : 3);
};
#ifndef TMPC_STREAM_DEPTH
#define TMPC_STREAM_DEPTH(G) StreamTune<G>::DEPTH
#endif
#ifndef TMPC_STREAM_WAVES
#define TMPC_STREAM_WAVES(G) StreamTune<G>::WAVES
#endif
#ifndef TMPC_STREAM_WAVES_IB
#define TMPC_STREAM_WAVES_IB(G, NX) StreamTune<G>::waves_ib(NX)
#endif
#ifndef TMPC_STREAM_WAVES64
#define TMPC_STREAM_WAVES64(G, EXT, OS) StreamTune<G>::waves64(EXT, OS)
#endif

}  // namespace tmpc
#endif  // TMPC_ADMM_STREAMG_HIP_H

#ifndef TMPC_STREAMG_BOTH
namespace tmpc {

// ADP: adaptive rho (admm.cpp:147-174 with rho_benchmark.cpp:44-213).  One family for the batch (its rows in LDS), but
// rho, Kinf and Pinf are every instance's own: the rows built from them (Kinf, Kinf^T, Pinf^T) are read from the lane's
// column of a scratch matrix that the kernel fills from the solver's adaptive state at entry and re-writes, together
// with that state, whenever it adapts — every 5th iteration, from norms gathered during that iteration's forward sweep.
//
// ST: the type of everything the iteration stores and streams — the scratch arrays, the knot buffers, slacks, duals, the
// residual maxima and the workspace kept between solves.  float: what precision 0 / 1 carry.  double (precision 2, with
// RT = double; one family, no adaptive rho): the reference's arithmetic end to end, as the generic kernel's fp64-state form
// computes it — same values, same order within a row; only the mat-vec sums are ordered by lane — with the workspace in the
// fp64 block P.ws64 (Ws64) and the tolerances compared in fp64.  Inputs, the LDS image and the outputs are the same fp32 arrays.
//
// MPC: the closed loop inside the launch (TINYMPC_HIP_STREAM_LOOP; workspace-keeping form, fixed rho, four lanes, fp64
// recurrences).  P.mpc_steps warm solves, each followed by the plant step the chain of launches takes between two of them
// (Solver::rollout_chain, plant_step_kernel): u0 = the fp32 control of knot 0, x+ = f + A x + B u0 in fp64 — f, then
// A's row by ascending column, then B's, one fma each — on the fp64 plant state in P.x0d, each lane its own rows, the other
// lanes' x_j and u_a by quad broadcasts; the next solve starts from (float)x+ with the workspace as the scratch block
// already holds it (what saving and reloading it would give: the kept arrays stay, the work arrays are zeroed), with the
// step's slice of P.xref_seq / P.uref_seq as its references.  The last solve leaves through the ordinary epilogue.
// The kernel below is compiled five times from this one text — the file includes itself at its end with TMPC_STREAMG_MPC = 1,
// then with TMPC_STREAMG_IB = 1, then with TMPC_STREAMG_IL = 1, then with TMPC_STREAMG_IC = 1 — as admm_streamg_kernel, as the
// loop form's admm_streamg_mpc_kernel<NX, NU, G, EXT, HET, ST>, as the per-instance-bounds form's admm_streamg_ib_kernel<NX, NU,
// G, EXT, HET, OS>, as the per-instance-rows form's admm_streamg_il_kernel<NX, NU, G, HET, OS> and as the per-instance-cones
// form's admm_streamg_ic_kernel<NX, NU, G, HET, OS>.  The preprocessor decides what
// `if constexpr` cannot wrap (the loop over steps around the iteration loop, the step's reference pointers), so that the plain
// kernel's text, name and code are what they were before the other forms existed (a further template parameter, even a
// defaulted one, renames every stream kernel).
//
// IB: box bounds PER INSTANCE (tinympc_set_instance_bounds; fp64 recurrences, fp32 state, fixed rho, four lanes).  A knot's
// bounds are not read from the LDS image but fetched with the knot's other arrays, D knots ahead, from P.ibx / P.ibu — fp32,
// [min | max][knot][instance][real row], the scratch block's layout — at knot strides that are 0 for bounds constant over the
// horizon (one line per instance, re-read from cache at every knot: no further HBM stream).  The clamp is the shared form's
// expression, so per-instance bounds that all equal a shared set give the plain kernel's results bit for bit.
//
// IL: linear rows PER INSTANCE (tinympc_set_instance_linear), the file's third self-inclusion: admm_streamg_il_kernel<NX, NU, G,
// HET, OS>, the IB form with EXT = 2 whose rows are the instance's own.  Rows are constant over the horizon, so they are read
// from HBM once, in the prologue — P.il_ax / P.il_au, [row][instance][real entry], a lane its RX / RU entries of a row in one
// load_rows at the IB form's instance offsets; P.il_bx .. P.il_n2u, [row][instance] — into a slice of LDS behind the bound
// image: [row][lane][entry] (a lane's entries RX / RU words apart from its neighbour's: no bank is hit twice), then per group
// b and |a|^2 of both sides.  Between knots they live there: not in registers ((12, 4) holds its EXT = 2 `ib` twin at two
// wavefronts with little to spare, and 8 + 8 rows are 64 more), not re-read through the cache (a dependent load in front of
// every row of a projection that takes them one after the other).  Only the rows present are held: 4 T (mlx RX + mlu RU) +
// 8 (T / G) (mlx + mlu) bytes a workgroup.  The projection is project_halfspaces_group, the shared form's, on other pointers.
//
// IC: the cone coefficient mu PER INSTANCE (tinympc_set_instance_cones), the file's fourth self-inclusion:
// admm_streamg_ic_kernel<NX, NU, G, HET, OS>, the IL form in full — bounds and rows per instance, the sides of rows and cones
// run-time flags — whose cones keep the batch's layout (P.Acx .. P.qcu, the membership masks) and take mu from P.ic_cx /
// P.ic_cu, fp32, [cone][instance].  A group reads its instance's ncx + ncu values once, where the IL slice is filled, into a
// group's part of that slice, behind b and |a|^2 ([state cones | input cones]: 4 (T / G) (ncx + ncu) bytes a workgroup) — not into
// registers, of which (12, 4) has none to spare.  At the two projection sites the value comes from there; +inf — the instance
// does not have the cone — skips the projection, a condition uniform over the group's lanes, so the quad sums inside
// project_soc_group stay whole.  The projection is project_soc_group, the shared form's, on another mu.
#if TMPC_STREAMG_IC
template <int NX, int NU, int G, bool HET, bool OS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TMPC_STREAM_WAVES_IB(G, NX)))) void admm_streamg_ic_kernel(const AdmmParams P) {
    using RT = double;
    using ST = float;
    constexpr int EXT = 2;
    constexpr bool ADP = false, MPC = false, IB = true, IL = true, IC = true;
#elif TMPC_STREAMG_IL
template <int NX, int NU, int G, bool HET, bool OS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TMPC_STREAM_WAVES_IB(G, NX)))) void admm_streamg_il_kernel(const AdmmParams P) {
    using RT = double;
    using ST = float;
    constexpr int EXT = 2;
    constexpr bool ADP = false, MPC = false, IB = true, IL = true, IC = false;
#elif TMPC_STREAMG_IB
template <int NX, int NU, int G, int EXT, bool HET, bool OS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TMPC_STREAM_WAVES_IB(G, NX)))) void admm_streamg_ib_kernel(const AdmmParams P) {
    using RT = double;
    using ST = float;
    constexpr bool ADP = false, MPC = false, IB = true, IL = false, IC = false;
#elif !TMPC_STREAMG_MPC
template <int NX, int NU, int G, class RT, int EXT, bool HET, bool OS, bool ADP = false, class ST = float>
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(sizeof(ST) == 8 ? TMPC_STREAM_WAVES64(G, EXT, OS) : TMPC_STREAM_WAVES(G)))) void admm_streamg_kernel(const AdmmParams P) {
    constexpr bool MPC = false, IB = false, IL = false, IC = false;
#else
template <int NX, int NU, int G, int EXT, bool HET, class ST = float>
__global__ __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(sizeof(ST) == 8 ? TMPC_STREAM_WAVES64(G, EXT, false) : TMPC_STREAM_WAVES(G)))) void admm_streamg_mpc_kernel(const AdmmParams P) {
    using RT = double;
    constexpr bool OS = false, ADP = false, MPC = true, IB = false, IL = false, IC = false;
#endif
    static_assert(!IB || (!ADP && sizeof(ST) == 4 && sizeof(RT) == 8 && G == 4), "per-instance bounds: fixed rho, fp32 state, fp64 recurrences, four lanes");
    static_assert(!ADP || (!HET && EXT == 0), "adaptive rho: one family, box sets only");
    static_assert(sizeof(ST) == 4 || (sizeof(RT) == 8 && !HET && !ADP), "fp64 state: fp64 recurrences, one family, fixed rho");
    static_assert(!MPC || (!OS && !ADP && G == 4 && sizeof(RT) == 8), "in-kernel closed loop: workspace kept, fixed rho, four lanes, fp64 recurrences");
    constexpr bool WIDE = sizeof(ST) == 8;
    using PK = StreamPackG<NX, NU, G>;
    using S = typename PK::S;
    constexpr int T = 256, D = TMPC_STREAM_DEPTH(G), RX = S::RX, RU = S::RU, NXP = S::NXP, NUP = S::NUP, NXL = S::NXL,
                  NUL = S::NUL;
    constexpr bool XFULL = NX % RX == 0, UFULL = NU % RU == 0;  // every owning lane owns RX / RU real rows
    constexpr bool ALLX = XFULL && NXL == G, ALLU = UFULL && NUL == G;  // ... and every lane is an owning lane
    extern __shared__ __align__(16) unsigned char s_rawg[];
    RT *s_coef = reinterpret_cast<RT *>(s_rawg);
    float *s_bnd = reinterpret_cast<float *>(s_rawg + sizeof(RT) * G * PK::CP);
    __shared__ uint4 s_cmask[8 * G];
    // linear inequalities (EXT == 2): per row and lane role the local entries, then right-hand sides and |a|^2
    __shared__ float s_lax[EXT == 2 && !IL ? LIN_MAX_ROWS * G * RX : 1], s_lau[EXT == 2 && !IL ? LIN_MAX_ROWS * G * RU : 1],
        s_lb[IL ? 1 : 4 * LIN_MAX_ROWS];

    const int N = P.N;
    const int tid = threadIdx.x;
    const RT *gcoef = reinterpret_cast<const RT *>(P.coef);
    if constexpr (!HET)  // role-major in HBM -> role-interleaved 16-byte chunks in LDS
        for (int i = tid; i < G * PK::CP; i += T) s_coef[CoefLds<RT, G>::slot(i % PK::CP, i / PK::CP)] = gcoef[i];
    const int bnd_len = N * G * PK::BW + G * PK::DW;
    for (int i = tid; i < bnd_len; i += T) s_bnd[i] = P.bounds[i];
    __syncthreads();

    const int q = tid % G;
    const long B = P.batch, BG = G * B;
    const long slot = (long)blockIdx.x * (T / G) + tid / G;
    const bool active = slot < B;
    const long bb = active ? slot : 0;                      // dense index: scratch columns (and families, HET)
    const long b = (active && P.idx) ? P.idx[slot] : slot;  // instance this lane group works on
    const long L = G * bb + q;  // this lane's column in the per-instance coefficient matrix (HET)
    const long EX = (long)NX * N, EU = (long)NU * (N - 1);
    const float *lb = s_bnd + q * PK::BW;

    float cQD[RX], cRD[RU];
    ST rho = WIDE ? (ST)P.rho_family : (ST)P.rho;
    if constexpr (HET) {  // per instance: het_aux = [Qd (nx) | Rd (nu) | rho][batch]
#pragma unroll
        for (int m = 0; m < RX; ++m) cQD[m] = (q * RX + m < NX) ? P.het_aux[(long)(q * RX + m) * B + bb] : 0.f;
#pragma unroll
        for (int m = 0; m < RU; ++m) cRD[m] = (q * RU + m < NU) ? P.het_aux[(long)(NX + q * RU + m) * B + bb] : 0.f;
        rho = P.het_aux[(long)(NX + NU) * B + bb];
    } else {
        const float *ld = s_bnd + N * G * PK::BW + q * PK::DW;
#pragma unroll
        for (int m = 0; m < RX; ++m) cQD[m] = ld[m];
#pragma unroll
        for (int m = 0; m < RU; ++m) cRD[m] = ld[RX + m];
    }
    using CPtr = std::conditional_t<HET, CoefCol<RT>, CoefRole<RT, G>>;
    CPtr cbase;
    if constexpr (HET)
        cbase = CoefCol<RT>{gcoef, BG, (unsigned)(L * sizeof(RT))};
    else
        cbase = CoefRole<RT, G>{s_coef + q * CoefRole<RT, G>::VEC, 0};
    const CPtr cA = cbase + S::O_A, cB = cbase + S::O_B, cAT = cbase + S::O_AT, cBT = cbase + S::O_BT, cQI = cbase + S::O_QI,
               cF = cbase + PK::O_F, cAPF = cbase + PK::O_APF, cBPF = cbase + PK::O_BPF, cATT = cbase + PK::O_ATT;
    (void)cATT;
    using KPtr = std::conditional_t<ADP, CoefCol<RT>, CPtr>;   // the rows made of Kinf / Pinf
    KPtr cK, cKT, cPT;
    RT *const adp_cols = ADP ? reinterpret_cast<RT *>(P.adp_cols) : nullptr;
    double rho_d = (double)P.rho;                           // ADP: this instance's rho as the adaptive state holds it
    if constexpr (ADP) {
        const CoefCol<RT> col{adp_cols, BG, (unsigned)(L * sizeof(RT))};
        cK = col + PK::AO_K, cKT = col + PK::AO_KT, cPT = col + PK::AO_PT;
        // fill the column from the solver's adaptive state [1 + nu nx + nx nx][batch] (rho | Kinf | Pinf, column-major)
        const long AB = P.adapt_stride;
        const double *ad = P.adapt + b;
        if (active) {
            rho_d = ad[0];
            rho = (ST)(float)rho_d;
            RT *mine = adp_cols + L;
#pragma unroll
            for (int m = 0; m < RU; ++m)
                for (int j = 0; j < NXP; ++j) {
                    const int a = q * RU + m;
                    mine[(long)(PK::AO_K + m * NXP + j) * BG] = (a < NU && j < NX) ? (RT)ad[(long)(1 + a + j * NU) * AB] : (RT)0;
                }
#pragma unroll
            for (int m = 0; m < RX; ++m) {
                const int r = q * RX + m;
                for (int a = 0; a < NUP; ++a)
                    mine[(long)(PK::AO_KT + m * NUP + a) * BG] = (r < NX && a < NU) ? (RT)ad[(long)(1 + a + r * NU) * AB] : (RT)0;
                for (int j = 0; j < NXP; ++j)
                    mine[(long)(PK::AO_PT + m * NXP + j) * BG] =
                        (r < NX && j < NX) ? (RT)ad[(long)(1 + NU * NX + j + r * NX) * AB] : (RT)0;   // Pinf^T[r][j] = Pinf[j][r]
            }
        }
    } else {
        cK = cbase + S::O_K, cKT = cbase + S::O_KT, cPT = cbase + S::O_PT;
    }

    // cone membership of each role's local rows, as bit masks in LDS: [cone][role]{x heads, x axis, u heads, u axis}
    const int ncx = EXT ? P.ncx : 0, ncu = EXT ? P.ncu : 0;
    if constexpr (EXT) {
        if (tid < 8 * G) {
            const int c = tid / G, r = tid % G;
            unsigned hx = 0u, ax = 0u, hu = 0u, au = 0u;
            if (c < ncx)
                for (int m = 0; m < RX; ++m) {
                    const int row = r * RX + m;
                    if (row >= P.Acx[c] && row < P.Acx[c] + P.qcx[c] - 1) hx |= 1u << m;
                    if (row == P.Acx[c] + P.qcx[c] - 1) ax |= 1u << m;
                }
            if (c < ncu)
                for (int m = 0; m < RU; ++m) {
                    const int row = r * RU + m;
                    if (row >= P.Acu[c] && row < P.Acu[c] + P.qcu[c] - 1) hu |= 1u << m;
                    if (row == P.Acu[c] + P.qcu[c] - 1) au |= 1u << m;
                }
            s_cmask[tid] = make_uint4(hx, ax, hu, au);
        }
        __syncthreads();
    }
    const uint4 *cm = s_cmask + q;
    const bool soc_x = ncx > 0, soc_u = ncu > 0;
    const int mlx = EXT == 2 ? P.mlx : 0, mlu = EXT == 2 ? P.mlu : 0;
    if constexpr (EXT == 2 && !IL) {
        const float *gAx = P.lin, *gbx = gAx + mlx * NX, *gn2x = gbx + mlx;
        const float *gAu = gn2x + mlx, *gbu = gAu + mlu * NU, *gn2u = gbu + mlu;
        for (int i = tid; i < LIN_MAX_ROWS * G * RX; i += T) {
            const int k = i / (G * RX), row = i % (G * RX);  // (role, local row) flattened = padded row index
            s_lax[i] = (k < mlx && row < NX) ? gAx[k * NX + row] : 0.f;
        }
        for (int i = tid; i < LIN_MAX_ROWS * G * RU; i += T) {
            const int k = i / (G * RU), row = i % (G * RU);
            s_lau[i] = (k < mlu && row < NU) ? gAu[k * NU + row] : 0.f;
        }
        if (tid < LIN_MAX_ROWS) {
            s_lb[tid] = tid < mlx ? gbx[tid] : 0.f;
            s_lb[LIN_MAX_ROWS + tid] = tid < mlx ? gn2x[tid] : 1.f;
            s_lb[2 * LIN_MAX_ROWS + tid] = tid < mlu ? gbu[tid] : 0.f;
            s_lb[3 * LIN_MAX_ROWS + tid] = tid < mlu ? gn2u[tid] : 1.f;
        }
        __syncthreads();
    }
    const bool lin_x = mlx > 0, lin_u = mlu > 0;
    // the rows this lane projects onto: its RX / RU entries of row k at lax / lau + k * LSX / LSU, right-hand sides and |a|^2 by
    // row at lbx, ln2x, lbu, ln2u — the workgroup's shared image, or (IL) the lane's and its group's places in the LDS slice
    // behind the bound image (filled below, once the instance offsets exist)
    constexpr int LSX = IL ? T * RX : G * RX, LSU = IL ? T * RU : G * RU;
    float *const s_il = IL ? s_bnd + bnd_len : nullptr;
    float *const s_ilb = IL ? s_il + (long)T * (mlx * RX + mlu * RU) + (tid / G) * (2 * (mlx + mlu) + (IC ? ncx + ncu : 0)) : nullptr;
    const float *lax = IL ? s_il + tid * RX : s_lax + q * RX, *lau = IL ? s_il + T * mlx * RX + tid * RU : s_lau + q * RU;
    const float *lbx = IL ? s_ilb : s_lb, *ln2x = IL ? s_ilb + mlx : s_lb + LIN_MAX_ROWS;
    const float *lbu = IL ? s_ilb + 2 * mlx : s_lb + 2 * LIN_MAX_ROWS, *ln2u = IL ? s_ilb + 2 * mlx + mlu : s_lb + 3 * LIN_MAX_ROWS;
    // (IC) the group's cone coefficients, state cones then input cones, behind its b and |a|^2.  In the sweeps the IC form reaches
    // them, and the four arrays in front of them, from s_ilb by offsets made opaque per use (knot_sgpr): pointers of their own are
    // loop invariants, hoisted out of the iteration loop into a register each, and the (one family per instance, workspace kept)
    // kernels of (6, 3) and (12, 4) have none to spare — with them they spill one and two registers, without them none
    float *const s_ic = IC ? s_ilb + 2 * (mlx + mlu) : nullptr;

    // Scratch: [array][knot][instance][real row].  Addresses are (uniform 64-bit base in SGPRs) + (32-bit byte
    // offset of the lane); the knot index is made opaque per knot (knot_sgpr) so that no per-array 64-bit
    // pointers are carried through the sweeps in VGPRs.  Lanes / rows beyond nx, nu read a clamped (valid)
    // address, the consumer discards the value (mkx / mku), and they do not store.
    const long BNX = B * NX, BNU = B * NU;
    const long SXN = BNX * N, SUN = BNU * (N - 1);
    const bool xl = q < NXL, ul = q < NUL;
    unsigned okx = 0u, oku = 0u, lxo[RX], luo[RU];
#pragma unroll
    for (int m = 0; m < RX; ++m) {
        const int row = q * RX + m;
        if (row < NX) okx |= 1u << m;
        const int rc = XFULL ? (q < NXL ? q : NXL - 1) * RX : (row < NX ? row : NX - 1);
        lxo[m] = (unsigned)((bb * NX + rc) * (long)sizeof(ST));
    }
#pragma unroll
    for (int m = 0; m < RU; ++m) {
        const int row = q * RU + m;
        if (row < NU) oku |= 1u << m;
        const int rc = UFULL ? (q < NUL ? q : NUL - 1) * RU : (row < NU ? row : NU - 1);
        luo[m] = (unsigned)((bb * NU + rc) * (long)sizeof(ST));
    }
    // IB: the bound arrays [min | max][knot][instance][real row] are addressed by the INSTANCE b, not by the dense slot bb of
    // the scratch columns (the two differ under compaction): a second set of lane offsets.  Inactive lanes and lanes without
    // a row read a clamped, valid address; the consumer discards the value (bxlo .. buhi below).
    unsigned lxi[IB ? RX : 1], lui[IB ? RU : 1];
    if constexpr (IB) {
        const long bi = active ? b : 0;
#pragma unroll
        for (int m = 0; m < RX; ++m) {
            const int row = q * RX + m;
            const int rc = XFULL ? (q < NXL ? q : NXL - 1) * RX : (row < NX ? row : NX - 1);
            lxi[m] = (unsigned)((bi * NX + rc) * (long)sizeof(float));
        }
#pragma unroll
        for (int m = 0; m < RU; ++m) {
            const int row = q * RU + m;
            const int rc = UFULL ? (q < NUL ? q : NUL - 1) * RU : (row < NU ? row : NU - 1);
            lui[m] = (unsigned)((bi * NU + rc) * (long)sizeof(float));
        }
    }
    const bool ibx_on = IB && (P.ib_on & IB_STATE) != 0, ibu_on = IB && (P.ib_on & IB_INPUT) != 0;   // wave-uniform: the side is read
    ST *const Sg = reinterpret_cast<ST *>(P.scratch), *const Sw = Sg + SXN, *const Sv = Sw + SXN;
    ST *const Sy = Sv + SXN, *const Szw = Sy + SUN, *const Sz = Szw + SUN, *const Sd = Sz + SUN;
    ST *const Sgc = Sd + SUN, *const Swc = Sgc + SXN, *const Svc = Swc + SXN;
    ST *const Syc = Svc + SXN, *const Szwc = Syc + SUN, *const Szc = Szwc + SUN;
    ST *const Sgl = Szc + SUN, *const Swl = Sgl + SXN, *const Svl = Swl + SXN;
    ST *const Syl = Svl + SXN, *const Szwl = Syl + SUN, *const Szl = Szwl + SUN;
    ST *const Ss = Sv, *const Ssu = Sz;  // OS: the fused arrays live where v and z would
#define SXP(arr, k, m) lane_elem(sgpr_ptr(arr + ((long)(k)*BNX + (XFULL ? (m) : 0))), lxo[XFULL ? 0 : (m)])
#define SUP(arr, k, m) lane_elem(sgpr_ptr(arr + ((long)(k)*BNU + (UFULL ? (m) : 0))), luo[UFULL ? 0 : (m)])
#define OKX(m) (ALLX || (XFULL ? xl : (((okx >> (m)) & 1u) != 0u)))
#define OKU(m) (ALLU || (UFULL ? ul : (((oku >> (m)) & 1u) != 0u)))
    auto ldx = [&](ST *arr, int k, ST (&dst)[RX]) {
        if constexpr (XFULL) {
            load_rows<RX>(SXP(arr, k, 0), dst);
        } else {
#pragma unroll
            for (int m = 0; m < RX; ++m) dst[m] = *SXP(arr, k, m);
        }
    };
    auto ldu = [&](ST *arr, int k, ST (&dst)[RU]) {
        if constexpr (UFULL) {
            load_rows<RU>(SUP(arr, k, 0), dst);
        } else {
#pragma unroll
            for (int m = 0; m < RU; ++m) dst[m] = *SUP(arr, k, m);
        }
    };
    // stores of one array's rows; the caller has already excluded lanes that own no row (XFULL / UFULL shapes)
    auto stx = [&](ST *arr, int k, const ST (&src)[RX]) {
        if constexpr (XFULL) {
            store_rows<RX>(SXP(arr, k, 0), src);
        } else {
#pragma unroll
            for (int m = 0; m < RX; ++m)
                if (OKX(m)) *SXP(arr, k, m) = src[m];
        }
    };
    auto stu = [&](ST *arr, int k, const ST (&src)[RU]) {
        if constexpr (UFULL) {
            store_rows<RU>(SUP(arr, k, 0), src);
        } else {
#pragma unroll
            for (int m = 0; m < RU; ++m)
                if (OKU(m)) *SUP(arr, k, m) = src[m];
        }
    };
    // IB: one half (h = 0 min, 1 max) of a knot's bounds of this lane's rows
    auto ldbx = [&](int h, int k, float (&dst)[IB ? RX : 1]) {
        if constexpr (IB) {
            const float *base = P.ibx + (h ? P.ib_hx : 0) + (long)k * P.ib_kx;
            if constexpr (XFULL) {
                load_rows<RX>(lane_elem(sgpr_ptr(base), lxi[0]), dst);
            } else {
#pragma unroll
                for (int m = 0; m < RX; ++m) dst[m] = *lane_elem(sgpr_ptr(base), lxi[m]);
            }
        }
    };
    auto ldbu = [&](int h, int k, float (&dst)[IB ? RU : 1]) {
        if constexpr (IB) {
            const float *base = P.ibu + (h ? P.ib_hu : 0) + (long)k * P.ib_ku;
            if constexpr (UFULL) {
                load_rows<RU>(lane_elem(sgpr_ptr(base), lui[0]), dst);
            } else {
#pragma unroll
                for (int m = 0; m < RU; ++m) dst[m] = *lane_elem(sgpr_ptr(base), lui[m]);
            }
        }
    };
    if constexpr (IL) {   // this instance's rows, HBM -> the LDS slice; entries of rows the lane does not own are 0, as the shared image has them
        const long bi = active ? b : 0;
        for (int k = 0; k < mlx; ++k) {
            float a[RX];
            const float *base = P.il_ax + (long)k * P.il_rx;
            if constexpr (XFULL) {
                load_rows<RX>(lane_elem(sgpr_ptr(base), lxi[0]), a);
            } else {
#pragma unroll
                for (int m = 0; m < RX; ++m) a[m] = *lane_elem(sgpr_ptr(base), lxi[m]);
            }
#pragma unroll
            for (int m = 0; m < RX; ++m) s_il[((long)k * T + tid) * RX + m] = OKX(m) ? a[m] : 0.f;
            if (q == 0) s_ilb[k] = P.il_bx[(long)k * P.il_rb + bi], s_ilb[mlx + k] = P.il_n2x[(long)k * P.il_rb + bi];
        }
        for (int k = 0; k < mlu; ++k) {
            float a[RU];
            const float *base = P.il_au + (long)k * P.il_ru;
            if constexpr (UFULL) {
                load_rows<RU>(lane_elem(sgpr_ptr(base), lui[0]), a);
            } else {
#pragma unroll
                for (int m = 0; m < RU; ++m) a[m] = *lane_elem(sgpr_ptr(base), lui[m]);
            }
#pragma unroll
            for (int m = 0; m < RU; ++m) s_il[(long)T * mlx * RX + ((long)k * T + tid) * RU + m] = OKU(m) ? a[m] : 0.f;
            if (q == 0) s_ilb[2 * mlx + k] = P.il_bu[(long)k * P.il_rb + bi], s_ilb[2 * mlx + mlu + k] = P.il_n2u[(long)k * P.il_rb + bi];
        }
        if constexpr (IC) {   // ... and its cone coefficients, one lane of the group each side
            if (q == 0)
                for (int c = 0; c < ncx; ++c) s_ic[c] = P.ic_cx[(long)c * P.ic_rc + bi];
            if (q == 1)
                for (int c = 0; c < ncu; ++c) s_ic[ncx + c] = P.ic_cu[(long)c * P.ic_rc + bi];
        }
        __syncthreads();
    }
    auto mkx = [&](ST v, int m) __attribute__((always_inline)) { return OKX(m) ? v : (ST)0; };
    auto mku = [&](ST v, int m) __attribute__((always_inline)) { return OKU(m) ? v : (ST)0; };
    const bool x_owner = ALLX || !XFULL || xl, u_owner = ALLU || !UFULL || ul;
    // One-shot solve without a finite state bound: vnew = x + g is never clamped, so the state dual stays at its
    // cold-start value, zero — it is neither streamed nor computed (bit-identical results).  Plain kernels only: with
    // the extensions compiled in, the extra run-time case costs config 4 (which has finite state bounds) 3 %.
    const bool nog = EXT == 0 && OS && !P.xb_active;

    RT x0[RX];
#pragma unroll
    for (int m = 0; m < RX; ++m) x0[m] = (active && q * RX + m < NX) ? (RT)P.x0[b * NX + q * RX + m] : (RT)0;
    const bool warm = active && !P.cold_start;
    // the workspace kept between solves: the fp32 arrays, or (fp64 state) the fp64 block, both instance-major
    const Ws64 w64(P.ws64, B, EX, EU);
#define WSA(f) ws_sel<ST>(P.f, w64.f)
    if (active) {
        for (int k = 0; k < N; ++k)
#pragma unroll
            for (int m = 0; m < RX; ++m) {
                const int row = q * RX + m;
                if (row >= NX) continue;
                *SXP(Sg, k, m) = warm ? WSA(sg)[b * EX + k * NX + row] : 0.f;
                *SXP(Sw, k, m) = 0.f;
                if constexpr (!OS) *SXP(Sv, k, m) = warm ? WSA(sv)[b * EX + k * NX + row] : 0.f;
                if (soc_x) {
                    *SXP(Sgc, k, m) = warm ? WSA(sgc)[b * EX + k * NX + row] : 0.f;
                    *SXP(Swc, k, m) = 0.f;
                    if constexpr (!OS) *SXP(Svc, k, m) = warm ? WSA(svc)[b * EX + k * NX + row] : 0.f;
                }
                if (lin_x) {
                    *SXP(Sgl, k, m) = warm ? WSA(sgl)[b * EX + k * NX + row] : 0.f;
                    *SXP(Swl, k, m) = 0.f;
                    if constexpr (!OS) *SXP(Svl, k, m) = warm ? WSA(svl)[b * EX + k * NX + row] : 0.f;
                }
            }
        for (int k = 0; k < N - 1; ++k)
#pragma unroll
            for (int m = 0; m < RU; ++m) {
                const int row = q * RU + m;
                if (row >= NU) continue;
                *SUP(Sy, k, m) = warm ? WSA(sy)[b * EU + k * NU + row] : 0.f;
                *SUP(Sd, k, m) = warm ? WSA(sd)[b * EU + k * NU + row] : 0.f;
                *SUP(Szw, k, m) = 0.f;
                if constexpr (!OS) *SUP(Sz, k, m) = warm ? WSA(sz)[b * EU + k * NU + row] : 0.f;
                if (soc_u) {
                    *SUP(Syc, k, m) = warm ? WSA(syc)[b * EU + k * NU + row] : 0.f;
                    *SUP(Szwc, k, m) = 0.f;
                    if constexpr (!OS) *SUP(Szc, k, m) = warm ? WSA(szc)[b * EU + k * NU + row] : 0.f;
                }
                if (lin_u) {
                    *SUP(Syl, k, m) = warm ? WSA(syl)[b * EU + k * NU + row] : 0.f;
                    *SUP(Szwl, k, m) = 0.f;
                    if constexpr (!OS) *SUP(Szl, k, m) = warm ? WSA(szl)[b * EU + k * NU + row] : 0.f;
                }
            }
    }
#if TMPC_STREAMG_MPC
    const float *xrefp = P.xref, *urefp = P.uref;   // the step's slice of the reference sequence
#define TMPC_XREF xrefp
#define TMPC_UREF urefp
#else
#define TMPC_XREF P.xref
#define TMPC_UREF P.uref
#endif
    auto ref_x = [&](int k, int m) __attribute__((always_inline)) -> float {
        const int row = q * RX + m;
        if (row >= NX || P.ref_mode == REF_ZERO) return 0.f;
        return P.ref_mode == REF_SHARED ? TMPC_XREF[k * NX + row] : TMPC_XREF[b * EX + k * NX + row];
    };
    auto ref_u = [&](int k, int m) __attribute__((always_inline)) -> float {
        const int row = q * RU + m;
        if (row >= NU || P.ref_mode == REF_ZERO) return 0.f;
        return P.ref_mode == REF_SHARED ? TMPC_UREF[k * NU + row] : TMPC_UREF[b * EU + k * NU + row];
    };

    int it = 0, conv = 0;
    float res0 = 0.f, res1 = 0.f, res2 = 0.f, res3 = 0.f;
    if (warm) {
        res0 = P.res[b * 4 + 0];
        res1 = P.res[b * 4 + 1];
        res2 = P.res[b * 4 + 2];
        res3 = P.res[b * 4 + 3];
    }
    const int ct = P.check_termination;
    const bool can_converge = WIDE ? (P.abs_pri_tol64 > 0.0 && P.abs_dua_tol64 > 0.0) : (P.abs_pri_tol > 0.f && P.abs_dua_tol > 0.f);
    const int last_check_it = ct > 0 ? (P.max_iter / ct) * ct : 0;
    // where the previous iteration's vnew / znew are found (dual residual, admm.cpp:93-96)
    ST *const Svold = OS ? Sw : Sv, *const Svcold = OS ? Swc : Svc, *const Szold = OS ? Szw : Sz,
                 *const Szcold = OS ? Szwc : Szc, *const Svlold = OS ? Swl : Svl, *const Szlold = OS ? Szwl : Szl;

    // what one knot of the forward / backward sweep reads from the scratch block, D knots ahead of its use
    struct FwdBuf {
        ST g[RX], v[RX], gc[RX], vc[RX], gl[RX], vl[RX], d[RU], y[RU], z[RU], yc[RU], zc[RU], yl[RU], zl[RU];
        float xlo[IB ? RX : 1], xhi[IB ? RX : 1], ulo[IB ? RU : 1], uhi[IB ? RU : 1];   // IB: the instance's bounds at the knot
    };
    struct BwdBuf {  // OS: the fused arrays in w / zw; else all of them
        ST w[RX], g[RX], wc[RX], gc[RX], wl[RX], gl[RX], zw[RU], y[RU], zwc[RU], yc[RU], zwl[RU], yl[RU];
    };

#if TMPC_STREAMG_MPC
    const int nsteps = P.mpc_steps;
    for (int step = 0; step < nsteps; ++step) {   // (the iteration loop below keeps its indentation)
#endif
    for (int i = 0; i < P.max_iter; ++i) {
        if (active && !conv) {
            const bool check = ct > 0 && (i + 1) % ct == 0;  // lanes still iterating have it == i: wave-uniform
            const bool need_res = check && (can_converge || i + 1 == last_check_it);
            // OS: vnew / znew themselves are only read back as "previous" values by a residual check and as the
            // solution, so they are stored when this iteration may be a lane's last or the next one checks
            const bool check_next = ct > 0 && (i + 2) % ct == 0;
            const bool keep_w = !OS || need_res || i + 1 == P.max_iter ||
                                (check_next && (can_converge || i + 2 == last_check_it));
            // ================= fused forward sweep (admm.cpp:25-69 + :93-96) =================
            RT x[RX];
#pragma unroll
            for (int m = 0; m < RX; ++m) x[m] = x0[m];
            ST pri_x = (ST)0, dua_x = (ST)0, pri_u = (ST)0, dua_u = (ST)0;
            // adaptive rho: the iterations that adapt (admm.cpp:147) gather the norms of rho_benchmark.cpp:44-213 on the
            // way — constraint rows [u_k; A x_k + B u_k (+ f) - x_{k+1}] against [znew_k; vnew_{k+1}], cost rows
            // P x + q + A'y with P = blkdiag(Q~, R~, .., Pinf), q = [Q~ x; R~ u] (zero reference), y = [y_k; g_{k+1}] —
            // each knot contributing the rows of knot k - 1 that needed its new dual g_k.
            const bool adapt_now = ADP && i > 0 && i % 5 == 0;
            const ST rho_lin = rho;   // the linear cost of this iteration is formed before the adaptation (admm.cpp:139 vs :147)
            RT a_pri = 0, a_axm = 0, a_zm = 0, a_dres = 0, a_pxm = 0, a_atym = 0, a_qm = 0;
            RT a_xp[RX];
            float a_gp[RX], a_up[RU], a_yp[RU];              // knot k - 1: x, new g, u, new y
#pragma unroll
            for (int m = 0; m < RX; ++m) a_xp[m] = (RT)0, a_gp[m] = 0.f;
#pragma unroll
            for (int m = 0; m < RU; ++m) a_up[m] = a_yp[m] = 0.f;
            FwdBuf fb[D];
#pragma unroll
            for (int j = 0; j < D; ++j) {
#pragma unroll
                for (int m = 0; m < RX; ++m)
                    fb[j].g[m] = fb[j].v[m] = fb[j].gc[m] = fb[j].vc[m] = fb[j].gl[m] = fb[j].vl[m] = (ST)0;
#pragma unroll
                for (int m = 0; m < RU; ++m)
                    fb[j].d[m] = fb[j].y[m] = fb[j].z[m] = fb[j].yc[m] = fb[j].zc[m] = fb[j].yl[m] = fb[j].zl[m] = (ST)0;
                if constexpr (IB) {   // a side the settings switch off is never read: it clamps against -+inf
#pragma unroll
                    for (int m = 0; m < RX; ++m) fb[j].xlo[m] = -__builtin_inff(), fb[j].xhi[m] = __builtin_inff();
#pragma unroll
                    for (int m = 0; m < RU; ++m) fb[j].ulo[m] = -__builtin_inff(), fb[j].uhi[m] = __builtin_inff();
                }
            }
            auto fetch_x = [&](int k_, FwdBuf &f) __attribute__((always_inline)) {
                const int k = knot_sgpr(k_);
                if (!nog) ldx(Sg, k, f.g);
                if (need_res) ldx(Svold, k, f.v);
                if (soc_x) {
                    ldx(Sgc, k, f.gc);
                    if (need_res) ldx(Svcold, k, f.vc);
                }
                if (lin_x) {
                    ldx(Sgl, k, f.gl);
                    if (need_res) ldx(Svlold, k, f.vl);
                }
                if constexpr (IB)
                    if (ibx_on) {
                        ldbx(0, k, f.xlo);
                        ldbx(1, k, f.xhi);
                    }
            };
            auto fetch_u = [&](int k_, FwdBuf &f) __attribute__((always_inline)) {
                const int k = knot_sgpr(k_);
                ldu(Sd, k, f.d);
                ldu(Sy, k, f.y);
                if (need_res) ldu(Szold, k, f.z);
                if (soc_u) {
                    ldu(Syc, k, f.yc);
                    if (need_res) ldu(Szcold, k, f.zc);
                }
                if (lin_u) {
                    ldu(Syl, k, f.yl);
                    if (need_res) ldu(Szlold, k, f.zl);
                }
                if constexpr (IB)
                    if (ibu_on) {
                        ldbu(0, k, f.ulo);
                        ldbu(1, k, f.uhi);
                    }
            };
            auto fwd_knot = [&](int k_, FwdBuf &f) __attribute__((always_inline)) {
                asm volatile("" ::: "memory");  // keep coefficient / bound loads per knot (no hoisting into registers)
                const int k = knot_sgpr(k_);
                const bool pf = k + D < N;  // this knot's buffer is refilled for knot k + D once consumed
                const float *bk = lb + k * G * PK::BW;
                ST xf[RX], vn[RX], gn[RX], wc[RX], gcn[RX], wl[RX], gln[RX], sx[RX];
                // the knot's bounds of this lane's rows: the shared image's, or (IB) the instance's own as fetched with the
                // knot's other arrays — a row the lane does not own is unbounded, as the shared image has it
                auto bxlo = [&](int m) __attribute__((always_inline)) -> ST {
                    if constexpr (IB) return OKX(m) ? (ST)f.xlo[m] : (ST)-__builtin_inff();
                    else return (ST)bk[m];
                };
                auto bxhi = [&](int m) __attribute__((always_inline)) -> ST {
                    if constexpr (IB) return OKX(m) ? (ST)f.xhi[m] : (ST)__builtin_inff();
                    else return (ST)bk[RX + m];
                };
                auto bulo = [&](int m) __attribute__((always_inline)) -> ST {
                    if constexpr (IB) return OKU(m) ? (ST)f.ulo[m] : (ST)-__builtin_inff();
                    else return (ST)bk[2 * RX + m];
                };
                auto buhi = [&](int m) __attribute__((always_inline)) -> ST {
                    if constexpr (IB) return OKU(m) ? (ST)f.uhi[m] : (ST)__builtin_inff();
                    else return (ST)bk[2 * RX + RU + m];
                };
#pragma unroll
                for (int m = 0; m < RX; ++m) {
                    const ST g_c = nog ? (ST)0 : mkx(f.g[m], m), v_c = mkx(f.v[m], m);
                    xf[m] = (ST)x[m];
                    vn[m] = gmin(bxhi(m), gmax(bxlo(m), xf[m] + g_c));
                    gn[m] = (g_c + xf[m]) - vn[m];
                    gupmax(pri_x, xf[m] - vn[m]);
                    gupmax(dua_x, v_c - vn[m]);
                    sx[m] = vn[m] - gn[m];
                }
                if constexpr (EXT) {
                    if (soc_x) {
#pragma unroll
                        for (int m = 0; m < RX; ++m) wc[m] = xf[m] + mkx(f.gc[m], m);
                        for (int c = 0; c < ncx; ++c) {
                            const uint4 mk = cm[c * G];
                            if constexpr (IC) {
                                const float mu = s_ilb[knot_sgpr(2 * (mlx + mlu) + c)];
                                if (mu <= FLT_MAX) project_soc_group<G, RX>(wc, mk.x, mk.y, (ST)mu);   // (+inf: not this instance's)
                            } else
                                project_soc_group<G, RX>(wc, mk.x, mk.y, (ST)P.cx[c]);
                        }
#pragma unroll
                        for (int m = 0; m < RX; ++m) {
                            gcn[m] = (mkx(f.gc[m], m) + xf[m]) - wc[m];
                            gupmax(pri_x, xf[m] - wc[m]);
                            gupmax(dua_x, mkx(f.vc[m], m) - wc[m]);
                            sx[m] += wc[m] - gcn[m];
                        }
                    }
                }
                if constexpr (EXT == 2) {
                    if (lin_x) {
#pragma unroll
                        for (int m = 0; m < RX; ++m) wl[m] = xf[m] + mkx(f.gl[m], m);
                        if constexpr (IC)
                            project_halfspaces_group<G, RX>(wl, lax, LSX, mlx, s_ilb, s_ilb + knot_sgpr(mlx));
                        else
                            project_halfspaces_group<G, RX>(wl, lax, LSX, mlx, lbx, ln2x);
#pragma unroll
                        for (int m = 0; m < RX; ++m) {
                            gln[m] = (mkx(f.gl[m], m) + xf[m]) - wl[m];
                            gupmax(pri_x, xf[m] - wl[m]);
                            gupmax(dua_x, mkx(f.vl[m], m) - wl[m]);
                            sx[m] += wl[m] - gln[m];
                        }
                    }
                }
                if (x_owner) {
                    if (!nog) stx(Sg, k, gn);
                    if (keep_w) stx(Sw, k, vn);
                    if constexpr (OS) stx(Ss, k, sx);
                    if constexpr (EXT)
                        if (soc_x) {
                            stx(Sgc, k, gcn);
                            if (keep_w) stx(Swc, k, wc);
                        }
                    if constexpr (EXT == 2)
                        if (lin_x) {
                            stx(Sgl, k, gln);
                            if (keep_w) stx(Swl, k, wl);
                        }
                }
                if constexpr (ADP) {
                    if (adapt_now) {
                        RT gk[RX], xfl[RX];
#pragma unroll
                        for (int m = 0; m < RX; ++m) gk[m] = (RT)gn[m], xfl[m] = (RT)xf[m];
                        if (k >= 1) {
                            RT atx[RX], atu[RU];
#pragma unroll
                            for (int m = 0; m < RX; ++m) atx[m] = (RT)0;
#pragma unroll
                            for (int m = 0; m < RU; ++m) atu[m] = (RT)0;
                            quad_matvec<G, RX, NXL, RX, NXP>(atx, cATT, gk);     // A' g_k
                            quad_matvec<G, RU, NXL, RX, NXP>(atu, cBT, gk);      // B' g_k
#pragma unroll
                            for (int m = 0; m < RX; ++m) {                       // state rows of knot k - 1
                                if (k >= 2) atx[m] -= (RT)a_gp[m];
                                const RT qv = (RT)cQD[m] * a_xp[m];
                                upmax_abs(a_dres, qv + qv + atx[m]);
                                upmax_abs(a_pxm, qv);
                                upmax_abs(a_qm, qv);
                                upmax_abs(a_atym, atx[m]);
                                // the rollout's own x_k makes A x + B u (+ f) - x_k vanish: the row is 0 against vnew_k
                                upmax_abs(a_pri, (RT)vn[m]);
                                upmax_abs(a_zm, (RT)vn[m]);
                            }
#pragma unroll
                            for (int m = 0; m < RU; ++m) {                       // input rows of knot k - 1
                                const RT px = (RT)cRD[m] * (RT)a_up[m], aty = (RT)a_yp[m] + atu[m];
                                upmax_abs(a_dres, px + px + aty);
                                upmax_abs(a_pxm, px);
                                upmax_abs(a_qm, px);
                                upmax_abs(a_atym, aty);
                            }
                        }
                        if (k == N - 1) {                                        // the terminal knot's own rows: Pinf x + Q~ x - g
                            RT px[RX];
#pragma unroll
                            for (int m = 0; m < RX; ++m) px[m] = (RT)0;
                            quad_matvec<G, RX, NXL, RX, NXP>(px, cPT, xfl);
#pragma unroll
                            for (int m = 0; m < RX; ++m) {
                                const RT qv = (RT)cQD[m] * xfl[m], aty = (k >= 1) ? -gk[m] : (RT)0;
                                upmax_abs(a_dres, px[m] + qv + aty);
                                upmax_abs(a_pxm, px[m]);
                                upmax_abs(a_qm, qv);
                                upmax_abs(a_atym, aty);
                            }
                        }
#pragma unroll
                        for (int m = 0; m < RX; ++m) a_xp[m] = xfl[m], a_gp[m] = gn[m];
                    }
                }
                if (pf) fetch_x(k + D, f);
                if (k < N - 1) {
                    RT u[RU], xn[RX];
                    ST uf[RU], zn[RU], yn[RU], zc2[RU], ycn[RU], zl2[RU], yln[RU], su[RU];
#pragma unroll
                    for (int m = 0; m < RU; ++m) u[m] = -(RT)mku(f.d[m], m);
#pragma unroll
                    for (int m = 0; m < RX; ++m) xn[m] = EXT ? (RT)cF[m] : (RT)0;
                    asm volatile("" ::: "memory");  // (and between products: each one's coefficient loads stay next to their use)
                    quad_matvec<G, RU, NXL, RX, NXP, true>(u, cK, x);    // u = -d - Kinf x
                    asm volatile("" ::: "memory");
                    quad_matvec<G, RX, NXL, RX, NXP>(xn, cA, x);   // A x (+ fdyn)
                    asm volatile("" ::: "memory");
#pragma unroll
                    for (int m = 0; m < RU; ++m) {
                        const ST y_c = mku(f.y[m], m);
                        uf[m] = (ST)u[m];
                        zn[m] = gmin(buhi(m), gmax(bulo(m), uf[m] + y_c));
                        yn[m] = (y_c + uf[m]) - zn[m];
                        gupmax(pri_u, uf[m] - zn[m]);
                        gupmax(dua_u, mku(f.z[m], m) - zn[m]);
                        su[m] = zn[m] - yn[m];
                    }
                    if constexpr (EXT) {
                        if (soc_u) {
#pragma unroll
                            for (int m = 0; m < RU; ++m) zc2[m] = uf[m] + mku(f.yc[m], m);
                            for (int c = 0; c < ncu; ++c) {
                                const uint4 mk = cm[c * G];
                                if constexpr (IC) {
                                    const float mu = s_ilb[knot_sgpr(2 * (mlx + mlu) + ncx + c)];
                                    if (mu <= FLT_MAX) project_soc_group<G, RU>(zc2, mk.z, mk.w, (ST)mu);
                                } else
                                    project_soc_group<G, RU>(zc2, mk.z, mk.w, (ST)P.cu[c]);
                            }
#pragma unroll
                            for (int m = 0; m < RU; ++m) {
                                ycn[m] = (mku(f.yc[m], m) + uf[m]) - zc2[m];
                                gupmax(pri_u, uf[m] - zc2[m]);
                                gupmax(dua_u, mku(f.zc[m], m) - zc2[m]);
                                su[m] += zc2[m] - ycn[m];
                            }
                        }
                    }
                    if constexpr (EXT == 2) {
                        if (lin_u) {
#pragma unroll
                            for (int m = 0; m < RU; ++m) zl2[m] = uf[m] + mku(f.yl[m], m);
                            if constexpr (IC)
                                project_halfspaces_group<G, RU>(zl2, lau, LSU, mlu, s_ilb + knot_sgpr(2 * mlx), s_ilb + knot_sgpr(2 * mlx + mlu));
                            else
                                project_halfspaces_group<G, RU>(zl2, lau, LSU, mlu, lbu, ln2u);
#pragma unroll
                            for (int m = 0; m < RU; ++m) {
                                yln[m] = (mku(f.yl[m], m) + uf[m]) - zl2[m];
                                gupmax(pri_u, uf[m] - zl2[m]);
                                gupmax(dua_u, mku(f.zl[m], m) - zl2[m]);
                                su[m] += zl2[m] - yln[m];
                            }
                        }
                    }
                    if (u_owner) {
                        stu(Sy, k, yn);
                        if (keep_w) stu(Szw, k, zn);
                        if constexpr (OS) stu(Ssu, k, su);
                        if constexpr (EXT)
                            if (soc_u) {
                                stu(Syc, k, ycn);
                                if (keep_w) stu(Szwc, k, zc2);
                            }
                        if constexpr (EXT == 2)
                            if (lin_u) {
                                stu(Syl, k, yln);
                                if (keep_w) stu(Szwl, k, zl2);
                            }
                    }
                    if constexpr (ADP) {
                        if (adapt_now) {
#pragma unroll
                            for (int m = 0; m < RU; ++m) {
                                upmax_abs(a_pri, (RT)uf[m] - (RT)zn[m]);
                                upmax_abs(a_axm, (RT)uf[m]);
                                upmax_abs(a_zm, (RT)zn[m]);
                                a_up[m] = uf[m], a_yp[m] = yn[m];
                            }
                        }
                    }
                    if (pf && k + D < N - 1) fetch_u(k + D, f);
                    asm volatile("" ::: "memory");
                    quad_matvec<G, RX, NUL, RU, NUP>(xn, cB, u);   // + B u
#pragma unroll
                    for (int m = 0; m < RX; ++m) x[m] = xn[m];
                }
            };
            sfor<0, D>([&](auto J) {
                constexpr int j = decltype(J)::value;
                if (j < N) {
                    fetch_x(j, fb[j]);
                    if (j < N - 1) fetch_u(j, fb[j]);
                }
            });
            for (int k0 = 0; k0 < N; k0 += D)
                sfor<0, D>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    if (k0 + j < N) fwd_knot(k0 + j, fb[j]);
                });
            it += 1;
            RT accP[RX];                                     // Pinf' xref_{N-1}, with the Pinf the linear cost was formed with
#pragma unroll
            for (int m = 0; m < RX; ++m) accP[m] = (RT)0;
            if constexpr (ADP) {
                if (P.ref_mode != REF_ZERO) {
                    RT xrl[RX];
#pragma unroll
                    for (int m = 0; m < RX; ++m) xrl[m] = (RT)ref_x(N - 1, m);
                    quad_matvec<G, RX, NXL, RX, NXP>(accP, cPT, xrl);
                }
                if (adapt_now) {
                    // predict_rho (rho_benchmark.cpp:173-195), then the first-order update of Kinf, Pinf (admm.cpp:160-172)
                    const RT pri = group_max_t<G>(a_pri), axm = group_max_t<G>(a_axm), zm = group_max_t<G>(a_zm),
                             dres = group_max_t<G>(a_dres), pxm = group_max_t<G>(a_pxm), atym = group_max_t<G>(a_atym),
                             qm = group_max_t<G>(a_qm);
                    const RT eps = (RT)1e-10, prin = axm > zm ? axm : zm;
                    RT duan = pxm > atym ? pxm : atym;
                    duan = qm > duan ? qm : duan;
                    const RT ratio = (pri / (prin + eps)) / (dres / (duan + eps) + eps);
                    RT nrho = (RT)rho_d * (RT)sqrt((double)ratio);
                    if (P.rho_clip) nrho = nrho < (RT)P.rho_min ? (RT)P.rho_min : (nrho > (RT)P.rho_max ? (RT)P.rho_max : nrho);
                    const double delta = (double)nrho - rho_d;
                    const long AB = P.adapt_stride;
                    double *ad = P.adapt + b;
                    RT *mine = adp_cols + L;
                    const double *sK = P.sens, *sP = P.sens + NU * NX;
#pragma unroll
                    for (int m = 0; m < RU; ++m) {
                        const int a = q * RU + m;
                        if (a < NU)
                            for (int j = 0; j < NX; ++j) {       // this lane owns row a of Kinf: the solver's state and its own copy
                                const double v = ad[(long)(1 + a + j * NU) * AB] + delta * sK[a + j * NU];
                                ad[(long)(1 + a + j * NU) * AB] = v;
                                mine[(long)(PK::AO_K + m * NXP + j) * BG] = (RT)v;
                            }
                    }
#pragma unroll
                    for (int m = 0; m < RX; ++m) {
                        const int r = q * RX + m;
                        if (r < NX) {
                            for (int a = 0; a < NU; ++a) {       // Kinf^T rows: another lane owns the state's copy
                                RT *c = mine + (long)(PK::AO_KT + m * NUP + a) * BG;
                                *c = (RT)((double)*c + delta * sK[a + r * NU]);
                            }
                            for (int j = 0; j < NX; ++j) {       // column r of Pinf
                                const double v = ad[(long)(1 + NU * NX + j + r * NX) * AB] + delta * sP[j + r * NX];
                                ad[(long)(1 + NU * NX + j + r * NX) * AB] = v;
                                mine[(long)(PK::AO_PT + m * NXP + j) * BG] = (RT)v;
                            }
                        }
                    }
                    if (q == 0) ad[0] = (double)nrho;
                    rho_d = (double)nrho;
                    rho = (ST)(float)nrho;
                }
            }
            if (need_res) {
                if constexpr (WIDE) {
                    // fp64 state compares what the reference compares: fp64 residuals against the fp64 tolerances (admm.cpp:99-103)
                    const ST r0 = group_max_s<G>(pri_x), r1 = group_max_s<G>(dua_x) * rho, r2 = group_max_s<G>(pri_u),
                             r3 = group_max_s<G>(dua_u) * rho;
                    res0 = (float)r0, res1 = (float)r1, res2 = (float)r2, res3 = (float)r3;
                    if (r0 < P.abs_pri_tol64 && r2 < P.abs_pri_tol64 && r1 < P.abs_dua_tol64 && r3 < P.abs_dua_tol64) conv = 1;
                } else {
                    res0 = group_max<G>(pri_x);
                    res1 = group_max<G>(dua_x) * rho;
                    res2 = group_max<G>(pri_u);
                    res3 = group_max<G>(dua_u) * rho;
                    if (res0 < P.abs_pri_tol && res2 < P.abs_pri_tol && res1 < P.abs_dua_tol && res3 < P.abs_dua_tol)
                        conv = 1;
                }
            }
            if (!conv) {
                // ================= fused backward sweep (admm.cpp:75-83, :196-197, :13-20) =================
                // per knot it needs vnew - g (+ the cone set's) and znew - y (+ ...): the fused arrays in OS mode,
                // else formed from w, g, (wc, gc) while copying w -> v, zw -> z (admm.cpp:196-197)
                auto fetchb_x = [&](int k_, BwdBuf &f) __attribute__((always_inline)) {
                    const int k = knot_sgpr(k_);
                    if constexpr (OS) {
                        ldx(Ss, k, f.w);
                    } else {
                        ldx(Sw, k, f.w);
                        ldx(Sg, k, f.g);
                        if (soc_x) {
                            ldx(Swc, k, f.wc);
                            ldx(Sgc, k, f.gc);
                        }
                        if (lin_x) {
                            ldx(Swl, k, f.wl);
                            ldx(Sgl, k, f.gl);
                        }
                    }
                };
                auto fetchb_u = [&](int k_, BwdBuf &f) __attribute__((always_inline)) {
                    const int k = knot_sgpr(k_);
                    if constexpr (OS) {
                        ldu(Ssu, k, f.zw);
                    } else {
                        ldu(Szw, k, f.zw);
                        ldu(Sy, k, f.y);
                        if (soc_u) {
                            ldu(Szwc, k, f.zwc);
                            ldu(Syc, k, f.yc);
                        }
                        if (lin_u) {
                            ldu(Szwl, k, f.zwl);
                            ldu(Syl, k, f.yl);
                        }
                    }
                };
                // consume the state-shaped part of a buffer: returns rho-less (vnew - g [+ cone set]) per row
                auto take_x = [&](int k, BwdBuf &f, ST (&sx)[RX]) {
                    if constexpr (OS) {
#pragma unroll
                        for (int m = 0; m < RX; ++m) sx[m] = mkx(f.w[m], m);
                    } else {
#pragma unroll
                        for (int m = 0; m < RX; ++m) {
                            sx[m] = mkx(f.w[m] - f.g[m], m);
                            if (soc_x) sx[m] += mkx(f.wc[m] - f.gc[m], m);
                            if (lin_x) sx[m] += mkx(f.wl[m] - f.gl[m], m);
                        }
                        if (x_owner) {
                            stx(Sv, k, f.w);
                            if (soc_x) stx(Svc, k, f.wc);
                            if (lin_x) stx(Svl, k, f.wl);
                        }
                    }
                };
                auto take_u = [&](int k, BwdBuf &f, ST (&su)[RU]) {
                    if constexpr (OS) {
#pragma unroll
                        for (int m = 0; m < RU; ++m) su[m] = mku(f.zw[m], m);
                    } else {
#pragma unroll
                        for (int m = 0; m < RU; ++m) {
                            su[m] = mku(f.zw[m] - f.y[m], m);
                            if (soc_u) su[m] += mku(f.zwc[m] - f.yc[m], m);
                            if (lin_u) su[m] += mku(f.zwl[m] - f.yl[m], m);
                        }
                        if (u_owner) {
                            stu(Sz, k, f.zw);
                            if (soc_u) stu(Szc, k, f.zwc);
                            if (lin_u) stu(Szl, k, f.zwl);
                        }
                    }
                };
                BwdBuf bbuf[D], bterm;
                fetchb_x(N - 1, bterm);
                sfor<0, D>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    if (j < N - 1) {
                        fetchb_x(N - 2 - j, bbuf[j]);
                        fetchb_u(N - 2 - j, bbuf[j]);
                    }
                });
                RT p[RX];
                {
                    RT acc[RX];
#pragma unroll
                    for (int m = 0; m < RX; ++m) acc[m] = accP[m];
                    if (!ADP && P.ref_mode != REF_ZERO) {
                        RT xrl[RX];
#pragma unroll
                        for (int m = 0; m < RX; ++m) xrl[m] = (RT)ref_x(N - 1, m);
                        quad_matvec<G, RX, NXL, RX, NXP>(acc, cPT, xrl);
                    }
                    ST sx[RX];
                    take_x(N - 1, bterm, sx);
#pragma unroll
                    for (int m = 0; m < RX; ++m) p[m] = -acc[m] - (RT)(rho_lin * sx[m]);
                }
                auto bwd_knot = [&](int t_, BwdBuf &f) __attribute__((always_inline)) {  // t counts knots from N-2 downwards
                    asm volatile("" ::: "memory");
                    const int t = knot_sgpr(t_);
                    const int k = N - 2 - t;
                    RT r[RU], qk[RX];
                    ST sx[RX], su[RU];
                    take_x(k, f, sx);
                    take_u(k, f, su);
#pragma unroll
                    for (int m = 0; m < RU; ++m) r[m] = (RT)(-((ST)ref_u(k, m) * (ST)cRD[m]) - rho_lin * su[m]);
#pragma unroll
                    for (int m = 0; m < RX; ++m) qk[m] = (RT)(-((ST)ref_x(k, m) * (ST)cQD[m]) - rho_lin * sx[m]);
                    if (t + D < N - 1) {
                        fetchb_x(k - D, f);
                        fetchb_u(k - D, f);
                    }
                    RT tt[RU], dn[RU], ap[RX];
                    ST dnf[RU];
#pragma unroll
                    for (int m = 0; m < RU; ++m) {
                        tt[m] = r[m] + (EXT ? (RT)cBPF[m] : (RT)0);
                        dn[m] = (RT)0;
                    }
                    asm volatile("" ::: "memory");
                    quad_matvec<G, RU, NXL, RX, NXP>(tt, cBT, p);   // B^T p + r (+ BPf)
                    asm volatile("" ::: "memory");
                    quad_matvec<G, RU, NUL, RU, NUP>(dn, cQI, tt);  // d = Quu_inv (...)
#pragma unroll
                    for (int m = 0; m < RU; ++m) dnf[m] = (ST)dn[m];
                    if (u_owner) stu(Sd, k, dnf);
#pragma unroll
                    for (int m = 0; m < RX; ++m) ap[m] = qk[m] + (EXT ? (RT)cAPF[m] : (RT)0);
                    asm volatile("" ::: "memory");
                    quad_matvec<G, RX, NUL, RU, NUP, true>(ap, cKT, r);   // q (+ APf) - Kinf^T r: does not wait for p
                    asm volatile("" ::: "memory");
                    quad_matvec<G, RX, NXL, RX, NXP>(ap, cAT, p);         // + AmBKt p
#pragma unroll
                    for (int m = 0; m < RX; ++m) p[m] = ap[m];
                };
                for (int t0 = 0; t0 < N - 1; t0 += D)
                    sfor<0, D>([&](auto J) {
                        constexpr int j = decltype(J)::value;
                        if (t0 + j < N - 1) bwd_knot(t0 + j, bbuf[j]);
                    });
            }
        }
        if (!__builtin_amdgcn_ballot_w64(active && !conv)) break;
    }
#if TMPC_STREAMG_MPC
    {
        // ---- one closed-loop step behind the solve (every lane of the wavefront is here: the loop above ends wave-wide) ----
        double *const xplant = const_cast<double *>(P.x0d);   // the launch owns the plant state, as plant_step_kernel does in the chain
        float u0[RU];
        double xd[RX], u0d[RU], xn[RX];
#pragma unroll
        for (int m = 0; m < RU; ++m) {
            u0[m] = (active && q * RU + m < NU) ? (float)*SUP(Szw, 0, m) : 0.f;
            u0d[m] = (double)u0[m];
        }
#pragma unroll
        for (int m = 0; m < RX; ++m) {
            xd[m] = (active && q * RX + m < NX) ? xplant[b * NX + q * RX + m] : 0.0;
            xn[m] = 0.0;
            if constexpr (EXT != 0)
                if (P.has_fdyn) xn[m] = (double)cF[m];
        }
        sfor<0, NXL>([&](auto s) {
            constexpr int S_ = decltype(s)::value;
#pragma unroll
            for (int k = 0; k < RX; ++k) {
                const double xv = gbcast<G, S_>(xd[k]);
                if (S_ * RX + k < NX) {
#pragma unroll
                    for (int m = 0; m < RX; ++m) xn[m] = fma((double)cA[m * NXP + S_ * RX + k], xv, xn[m]);
                }
            }
        });
        sfor<0, NUL>([&](auto s) {
            constexpr int S_ = decltype(s)::value;
#pragma unroll
            for (int k = 0; k < RU; ++k) {
                const double uv = gbcast<G, S_>(u0d[k]);
                if (S_ * RU + k < NU) {
#pragma unroll
                    for (int m = 0; m < RX; ++m) xn[m] = fma((double)cB[m * NUP + S_ * RU + k], uv, xn[m]);
                }
            }
        });
        const bool more = step + 1 < nsteps;
        if (active) {
            const long so = b * nsteps + step;
#pragma unroll
            for (int m = 0; m < RX; ++m)
                if (q * RX + m < NX) {
                    xplant[b * NX + q * RX + m] = xn[m];
                    P.mpc_x[so * NX + q * RX + m] = (float)xn[m];
                    if (!more) P.x0_out[b * NX + q * RX + m] = (float)xn[m];
                }
#pragma unroll
            for (int m = 0; m < RU; ++m)
                if (q * RU + m < NU) P.mpc_u[so * NU + q * RU + m] = u0[m];
            if (q == 0) P.mpc_iter[so] = conv ? P.iter_offset + it : -(P.iter_offset + it);
        }
        if (more) {
            // the next solve: from the rounded plant state, iteration count and flag reset, residuals kept (a warm launch reads
            // back what the previous one wrote), the work arrays zeroed as the warm load zeroes them
#pragma unroll
            for (int m = 0; m < RX; ++m) x0[m] = (active && q * RX + m < NX) ? (RT)(float)xn[m] : (RT)0;
            it = 0, conv = 0;
            if (P.xref_seq) xrefp = P.xref_seq + (long)(step + 1) * EX, urefp = P.uref_seq + (long)(step + 1) * EU;
            if (active) {
                for (int k = 0; k < N; ++k)
#pragma unroll
                    for (int m = 0; m < RX; ++m) {
                        if (q * RX + m >= NX) continue;
                        *SXP(Sw, k, m) = 0.f;
                        if (soc_x) *SXP(Swc, k, m) = 0.f;
                        if (lin_x) *SXP(Swl, k, m) = 0.f;
                    }
                for (int k = 0; k < N - 1; ++k)
#pragma unroll
                    for (int m = 0; m < RU; ++m) {
                        if (q * RU + m >= NU) continue;
                        *SUP(Szw, k, m) = 0.f;
                        if (soc_u) *SUP(Szwc, k, m) = 0.f;
                        if (lin_u) *SUP(Szwl, k, m) = 0.f;
                    }
            }
        }
    }
    }
#endif

    if (active) {
        for (int k = 0; k < N; ++k)
#pragma unroll
            for (int m = 0; m < RX; ++m)
                if (q * RX + m < NX) P.xout[b * EX + k * NX + q * RX + m] = (float)*SXP(Sw, k, m);
        for (int k = 0; k < N - 1; ++k)
#pragma unroll
            for (int m = 0; m < RU; ++m)
                if (q * RU + m < NU) P.uout[b * EU + k * NU + q * RU + m] = (float)*SUP(Szw, k, m);
        if (q == 0) {
            P.iter[b] = P.iter_offset + it;
            P.solved[b] = conv;
            P.res[b * 4 + 0] = res0;
            P.res[b * 4 + 1] = res1;
            P.res[b * 4 + 2] = res2;
            P.res[b * 4 + 3] = res3;
        }
        if constexpr (!OS) {
            if (P.save_state) {
                for (int k = 0; k < N; ++k)
#pragma unroll
                    for (int m = 0; m < RX; ++m) {
                        const int row = q * RX + m;
                        if (row < NX) {
                            WSA(sg)[b * EX + k * NX + row] = *SXP(Sg, k, m);
                            WSA(sv)[b * EX + k * NX + row] = *SXP(Sv, k, m);
                            if (soc_x) {
                                WSA(sgc)[b * EX + k * NX + row] = *SXP(Sgc, k, m);
                                WSA(svc)[b * EX + k * NX + row] = *SXP(Svc, k, m);
                            }
                            if (lin_x) {
                                WSA(sgl)[b * EX + k * NX + row] = *SXP(Sgl, k, m);
                                WSA(svl)[b * EX + k * NX + row] = *SXP(Svl, k, m);
                            }
                        }
                    }
                for (int k = 0; k < N - 1; ++k)
#pragma unroll
                    for (int m = 0; m < RU; ++m) {
                        const int row = q * RU + m;
                        if (row < NU) {
                            WSA(sy)[b * EU + k * NU + row] = *SUP(Sy, k, m);
                            WSA(sz)[b * EU + k * NU + row] = *SUP(Sz, k, m);
                            WSA(sd)[b * EU + k * NU + row] = *SUP(Sd, k, m);
                            if (soc_u) {
                                WSA(syc)[b * EU + k * NU + row] = *SUP(Syc, k, m);
                                WSA(szc)[b * EU + k * NU + row] = *SUP(Szc, k, m);
                            }
                            if (lin_u) {
                                WSA(syl)[b * EU + k * NU + row] = *SUP(Syl, k, m);
                                WSA(szl)[b * EU + k * NU + row] = *SUP(Szl, k, m);
                            }
                        }
                    }
            }
        }
    }
#undef WSA
#undef SXP
#undef SUP
#undef OKX
#undef OKU
#undef TMPC_XREF
#undef TMPC_UREF
    {
        float m0 = active ? res0 : 0.f, m1 = active ? res1 : 0.f, m2 = active ? res2 : 0.f, m3 = active ? res3 : 0.f;
#pragma unroll
        for (int off = G; off < 64; off <<= 1) {
            m0 = fmaxf(m0, __shfl_xor(m0, off, 64));
            m1 = fmaxf(m1, __shfl_xor(m1, off, 64));
            m2 = fmaxf(m2, __shfl_xor(m2, off, 64));
            m3 = fmaxf(m3, __shfl_xor(m3, off, 64));
        }
        const unsigned long long unsolved = __builtin_amdgcn_ballot_w64(active && !conv && q == 0);
        fold_status(P, m0, m1, m2, m3, __popcll(unsolved), tid);
    }
}

}  // namespace tmpc
#if !TMPC_STREAMG_MPC && !TMPC_STREAMG_IB && !TMPC_STREAMG_IL && !TMPC_STREAMG_IC
#undef TMPC_STREAMG_MPC
#define TMPC_STREAMG_MPC 1
#include "admm_streamg.hip.h"
#undef TMPC_STREAMG_MPC
#define TMPC_STREAMG_MPC 0
#undef TMPC_STREAMG_IB
#define TMPC_STREAMG_IB 1
#include "admm_streamg.hip.h"
#undef TMPC_STREAMG_IB
#define TMPC_STREAMG_IB 0
#undef TMPC_STREAMG_IL
#define TMPC_STREAMG_IL 1
#include "admm_streamg.hip.h"
#undef TMPC_STREAMG_IL
#define TMPC_STREAMG_IL 0
#undef TMPC_STREAMG_IC
#define TMPC_STREAMG_IC 1
#include "admm_streamg.hip.h"
#define TMPC_STREAMG_BOTH
#endif
#endif  // TMPC_STREAMG_BOTH
