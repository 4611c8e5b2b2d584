// Fused TinyMPC ADMM kernel for gfx950 — "lean" layout: the benchmark's calling pattern of the small shapes with as few
// vector instructions per ADMM iteration as the arithmetic allows.
//
// What it computes: the reference's solve() loop (src/codegen_src/tinympc/admm.cpp:109-207; phases :13-107) of a
// box-constrained family, zero or shared references, fp64 recurrences: one-shot solves — cold start (the zero workspace
// tiny_setup leaves, tiny_api.cpp:73-88), nothing of the workspace kept — and, in the WS form (described at the kernel, routed
// to with TINYMPC_HIP_LEAN_WS), solves that go on from the kept workspace and leave it as the reference does, which is what a
// host-stepped or chained closed loop is made of.  One lane per instance, like quad<..., g1> (admm_quad.hip.h), which stays the
// kernel of every other calling pattern of the shape (per-instance references, adaptive rho, fp32 recurrences, chunked
// solves, the in-kernel closed loop — and, without the switch, every kept-workspace solve).  The benchmark's pattern — no active state bound, zero
// references — is the XB = false, REFS = REF_ZERO instantiation described first; XB / REF_SHARED add what they need and
// nothing to that instantiation (profiles/r04_cartpole_isa_census.json is its loop).
//
// Why a separate kernel (round 3 review, item 1): quad<4,1,20,g1> executed 1 506 vector instructions per iteration, of
// which 911 were the recurrences' fp64 FMAs; 268 were v_accvgpr moves (its state homed in AGPRs and copied through VGPRs
// every iteration) and 228 fp32 <-> fp64 conversions.  A lone wavefront issues one vector instruction per 4 cycles
// whatever its type (MI355X_MICROARCH.md, "vector-instruction ISSUE cost"), so the instruction count IS the time.  Here:
//   * without an active state bound the state slack is the rollout itself (vnew = x + g clamps nothing, so g stays 0 and
//     vnew = x: admm.cpp:46-58, :67-68) — the trajectory x is kept in fp64 registers and IS v: no x -> fp32 -> fp64 round
//     trip between the forward and the backward sweep (8 conversions per knot), and v is MORE accurate than the fp32 copy;
//   * the whole iterated state — x (fp64), y, znew, d (fp32): 2 nx N + 3 nu (N-1) registers = 217 for cartpole N = 20 —
//     plus the working set of a knot fits the 256 architectural VGPRs: no AGPR homes, no moves, and the kernel may run two
//     wavefronts per SIMD when the batch has them (__launch_bounds__(256, 2));
//   * the backward recursion runs on p~ = -p / rho, r~ = -r / rho: with zero references q = -rho x, r = -rho (z - y)
//     (admm.cpp:77-80), so p~_k = x_k + AmBKt p~_{k+1} - Kinf' r~_k starts from the x register itself and the products by
//     rho disappear; d_k = (-rho Quu_inv) (B' p~_{k+1} + r~_k) (admm.cpp:17-18);
//   * the rollout is regrouped as x+ = (A - B Kinf) x - B d, u = -Kinf x - d (admm.cpp:29-30; fp64, results move by
//     ~1e-16): x+ does not wait for u, and (A - B Kinf) is the transpose of the AmBKt the backward sweep reads, so ONE set
//     of 25 fp64 coefficients (50 SGPRs) serves both sweeps and stays resident for the whole solve — no per-sweep scalar
//     reloads.  (The host only selects this kernel when cache.AmBKt equals (A - B Kinf)' — set_cache_terms may break that.)
// XB (some enabled state bound is finite): the state slack is no longer the rollout.  The rollout is then a running fp64
// vector; per element the iteration keeps the state dual g and q~ = vnew - g (what the backward sweep starts from) in fp32
// — still 217 registers — and forms them in fp32 from the rounded x as every fp32-state kernel does (admm.cpp:46-58, 67-68,
// 79-80); the solution vnew = q~ + g is re-clamped at the store.  REF_SHARED: the reference terms of update_linear_cost
// (admm.cpp:77-82) scaled by -1 / rho — Q~ xref_k / rho, R~ uref_k / rho, Pinf' xref_{N-1} / rho — are formed once per
// workgroup in fp64 and read from LDS (broadcast) in the backward sweep.
// Termination (admm.cpp:89-107) as in the quad kernel: residual maxima only on the iterations whose check can matter; with
// positive tolerances (LIVE) an instance that converges stores its solution at that iteration and its lane idles on
// (what the matrix-core kernels do), the wavefront leaves when all its instances are done.
#pragma once
#include <hip/hip_runtime.h>

#include "admm_params.h"
#include "admm_quad.hip.h"   // SBlock, sfor

#ifndef TMPC_LEAN_KNOT_BARRIER
#define TMPC_LEAN_KNOT_BARRIER 0   // 1: a scheduling barrier per knot (keeps the scheduler from hoisting a later knot's loads / conversions)
#endif
#ifndef TMPC_LEAN_SPLITK
#define TMPC_LEAN_SPLITK 0    // 1: Kinf x as two chains of two (+ an add): shorter dependent chain, one more instruction
#endif

#ifndef TMPC_LEAN_WIDE_STORE
#define TMPC_LEAN_WIDE_STORE 1    // 0: the final store in 4-byte pieces (store_wave_coalesced) at every shape
#endif
#ifndef TMPC_LEAN_STORE_W
#define TMPC_LEAN_STORE_W 0       // floats per instance and pass of the wide store; 0: wide_stage_width(EX) (tuning aid)
#endif
#ifndef TMPC_LEAN_PK
// 1: the headline form (PK, at the kernel) updates input slack and dual of two knots at a time with packed fp32 adds
// (v_pk_add_f32: a lone wavefront issues it at the rate of any vector instruction, profiles/r07_fp64_issue_probe.txt);
// 0: one knot at a time everywhere (the A/B switch)
#define TMPC_LEAN_PK 1
#endif
#ifndef TMPC_LEAN_FOLD_FIRST
// 1: the status fold ahead of the final store (its fence then has no solution stores to wait for).  Tried and left off: the
// folding wavefront's stores then wait for the fold's atomics and ticket (the fold is 11-20 us behind 256 workgroups, not 3),
// while the other three wavefronts' stores already fill the L2 its fence writes back — the headline step 0.1352 -> 0.1405 ms
// (profiles/r07_lean_ab.txt)
#define TMPC_LEAN_FOLD_FIRST 0
#endif

namespace tmpc {

template <int NX, int NU>
struct LeanPack {
    static constexpr LeanLayout LL = lean_layout(NX, NU);
    static constexpr int O_M = LL.oM, O_K = LL.oK, O_B = LL.oB, O_C = LL.oC, O_H = LL.oH, O_S = LL.oS, O_P = LL.oP, O_T = LL.oT, LEN = LL.len;
    static constexpr int NLOADS = LL.padded / 8;     // s_load_dwordx16 per 8 doubles
    static constexpr int O_Z = LL.oZ, O_W = LL.oW, O_SC = LL.oSc, O_SI = LL.oSi, NLOADS_Z = LL.padZ / 8;   // the scaled block (SCL)
};

typedef float lean_f2 __attribute__((ext_vector_type(2)));   // a pair of knots' fp32 values (PK)

// clamp(t, lo, hi) as one v_med3_f32 (lo <= hi; +-inf for "no bound")
__device__ __forceinline__ float clamp3(float t, float lo, float hi) { return __builtin_amdgcn_fmed3f(t, lo, hi); }
__device__ __forceinline__ double clamp3(double t, double lo, double hi) { return fmin(fmax(t, lo), hi); }
__device__ __forceinline__ float lean_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double lean_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float lean_abs(float a) { return fabsf(a); }
__device__ __forceinline__ double lean_abs(double a) { return fabs(a); }

// ONE: the launch has at most one wavefront per SIMD (batch <= 256 x CUs), so the kernel may take the whole register file:
// the feed-forward term d is then kept in fp64 too (nu (N-1) more registers, two conversions per knot fewer: 3.5 % of the
// instructions).  Otherwise (fixed-iteration solves of larger batches) the kernel is held to 256 registers and two wavefronts
// share a SIMD: within 3 % of 512-register wavefronts taking turns without a state bound, 12 % better with one; the
// tolerance-terminated (LIVE) kernels spill at 256 registers and are only built in the ONE form (lean_entry.hip.h).
// ST: the type of the slack / dual state.  float: the library's precision 0 (fp64 recurrences, fp32 state).  double: the
// reference's own arithmetic end to end (types.hpp:15) — precision 2 for one-shot solves of the shapes this kernel holds, at
// this kernel's speed instead of the generic kernel's; only ever specialised on request (jit.cpp), in the ONE form.
// SP: the zero / unit pattern of the model's (A, B) the kernel is built for (admm_params.h: lean_pattern_covers), 0: none.
// WS: the workspace-keeping form.  P.cold_start / P.save_state are honoured at run time, as the quad kernel does: a warm solve
// goes on from the d, y, g, v, z the previous one left (admm.cpp:111-115), a saving one leaves what the reference's workspace
// holds at its exit — and the plant state comes from P.x0d (fp64) when the caller chains a closed loop.  The arrays travel
// through the wavefront's LDS staging both ways (load_wave_x / load_wave_u, the staged stores below).  A converged exit
// returns BEFORE v = vnew, z = znew and the backward pass (admm.cpp:181-193), so the workspace then holds the PREVIOUS
// iteration's v, z and d: d is still in its registers; v and z are parked in LDS as floats (what the workspace holds anyway)
// by the residual iteration just before each knot overwrites them.  A converging wavefront stores solution and workspace
// through the staging with the ballot of its converging lanes as the mask — in the steady state of a warm-started loop every
// lane of a wavefront converges at the same check — and its lanes idle on as in the one-shot form; nothing of them is
// stored again.  Without XB the form assumes the workspace's g is zero and leaves it alone (the host picks XB otherwise).
// MPC (WS, LIVE, ONE; routed to with TINYMPC_HIP_LEAN_LOOP beside TINYMPC_HIP_LEAN_WS): the closed loop of P.mpc_steps warm
// solves in one launch — what the chain of WS launches and plant_step_kernel (solver.hip) computes, step by step, with the
// workspace kept on chip between the steps.  The instances of a wavefront do not leave a step together (their iteration
// counts differ; at a sparse check converged and max_iter exits mix), so every lane keeps the workspace of ITS OWN exit while
// the rest of its wavefront iterates on:
//   * v, z: the lane's row of the parked slack.  The parking writes are masked by `!conv`, so a converged lane's row stays
//     what it was at its exit (the previous iteration's v, z); a lane that leaves at max_iter writes its vnew, znew there;
//   * y, d (and g): to the workspace arrays through the masked staged stores — a converged lane's at its convergence, ahead
//     of the backward pass that would overwrite the d it leaves; the others' at the end of the step — 2 nu (N-1) floats per
//     instance and step where a chained launch moves the whole workspace and the solution both ways;
//   * the control it applies, znew_0 as a float, captured at the exit.
// A step then starts from the rows and the arrays: every value crosses the workspace's own format (fp32), as in the chain.
// The arrays are re-read by the wavefront that wrote them: s_waitcnt vmcnt(0) behind the stores, an agent-scope acquire
// ahead of the loads (the L1 may hold the lines of the previous read).  Nothing between the steps is wider than a
// wavefront: no workgroup barrier (wavefronts of a workgroup reach their steps at different times, ragged workgroups have
// wavefronts without an active lane).  The plant step x0 <- A x0 + B u0 is plant_step_kernel's arithmetic (fp64, the model's
// own A and B from the pack's sparse block, A terms by column, then B terms), the log its layout.  The last step is the WS
// form's solve unchanged: solution, status, residuals, the workspace when P.save_state; behind it the last plant step leaves
// the plant state in P.x0_out and, in fp64, in P.x0d, where it came from.  The kept workspace is always loaded (the host
// sends no cold start here).
constexpr int lean_park_stride(int EX) { return (((EX + 3) / 4) % 2 ? (EX + 3) / 4 : (EX + 3) / 4 + 1) * 4; }   // an odd number of float4
template <int NX, int NU, int N, bool LIVE, bool UBK, bool ONE, bool XB = false, int REFS = REF_ZERO, class ST = float, uint64_t SP = 0, bool WS = false,
          bool MPC = false>
__global__ __launch_bounds__(256, (ONE ? 1 : 2)) void admm_lean_kernel(const AdmmParams P) {
    constexpr bool F64 = std::is_same<ST, double>::value;
    static_assert(!F64 || ONE, "fp64 state: the 512-register form");
    static_assert(!WS || !F64, "kept workspace: fp32 state (the fp64 workspace has another format)");
    static_assert(!MPC || (WS && LIVE && ONE), "in-kernel closed loop: the tolerance-terminated workspace-keeping form");
    static_assert(REFS == REF_ZERO || REFS == REF_SHARED, "lean kernel: zero or shared references");
#ifdef TMPC_LEAN_CLOCK_PROBE
    const unsigned long long probe_entry = __builtin_amdgcn_s_memrealtime();
#endif
    using L = LeanPack<NX, NU>;
    constexpr int EX = NX * N, EU = NU * (N - 1);
    // Fixed-iteration solves without an active state bound iterate in controller-Hessenberg coordinates x = T x^ (T
    // orthogonal, admm_params.h: LeanLayout): M^ = T' M T has lower bandwidth NU and b^ = T' B is upper trapezoidal, so the
    // sweeps skip M^[m][j] (j < m - NU) and b^[m][a] (m > a) at compile time — cartpole: 37 fp64 FMAs per knot for 49.  The
    // recursion keeps its form (p^ = x^ + M^' p^ - k^' r~ needs T' T = I); u, z, y, d, r~ are input-space and unchanged.  The
    // state is mapped back (x = T x^) only where it leaves the sweeps: the residual iteration and the store.  LIVE would pay
    // that at every check, XB needs x at every knot: both keep the plain coordinates.  So does the 256-register form: it
    // sits at 246 registers and the reordered residual iteration spills 30-50 of them there (and its launches are bound by
    // two wavefronts sharing a SIMD's issue, not by one wavefront's instruction count alone).
    // SP != 0 (any variant): the sweeps in the plain coordinates on the model's own sparse A and B instead of the dense
    // A - B Kinf — u = -Kinf x - d, x+ = A x + B u; t = B' p~ + r~, d = C t, p~ = x + A' p~ - Kinf' t (the recursion above with
    // AmBKt = A' - Kinf' B') — skipping the zeros of the pattern at compile time and never reading its units: a row of x+
    // starts from x_j where A[m][j] is 1, a unit of A' p~ is an add.  Cartpole: 27 fp64 FMAs per knot for 37 (HB) or 49.
    constexpr bool SPR = SP != 0;
    // SCL (SP a scaled pattern, admm_params.h: lean_pattern_scaled; one-shot forms without a state bound): the sparse sweeps on the
    // diagonally scaled model x^ = S x — A^ = S A S^-1 and B^ = S B have units the model's own A and B lack, so a forward row
    // that had no free start gets one (from x^_j, or from u_a where B^'s unit sits) — cartpole: 25 fp64 per knot for 27.  The
    // backward recursion runs on p^ = S^-1 p~: a column starts fma(w_m, x^_m, <a unit term>), w = s^-2 beside the coefficients
    // in SGPRs.  u, d, t, r~, y, z and the clamp are input-space and unchanged; x = S^-1 x^ only at the stores, and the state
    // dual residual is max_m (max_k |x^_prev - x^_new|)_m / |s_m| (the maximum commutes with a positive scale).
    // FOLD (SCL with one input): C = -rho Quu_inv is then a scalar c, and the costate's scale relative to x^ — which the diagonal
    // scaling left free — takes it in: the recursion carries pv = c p^.  d_k = c r~_k + B^' pv_{k+1} needs no product by C (the
    // one chain of the iteration that had no free start), pv_k = Wv x^_k + A^' pv_{k+1} - K^' d_k keeps the chains of p^_k with
    // d_k where t_k stood, pv_{N-1} = Wv x^_{N-1}, and the pack's w holds Wv = c S^-2 (kernels.hip: build_lean_pack) —
    // cartpole: 24 fp64 per knot for 25.  Only the costate, which is never stored, changes its scale: d, u, x^ and every
    // fp32 quantity are what they were up to fp64 rounding.
    constexpr bool SCL = lsp_scaled(SP);
    constexpr bool FOLD = SCL && NU == 1;
    static_assert(!SCL || (!XB && !WS && !F64 && REFS == REF_ZERO), "scaled pattern: one-shot, no state bound, zero references, fp32 state");
    static_assert(!SCL || L::NLOADS_Z <= 4, "scaled coefficient block too large for SGPRs");
    static_assert(!SPR || (NX <= 4 && NU <= 4), "sparse pattern: nx, nu <= 4");
    constexpr bool HB = !SPR && !LIVE && !XB && ONE;
    // PK (the headline form: one wavefront per SIMD, fixed iterations, no state bound, nothing kept, one set of input bounds,
    // fp32 state): the iterations without residuals update slack and dual of the knots (k - 1, k), k odd, together — per input
    // row t = {u_{k-1}, u_k} + {y_{k-1}, y_k} and y = t - znew as packed adds (the clamp has no packed form), and in the
    // backward sweep r~ = znew - y of both knots in one packed subtract.  The slack is not on the rollout's chain (x+ takes the
    // unclamped u), so the even knot only parks (float)u for one knot; an unpaired last knot stays scalar.  The same IEEE
    // operations on the same values: results are bit-identical to the scalar form.
    constexpr bool PK = TMPC_LEAN_PK && ONE && !LIVE && !XB && !WS && UBK && !F64;
    auto mh_zero = [](int m, int j) { return HB && j < m - NU; };               // M^[m][j] outside the band
    auto bh_zero = [](int m, int a) { return HB && m > a; };                    // b^[m][a] below the trapezoid
    auto a_nz = [](int m, int j) { return !SPR || lsp_a(SP, NX, m, j); };       // SP: A[m][j] is not zero
    auto a_one = [](int m, int j) { return SPR && lsp_one(SP, NX, m, j); };     //     A[m][j] is exactly 1
    auto b_nz = [](int m, int a) { return !SPR || lsp_b(SP, NU, m, a); };       //     B[m][a] is not zero
    auto b_one = [](int m, int a) { return SCL && lsp_b_one(SP, NU, m, a); };   // SCL: B^[m][a] is exactly 1
    constexpr int BW = 2 * NX + 2 * NU;              // the quad kernel's bounds pack, one lane per instance: [N][xmin xmax umin umax]
    static_assert(L::NLOADS <= 4, "coefficient block too large for SGPRs");

    __shared__ float s_bnd[UBK ? 1 : 2 * NU * (N - 1)];
    __shared__ float s_xb[XB ? 2 * NX * N : 1];                                  // [knot][x_min[NX] x_max[NX]]
    __shared__ double s_cq[REFS == REF_SHARED ? NX * N : 1], s_cr[REFS == REF_SHARED ? NU * (N - 1) : 1], s_cpt[REFS == REF_SHARED ? NX : 1];
    const int tid = threadIdx.x;
    if constexpr (!UBK) {
        for (int i = tid; i < 2 * NU * (N - 1); i += 256) {
            const int k = i / (2 * NU), j = i % (2 * NU);
            s_bnd[i] = P.bounds[k * BW + 2 * NX + j];
        }
    }
    if constexpr (XB)
        for (int i = tid; i < 2 * NX * N; i += 256) s_xb[i] = P.bounds[(i / (2 * NX)) * BW + i % (2 * NX)];
    if constexpr (REFS == REF_SHARED) {
        // -(Xref .* Q~) / (-rho), -(Uref .* R~) / (-rho), (Xref_{N-1}' Pinf)' / rho  (admm.cpp:77-82 on the scaled recursion)
        const float *qd = P.bounds + N * BW, *rd = qd + NX;                      // diag(Q) + rho, diag(R) + rho behind the bounds
        const double irho = 1.0 / P.rho_family;
        for (int i = tid; i < NU * (N - 1); i += 256) s_cr[i] = (double)P.uref[i] * (double)rd[i % NU] * irho;
        if constexpr (HB) {   // the state terms in the sweeps' coordinates: T' (Q~ xref_k / rho), T' (Pinf' xref_{N-1} / rho)
            const double *T = P.lean + L::O_T;
            for (int k = tid; k < N; k += 256) {
                double c[NX];
                for (int j = 0; j < NX; ++j) c[j] = (double)P.xref[k * NX + j] * (double)qd[j] * irho;
                for (int m = 0; m < NX; ++m) {
                    double acc = 0.0;
                    for (int j = 0; j < NX; ++j) acc = fma(T[j * NX + m], c[j], acc);
                    s_cq[k * NX + m] = acc;
                }
            }
            if (tid == 0) {
                double c[NX];
                for (int i = 0; i < NX; ++i) {
                    double acc = 0.0;
                    for (int j = 0; j < NX; ++j) acc = fma(P.lean[L::O_P + j * NX + i], (double)P.xref[(N - 1) * NX + j], acc);
                    c[i] = acc * irho;
                }
                for (int m = 0; m < NX; ++m) {
                    double acc = 0.0;
                    for (int j = 0; j < NX; ++j) acc = fma(T[j * NX + m], c[j], acc);
                    s_cpt[m] = acc;
                }
            }
        } else {
            for (int i = tid; i < NX * N; i += 256) s_cq[i] = (double)P.xref[i] * (double)qd[i % NX] * irho;
            if (tid < NX) {
                double acc = 0.0;
                for (int j = 0; j < NX; ++j) acc = fma(P.lean[L::O_P + j * NX + tid], (double)P.xref[(N - 1) * NX + j], acc);
                s_cpt[tid] = acc * irho;
            }
        }
    }
    __shared__ double s_T[HB ? NX * NX : 1];                                    // HB: T, for the residual iteration and the store
    if constexpr (HB)
        if (tid < NX * NX) s_T[tid] = P.lean[L::O_T + tid];
    if constexpr (!UBK || XB || REFS == REF_SHARED || HB) __syncthreads();
    const long b = (long)blockIdx.x * 256 + tid;     // (no index list: the solver sends compacted / chunked solves to the quad kernel)
    const bool active = b < P.batch;
    const int lane = tid & 63;
    // staging of a wavefront's solution for the final store (below): the wide form's [64 instances][W (+ 4) floats] / flat
    // [64][nu (N-1)] where the shape takes it (nx N a multiple of 4), else [64][16 + 1 floats] / [64][nu (N-1) | 1]
    constexpr int SW = !TMPC_LEAN_WIDE_STORE ? 0 : (TMPC_LEAN_STORE_W ? TMPC_LEAN_STORE_W : wide_stage_width(EX));
    static_assert(SW == 0 || (SW % 4 == 0 && EX % SW == 0), "wide store: W a multiple of 4 that divides nx N");
    constexpr int STAGE = SW ? wave_stage_floats_wide(EU, SW) : wave_stage_floats(EU);
    // (the wide image is held to 48 KiB by wide_stage_width; the predicated controls' [64][nu (N-1) | 1] may exceed it at long
    // horizons, as it always could: the workgroup's 64 KiB of static LDS is the compiler's to check)
    static_assert(SW == 0 || 4 * 64 * wide_stage_stride(SW) * sizeof(float) <= 48 * 1024, "wide store: staging beyond its 48 KiB");
    __shared__ __attribute__((aligned(16))) float s_stage[4][STAGE];
    // WS, LIVE: the previous iteration's v and z of every lane (rows of an odd number of float4, written 16 bytes at a time —
    // park_v — / of an odd number of floats, written 4 bytes at a time: conflict-free both)
    constexpr bool PARK = WS && LIVE;
    constexpr int PVS = lean_park_stride(EX), PZS = EU | 1;
    __shared__ __attribute__((aligned(16))) float s_pv[PARK ? 256 * PVS : 4];
    __shared__ float s_pz[PARK ? 256 * PZS : 1];

    const SBlock<double, (SCL ? L::NLOADS_Z : L::NLOADS)> blk(P.lean + (HB ? L::O_H : (SCL ? L::O_Z : (SPR ? L::O_S : 0))));   // (SPR: A where M is)
    const auto cM = blk.at(L::O_M), cK = blk.at(L::O_K), cB = blk.at(L::O_B), cC = blk.at(L::O_C);
    const auto cW = blk.at(SCL ? L::O_W : 0);                                   // SCL: w = s^-2 (FOLD: c s^-2)

    ST lo[NU], hi[NU];
#pragma unroll
    for (int a = 0; a < NU; ++a) lo[a] = (ST)P.bounds[2 * NX + a], hi[a] = (ST)P.bounds[2 * NX + NU + a];

    // ---- the iterated state: x (= v = vnew) in fp64 — or, with an active state bound, the state dual g and q~ = vnew - g in
    // fp32 beside a running x — and input dual / slack / feed-forward in fp32 ----
    double X[XB ? 1 : N][NX];           // XB: X[0] is the plant state x0 only
    ST G[XB ? N : 1][NX], QT[XB ? N : 1][NX];
    ST Y[N - 1][NU], Z[N - 1][NU];
    using DT = std::conditional_t<ONE, double, float>;
    DT D[N - 1][NU];
#pragma unroll
    for (int m = 0; m < NX; ++m) {
        if constexpr (WS) X[0][m] = !active ? 0.0 : (P.x0d ? P.x0d[b * NX + m] : (double)P.x0[b * NX + m]);
        else X[0][m] = active ? (double)P.x0[b * NX + m] : 0.0;
        if constexpr (SCL) X[0][m] *= P.lean[L::O_SC + m];                      // x^_0 = S x0
    }
    if constexpr (HB) {                                                         // x^_0 = T' x0
        double x0[NX];
#pragma unroll
        for (int m = 0; m < NX; ++m) x0[m] = X[0][m];
#pragma unroll
        for (int m = 0; m < NX; ++m) {
            double acc = P.lean[L::O_T + m] * x0[0];
#pragma unroll
            for (int j = 1; j < NX; ++j) acc = fma(P.lean[L::O_T + j * NX + m], x0[j], acc);
            X[0][m] = acc;
        }
    }
#pragma unroll
    for (int k = 1; k < (XB ? 1 : N); ++k)
#pragma unroll
        for (int m = 0; m < NX; ++m) X[k][m] = 0.0;
#pragma unroll
    for (int k = 0; k < (XB ? N : 1); ++k)
#pragma unroll
        for (int m = 0; m < NX; ++m) G[k][m] = (ST)0, QT[k][m] = (ST)0;
#pragma unroll
    for (int k = 0; k < N - 1; ++k)
#pragma unroll
        for (int a = 0; a < NU; ++a) Y[k][a] = (ST)0, Z[k][a] = (ST)0, D[k][a] = (DT)0;
    if constexpr (MPC) {
        // the kept v, z into the lanes' rows: every step, the first included, then starts from the rows and the arrays
        // (lanes without an instance get zeros)
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(active);
        int td = tid;
        asm volatile("" : "+v"(td));
        const int ln = td & 63;
        const long w0 = (long)blockIdx.x * 256 + (td & ~63);
        float *so = s_stage[td >> 6];
        load_wave_x<EX>(so, P.sv + w0 * EX, ln, mask, [&](auto ee, float val) { s_pv[td * PVS + decltype(ee)::value] = val; });
        load_wave_u<EU>(so, P.sz + w0 * EU, ln, mask, [&](auto ee, float val) { s_pz[td * PZS + decltype(ee)::value] = val; });
    }
    if constexpr (WS && !MPC) {
        if (!P.cold_start) {                                                    // go on from the kept workspace (admm.cpp:111-115)
            const unsigned long long mask = __builtin_amdgcn_ballot_w64(active);
            int td = tid;                                                       // (opaque, as at the stores: nothing of the
            asm volatile("" : "+v"(td));                                        // loads' addressing stays live across the loop)
            const int ln = td & 63;
            const long w0 = (long)blockIdx.x * 256 + (td & ~63);
            float *so = s_stage[td >> 6];
            if (mask) {
                if constexpr (XB) {
                    load_wave_x<EX>(so, P.sg + w0 * EX, ln, mask, [&](auto ee, float val) { constexpr int e = decltype(ee)::value; G[e / NX][e % NX] = val; });
                    load_wave_x<EX>(so, P.sv + w0 * EX, ln, mask, [&](auto ee, float val) { constexpr int e = decltype(ee)::value; QT[e / NX][e % NX] = val - G[e / NX][e % NX]; });
                } else {   // v is the trajectory; knot 0 is the new x0 (the kept v_0 is read where it matters: forward)
                    load_wave_x<EX>(so, P.sv + w0 * EX, ln, mask, [&](auto ee, float val) { constexpr int e = decltype(ee)::value; if constexpr (e >= NX) X[e / NX][e % NX] = (double)val; });
                    if constexpr (HB) {                                         // x^_k = T' v_k
#pragma unroll
                        for (int k = 1; k < N; ++k) {
                            double vk[NX];
#pragma unroll
                            for (int m = 0; m < NX; ++m) vk[m] = X[k][m];
#pragma unroll
                            for (int m = 0; m < NX; ++m) {
                                double acc = P.lean[L::O_T + m] * vk[0];
#pragma unroll
                                for (int j = 1; j < NX; ++j) acc = fma(P.lean[L::O_T + j * NX + m], vk[j], acc);
                                X[k][m] = acc;
                            }
                        }
                    }
                }
                load_wave_u<EU>(so, P.sy + w0 * EU, ln, mask, [&](auto ee, float val) { constexpr int e = decltype(ee)::value; Y[e / NU][e % NU] = val; });
                load_wave_u<EU>(so, P.sz + w0 * EU, ln, mask, [&](auto ee, float val) { constexpr int e = decltype(ee)::value; Z[e / NU][e % NU] = val; });
                load_wave_u<EU>(so, P.sd + w0 * EU, ln, mask, [&](auto ee, float val) { constexpr int e = decltype(ee)::value; D[e / NU][e % NU] = (DT)val; });
            }
        }
    }

#ifdef TMPC_LEAN_CLOCK_PROBE
    const unsigned long long probe_t0 = __builtin_amdgcn_s_memtime(), probe_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    int it = 0, conv = 0;
    ST res0 = 0, res1 = 0, res2 = 0, res3 = 0;
    const int ct = P.check_termination;
    const int last_check_it = ct > 0 ? (P.max_iter / ct) * ct : 0;
    const ST rho = F64 ? (ST)P.rho_family : (ST)P.rho;
    const ST ptol = F64 ? (ST)P.abs_pri_tol64 : (ST)P.abs_pri_tol, dtol = F64 ? (ST)P.abs_dua_tol64 : (ST)P.abs_dua_tol;
    double dua_x = 0.0;
    double dua_xs[SCL ? NX : 1] = {};                                           // SCL: max_k |x^_prev - x^_new| per component
    ST pri_u = 0, dua_u = 0, pri_xf = 0, dua_xf = 0;                             // (XB: the state residuals in the slack's own type)
    // PARK: knot k's previous state slack into the lane's row — whole float4 where nx allows (16-byte writes at a row stride of
    // an odd number of float4: conflict-free), written as such rather than left to the compiler to merge
    auto park_v = [&](int k, const float (&pv)[NX]) {
        float *row = s_pv + tid * PVS + k * NX;
        if constexpr (NX % 4 == 0) {
#pragma unroll
            for (int q = 0; q < NX / 4; ++q)
                *reinterpret_cast<float4 *>(row + 4 * q) = make_float4(pv[4 * q], pv[4 * q + 1], pv[4 * q + 2], pv[4 * q + 3]);
        } else {
#pragma unroll
            for (int m = 0; m < NX; ++m) row[m] = pv[m];
        }
    };
    // XB: knot k's state slack / dual from the rollout's x_k  (admm.cpp:46, 55-58, 68; q~ for :79-80)
    auto state_sets = [&](auto res_tag, auto kk, const double (&x)[NX]) {
        constexpr bool RES = decltype(res_tag)::value;
        constexpr int k = decltype(kk)::value;
#pragma unroll
        for (int m = 0; m < NX; ++m) {
            const ST xf = (ST)x[m];
            const ST t = xf + G[k][m];                                          // vnew = x + g
            const ST vn = clamp3(t, (ST)s_xb[k * 2 * NX + m], (ST)s_xb[k * 2 * NX + NX + m]);
            const ST gn = t - vn;                                               // g = g + x - vnew
            // PARK: the previous v, kept for a converged exit (element by element here: gathered into a float4 of its own the
            // four values cost this form 12 parked registers; the compiler merges a knot's four writes — tests/test_lean_ws_asm.py)
            if constexpr (RES && PARK) {
                if constexpr (MPC) {                                            // (a converged lane's row stays its exit's)
                    if (!conv) s_pv[tid * PVS + k * NX + m] = (float)(QT[k][m] + G[k][m]);
                } else {
                    s_pv[tid * PVS + k * NX + m] = (float)(QT[k][m] + G[k][m]);
                }
            }
            if constexpr (RES) {
                pri_xf = lean_max(pri_xf, lean_abs(xf - vn));
                dua_xf = lean_max(dua_xf, lean_abs((QT[k][m] + G[k][m]) - vn)); // v = the previous vnew = q~ + g
            }
            G[k][m] = gn;
            QT[k][m] = vn - gn;
        }
    };

    // HB: element m of x = T x^, in fp64.  T comes from LDS (s_T) through an opaque pointer at each use (a knot of the
    // residual iteration, the store): left alone the compiler keeps its 16 values live across the whole solve
    auto load_T = [&](double (&Tm)[NX * NX]) {
        const double *tp = s_T;
        asm volatile("" : "+v"(tp));
#pragma unroll
        for (int i = 0; i < NX * NX; ++i) Tm[i] = tp[i];
    };
    auto to_x = [](const double (&Tm)[NX * NX], const double (&xh)[NX], int m) {
        double acc = Tm[m * NX] * xh[0];
#pragma unroll
        for (int j = 1; j < NX; ++j) acc = fma(Tm[m * NX + j], xh[j], acc);
        return acc;
    };

    // ================= fused forward sweep: forward_pass (admm.cpp:25-35) + update_slack (:43-59) + update_dual (:65-69)
    // (+ RES: the residual maxima of termination_condition, :93-96) =================
    auto forward = [&](auto res_tag, bool first_iter) {
        constexpr bool RES = decltype(res_tag)::value;
        if constexpr (RES) {
            dua_x = 0.0, pri_u = 0, dua_u = 0, pri_xf = 0, dua_xf = 0;
            if constexpr (SCL)
#pragma unroll
                for (int m = 0; m < NX; ++m) dua_xs[m] = 0.0;
            if constexpr (WS && !XB) {
                // knot 0: vnew is x0; the previous slack is the workspace's v_0 in the first iteration (zero when cold) and
                // x0 after any iteration (admm.cpp:94)
                float v0p[NX];
#pragma unroll
                for (int m = 0; m < NX; ++m) v0p[m] = (float)X[0][m];          // (parked by the LIVE kernels only, which are never HB)
                if (first_iter) {
                    // (the instance's index opaque here: the address of its v_0 is then formed in this branch, not ahead of the
                    // iteration loop and kept across it)
                    int td = tid;
                    asm volatile("" : "+v"(td));
                    const long bb = (long)blockIdx.x * 256 + td;
                    const bool warm0 = bb < P.batch && !P.cold_start;
                    double x0v[NX];
                    if constexpr (HB) {
                        double Tm[NX * NX];                                   // (T from the pack, once per solve at most)
#pragma unroll
                        for (int i = 0; i < NX * NX; ++i) Tm[i] = P.lean[L::O_T + i];
#pragma unroll
                        for (int m = 0; m < NX; ++m) x0v[m] = to_x(Tm, X[0], m);
                    } else {
#pragma unroll
                        for (int m = 0; m < NX; ++m) x0v[m] = X[0][m];
                    }
#pragma unroll
                    for (int m = 0; m < NX; ++m) {
                        if constexpr (MPC) v0p[m] = s_pv[td * PVS + m];      // (the lane's row: the v_0 of its last exit)
                        else v0p[m] = warm0 ? P.sv[bb * EX + m] : 0.f;
                        dua_x = fmax(dua_x, fabs((double)v0p[m] - x0v[m]));
                    }
                }
                if constexpr (PARK) {
                    if constexpr (MPC) {
                        if (!conv) park_v(0, v0p);
                    } else {
                        park_v(0, v0p);
                    }
                }
            }
            if constexpr (!WS && !XB)
                if (first_iter) {   // cold start: the previous state slack is the zero workspace at knot 0 too, where vnew is x0 (admm.cpp:94)
#pragma unroll
                    for (int m = 0; m < NX; ++m) {
                        if constexpr (HB) {
                            double Tm[NX * NX];
                            load_T(Tm);
                            dua_x = fmax(dua_x, fabs(to_x(Tm, X[0], m)));
                        } else if constexpr (SCL) {                             // (|x0| once the component's scale is taken out, below)
                            dua_xs[m] = fabs(X[0][m]);
                        } else {
                            dua_x = fmax(dua_x, fabs(X[0][m]));
                        }
                    }
                }
        }
        // HB: x^_0 is loop-invariant, and so are the products of its band rows that no b^ term starts: hoisted out of the
        // iteration loop they would stay live across it (18 registers for cartpole; SPR: A x_0 likewise — except in the
        // 256-register form without a state bound, which spills 33 registers with the opaque use and none without)
        // (SCL in the 512-register form: 290 of 512 registers, the products leave the loop)
        if constexpr (HB || (SPR && (ONE || XB) && !(SCL && ONE)))
#pragma unroll
            for (int m = 0; m < NX; ++m) asm volatile("" : "+v"(X[0][m]));
        double xr[NX];                                                          // XB: the running x_k
#pragma unroll
        for (int m = 0; m < NX; ++m) xr[m] = X[0][m];
        float upk[PK ? NU : 1];                                                 // PK: the even knot's (float)u, until its partner
        sfor<0, N - 1>([&](auto kk) {
            constexpr int k = decltype(kk)::value;
            constexpr int kx = XB ? 0 : k;                                      // where x_k lives: the running vector, or the trajectory
            if constexpr (!UBK || XB) asm volatile("" ::: "memory");   // per-knot bounds are re-read from LDS at their knot, not hoisted out of the solve
            if constexpr (XB) state_sets(res_tag, kk, xr);
            const double (&xk)[NX] = XB ? xr : X[kx];
            double dk[NU], u[NU], xn[NX];
#pragma unroll
            for (int a = 0; a < NU; ++a) dk[a] = (double)D[k][a];
            // x+ = (A - B Kinf) x - B d: NX independent chains, none waits for u (HB: the chains start at their band)
            bool started[NX];
            if constexpr (!SPR) {
#pragma unroll
                for (int m = 0; m < NX; ++m) {
                    started[m] = false;
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        if (bh_zero(m, a)) continue;
                        xn[m] = started[m] ? fma(-cB[m * NU + a], dk[a], xn[m]) : -(cB[m * NU + a] * dk[a]);
                        started[m] = true;
                    }
                }
#pragma unroll
                for (int j = 0; j < NX; ++j)
#pragma unroll
                    for (int m = 0; m < NX; ++m) {
                        if (mh_zero(m, j)) continue;
                        xn[m] = started[m] ? fma(cM[m * NX + j], xk[j], xn[m]) : cM[m * NX + j] * xk[j];
                        started[m] = true;
                    }
            }
            // u = -Kinf x - d  (SPR: x_k's rows without a B term first — the others wait for the previous knot's u)
            // SCL, 512 registers, knot 0: x^_0 does not change over the iterations, so the chains are grouped with its terms
            // first — u_0 = (-K^ x^_0) - d_0, a row A^ x^_0 before its u terms — and those groups leave the iteration loop
            constexpr bool K0H = SCL && ONE && k == 0;
#pragma unroll
            for (int a = 0; a < NU; ++a) {
                if constexpr (K0H) {
                    double acc = -(cK[a * NX] * xk[0]);
#pragma unroll
                    for (int j = 1; j < NX; ++j) acc = fma(-cK[a * NX + j], xk[j], acc);
                    u[a] = acc - dk[a];
                } else if constexpr (SPR) {
                    double acc = -dk[a];
#pragma unroll
                    for (int pass = 0; pass < 2; ++pass)
#pragma unroll
                        for (int j = 0; j < NX; ++j) {
                            bool late = false;
#pragma unroll
                            for (int c = 0; c < NU; ++c) late = late || b_nz(j, c);
                            if (late == (pass == 1)) acc = fma(-cK[a * NX + j], xk[j], acc);
                        }
                    u[a] = acc;
                } else if constexpr (TMPC_LEAN_SPLITK && NX >= 4) {
                    double u0 = -dk[a], u1 = -(cK[a * NX + NX / 2] * xk[NX / 2]);
#pragma unroll
                    for (int j = 0; j < NX / 2; ++j) u0 = fma(-cK[a * NX + j], xk[j], u0);
#pragma unroll
                    for (int j = NX / 2 + 1; j < NX; ++j) u1 = fma(-cK[a * NX + j], xk[j], u1);
                    u[a] = u0 + u1;
                } else {
                    double acc = -dk[a];
#pragma unroll
                    for (int j = 0; j < NX; ++j) acc = fma(-cK[a * NX + j], xk[j], acc);
                    u[a] = acc;
                }
            }
            if constexpr (SPR) {   // x+ = A x + B u: a row's chain starts from x_j at its first unit; the u terms last
#pragma unroll
                for (int m = 0; m < NX; ++m) {
                    int s = -1, sb = -1;
#pragma unroll
                    for (int j = NX - 1; j >= 0; --j)
                        if (a_one(m, j)) s = j;
#pragma unroll
                    for (int a = NU - 1; a >= 0; --a)                           // SCL: ... or, without one, from u_a at B^'s unit
                        if (s < 0 && b_one(m, a) && !K0H) sb = a;
                    started[m] = s >= 0 || sb >= 0;
                    xn[m] = 0.0;                                                // (a row without terms)
                    if (s >= 0) xn[m] = xk[s];
                    else if (sb >= 0) xn[m] = u[sb];
#pragma unroll
                    for (int j = 0; j < NX; ++j) {
                        if (!a_nz(m, j) || j == s) continue;
                        xn[m] = !started[m] ? cM[m * NX + j] * xk[j] : (a_one(m, j) ? xn[m] + xk[j] : fma(cM[m * NX + j], xk[j], xn[m]));
                        started[m] = true;
                    }
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        if (!b_nz(m, a) || a == sb) continue;
                        xn[m] = !started[m] ? cB[m * NU + a] * u[a] : (b_one(m, a) ? xn[m] + u[a] : fma(cB[m * NU + a], u[a], xn[m]));
                        started[m] = true;
                    }
                }
            }
            constexpr bool PK_ODD = PK && !RES && (k & 1), PK_EVEN = PK && !RES && !(k & 1) && k + 1 < N - 1;
            if constexpr (PK_EVEN) {
#pragma unroll
                for (int a = 0; a < NU; ++a) upk[a] = (float)u[a];
            }
            if constexpr (PK_ODD) {                                             // knots k - 1 and k: admm.cpp:45, :50-52, :67
#pragma unroll
                for (int a = 0; a < NU; ++a) {
                    const lean_f2 t = lean_f2{upk[a], (float)u[a]} + lean_f2{(float)Y[k - 1][a], (float)Y[k][a]};
                    const lean_f2 zn = {clamp3(t.x, (float)lo[a], (float)hi[a]), clamp3(t.y, (float)lo[a], (float)hi[a])};
                    const lean_f2 yn = t - zn;
                    Y[k - 1][a] = yn.x, Y[k][a] = yn.y;
                    Z[k - 1][a] = zn.x, Z[k][a] = zn.y;
                }
            }
            if constexpr (!PK_ODD && !PK_EVEN)
#pragma unroll
            for (int a = 0; a < NU; ++a) {
                const ST uf = (ST)u[a];
                const ST t = uf + Y[k][a];                                      // znew = u + y  (admm.cpp:45)
                ST l_ = lo[a], h_ = hi[a];
                if constexpr (!UBK) l_ = (ST)s_bnd[k * 2 * NU + a], h_ = (ST)s_bnd[k * 2 * NU + NU + a];
                const ST zn = clamp3(t, l_, h_);                                //   clamped to [u_min, u_max]  (:50-52)
                Y[k][a] = t - zn;                                               // y = y + u - znew  (:67)
                if constexpr (RES) {
                    pri_u = lean_max(pri_u, lean_abs(uf - zn));                 // (:95)
                    dua_u = lean_max(dua_u, lean_abs(Z[k][a] - zn));            // (:96), times rho at the check
                    if constexpr (PARK) {
                        if constexpr (MPC) {
                            if (!conv) s_pz[tid * PZS + k * NU + a] = (float)Z[k][a];
                        } else {
                            s_pz[tid * PZS + k * NU + a] = (float)Z[k][a];
                        }
                    }
                }
                Z[k][a] = zn;
            }
            if constexpr (RES && PARK && !XB) {                                 // the previous v of knot k + 1, before it is overwritten
                float pv[NX];
#pragma unroll
                for (int m = 0; m < NX; ++m) pv[m] = (float)X[k + 1][m];
                if constexpr (MPC) {
                    if (!conv) park_v(k + 1, pv);
                } else {
                    park_v(k + 1, pv);
                }
            }
#pragma unroll
            for (int m = 0; m < NX; ++m) {
                if constexpr (XB) {
                    xr[m] = xn[m];
                } else {
                    if constexpr (RES && SCL) dua_xs[m] = fmax(dua_xs[m], fabs(X[k + 1][m] - xn[m]));
                    else if constexpr (RES && !HB) dua_x = fmax(dua_x, fabs(X[k + 1][m] - xn[m]));   // v - vnew with v = the previous x  (:94)
                    if constexpr (!(RES && HB)) X[k + 1][m] = xn[m];
                }
            }
            if constexpr (RES && HB) {                                          // ... in the original coordinates: T (x^_prev - x^_new)
                double dl[NX], Tm[NX * NX];
                load_T(Tm);                                                     // (per knot: live for these 16 FMAs only)
#pragma unroll
                for (int m = 0; m < NX; ++m) dl[m] = X[k + 1][m] - xn[m], X[k + 1][m] = xn[m];
#pragma unroll
                for (int m = 0; m < NX; ++m) dua_x = fmax(dua_x, fabs(to_x(Tm, dl, m)));
            }
            // (the residual maxima are only read under `!conv`: left alone, the compiler sinks the whole chain into that
            // branch, behind the sweep, and keeps every knot's u, znew and previous x alive for it — 190 spilled registers)
            if constexpr (RES) asm volatile("" : "+v"(pri_u), "+v"(dua_u), "+v"(dua_x), "+v"(pri_xf), "+v"(dua_xf));
            if constexpr (RES && SCL)
#pragma unroll
                for (int m = 0; m < NX; ++m) asm volatile("" : "+v"(dua_xs[m]));
            if constexpr (TMPC_LEAN_KNOT_BARRIER) __builtin_amdgcn_sched_barrier(0);
        });
        if constexpr (RES && SCL) {                                             // the state dual residual in the original coordinates
#pragma unroll
            for (int m = 0; m < NX; ++m) dua_x = fmax(dua_x, dua_xs[m] * fabs(P.lean[L::O_SI + m]));
            asm volatile("" : "+v"(dua_x));
        }
        if constexpr (XB) {
            asm volatile("" ::: "memory");
            state_sets(res_tag, std::integral_constant<int, N - 1>{}, xr);      // the terminal knot's slack / dual
            if constexpr (RES) asm volatile("" : "+v"(pri_xf), "+v"(dua_xf));
        }
    };

    // ================= fused backward sweep: update_linear_cost (admm.cpp:75-83) + backward_pass_grad (:13-20), scaled by
    // -1 / rho; q, r, p never stored =================
    auto backward = [&]() {
        double p[NX];
        if constexpr (REFS == REF_SHARED) asm volatile("" ::: "memory");        // (reference terms: read from LDS where used)
#pragma unroll
        for (int m = 0; m < NX; ++m) {                                          // p~_{N-1} = vnew_{N-1} - g_{N-1} (+ Pinf' xref / rho)  (:81-82)
            p[m] = XB ? (double)QT[N - 1][m] : X[XB ? 0 : N - 1][m];
            if constexpr (SCL) p[m] *= cW[m];                                   // p^_{N-1} = W x^_{N-1}
            if constexpr (REFS == REF_SHARED) p[m] += s_cpt[m];
        }
        float rpk[PK ? NU : 1];                                                 // PK: the even knot's r~, formed with its partner's
        sfor<0, N - 1>([&](auto kk) {
            constexpr int k = N - 2 - decltype(kk)::value;
            double r[NU], t[NU];
            if constexpr (REFS == REF_SHARED) asm volatile("" ::: "memory");
#pragma unroll
            for (int a = 0; a < NU; ++a) {
                if constexpr (PK && (k & 1)) {                                  // r~ of knots k - 1 and k
                    const lean_f2 rp = lean_f2{(float)Z[k - 1][a], (float)Z[k][a]} - lean_f2{(float)Y[k - 1][a], (float)Y[k][a]};
                    rpk[a] = rp.x;
                    r[a] = (double)rp.y;
                } else if constexpr (PK && k + 1 < N - 1) {
                    r[a] = (double)rpk[a];
                } else
                r[a] = (double)(Z[k][a] - Y[k][a]);                             // r~ = znew - y  (:77-78)
                if constexpr (REFS == REF_SHARED) r[a] += s_cr[k * NU + a];     //      + R~ uref / rho
                t[a] = r[a];
            }
            if constexpr (FOLD) {
                // d_k = c r~_k + B^' pv_{k+1}, two operations for cartpole.  r~_k has been in registers since the forward
                // sweep and every pv_{k+1}[j] ends in the product by d_{k+1}, so the costates are what the chain waits for:
                // the one at B^'s unit enters first, as the addend of the product c r~ — fma(c, r~, pv_j), nothing is
                // multiplied by C afterwards — and the one with a coefficient of its own enters LAST (cartpole: pv_3 then
                // B^_1 pv_1; the other order, fma(c, r~, fma(B^_1, pv_1, pv_3)), needs both costates at its first operation)
                bool begun = false;
#pragma unroll
                for (int j = 0; j < NX; ++j)
                    if (b_nz(j, 0) && b_one(j, 0)) t[0] = fma(cC[0], r[0], p[j]), begun = true;
                if (!begun) t[0] = cC[0] * r[0];
#pragma unroll
                for (int j = 0; j < NX; ++j)
                    if (b_nz(j, 0) && !b_one(j, 0)) t[0] = fma(cB[j * NU], p[j], t[0]);
                D[k][0] = (DT)t[0];                                             // (t is d from here on: K^' d = c K^' t below)
            } else {
#pragma unroll
            for (int j = 0; j < NX; ++j)
#pragma unroll
                for (int a = 0; a < NU; ++a)
                    if (!bh_zero(j, a) && b_nz(j, a)) t[a] = b_one(j, a) ? t[a] + p[j] : fma(cB[j * NU + a], p[j], t[a]);   // B' p~_{k+1} + r~_k
#pragma unroll
            for (int a = 0; a < NU; ++a) {                                      // d_k = Quu_inv (B' p_{k+1} + r_k)  (:17)
                double acc = cC[a * NU] * t[0];
#pragma unroll
                for (int c = 1; c < NU; ++c) acc = fma(cC[a * NU + c], t[c], acc);
                D[k][a] = (DT)acc;
            }
            }
            if constexpr (k > 0 && SPR) {                                       // p~_k = q~_k + A' p~_{k+1} - Kinf' t_k
                double ap[NX];
#pragma unroll
                for (int m = 0; m < NX; ++m) {
                    double acc = XB ? (double)QT[k][m] : X[XB ? 0 : k][m];
                    if constexpr (REFS == REF_SHARED) acc += s_cq[k * NX + m];
                    int ju = -1;                                                // SCL: the column starts fma(w_m, x^_m, p^_j) at its first unit
                    if constexpr (SCL) {
#pragma unroll
                        for (int j = NX - 1; j >= 0; --j)
                            if (a_one(j, m)) ju = j;
                        acc = ju >= 0 ? fma(cW[m], acc, p[ju]) : cW[m] * acc;
                    }
#pragma unroll
                    for (int j = 0; j < NX; ++j)
                        if (a_nz(j, m) && j != ju) acc = a_one(j, m) ? acc + p[j] : fma(cM[j * NX + m], p[j], acc);
#pragma unroll
                    for (int a = 0; a < NU; ++a) acc = fma(-cK[a * NX + m], t[a], acc);
                    ap[m] = acc;
                }
#pragma unroll
                for (int m = 0; m < NX; ++m) p[m] = ap[m];
            } else if constexpr (k > 0) {                                       // (p_0 is never read)
                double ap[NX];
#pragma unroll
                for (int m = 0; m < NX; ++m) {                                  // q~_k - Kinf' r~_k
                    double acc = XB ? (double)QT[k][m] : X[XB ? 0 : k][m];     // q~_k = vnew_k - g_k  (:79-80)
                    if constexpr (REFS == REF_SHARED) acc += s_cq[k * NX + m];  //      + Q~ xref / rho
#pragma unroll
                    for (int a = 0; a < NU; ++a) acc = fma(-cK[a * NX + m], r[a], acc);
                    ap[m] = acc;
                }
#pragma unroll
                for (int j = 0; j < NX; ++j)
#pragma unroll
                    for (int m = 0; m < NX; ++m)
                        if (!mh_zero(j, m)) ap[m] = fma(cM[j * NX + m], p[j], ap[m]);   // + AmBKt p~_{k+1}  (:18)
#pragma unroll
                for (int m = 0; m < NX; ++m) p[m] = ap[m];
            }
            if constexpr (TMPC_LEAN_KNOT_BARRIER) __builtin_amdgcn_sched_barrier(0);
        });
    };

    // solution = projected slack of the iteration (admm.cpp:187-188, :204-205); status of the instance.  This direct form
    // (every lane its own instance: scattered 16-byte pieces) serves the instances that converge inside the loop, a few at
    // a time; the final store below goes through LDS
    // element (k, m) of the solution: the state slack vnew — x itself, or q~ + g brought back inside the bounds it was clamped
    // to (fp32 rounding of the sum can leave them by an ulp)
    double Ts[HB ? NX * NX : 1];                                               // HB: T, loaded at the final store
    double Si[SCL ? NX : 1];                                                    // SCL: 1 / s, loaded at each store
    auto load_Si = [&]() {   // (through an opaque pointer: the four values are not kept across the iteration loop)
        const double *sp = P.lean + L::O_SI;
        asm volatile("" : "+s"(sp));
#pragma unroll
        for (int m = 0; m < (SCL ? NX : 0); ++m) Si[m] = sp[m];
    };
    auto vnew_at = [&](auto kk, auto mm) -> float {
        constexpr int k = decltype(kk)::value, m = decltype(mm)::value;
        if constexpr (XB) return (float)clamp3(QT[k][m] + G[k][m], (ST)s_xb[k * 2 * NX + m], (ST)s_xb[k * 2 * NX + NX + m]);
        else if constexpr (HB) return (float)to_x(Ts, X[k], m);
        else if constexpr (SCL) return (float)(X[k][m] * Si[m]);               // x = S^-1 x^
        else return (float)X[XB ? 0 : k][m];
    };
    auto store = [&](bool solved_flag) {
        // one opaque base address per array, constant offsets behind it: left to itself the compiler forms the 99 store
        // addresses once, outside the iteration loop (the LIVE variant stores inside it), and spills 200 registers for them
        float *xo = P.xout + b * EX, *uo = P.uout + b * EU, *ro = P.res + b * 4;
        asm volatile("" : "+v"(xo), "+v"(uo), "+v"(ro));
        if constexpr (SCL) load_Si();
        sfor<0, N>([&](auto kk) {
            constexpr int k = decltype(kk)::value;
            sfor<0, NX>([&](auto mm) { xo[k * NX + decltype(mm)::value] = vnew_at(kk, mm); });
            __builtin_amdgcn_sched_barrier(0);   // (a knot's conversions next to its stores, not eighty temporaries up front)
        });
#pragma unroll
        for (int k = 0; k < N - 1; ++k)
#pragma unroll
            for (int a = 0; a < NU; ++a) uo[k * NU + a] = (float)Z[k][a];
        P.iter[b] = P.iter_offset + it;
        P.solved[b] = solved_flag ? 1 : 0;
        ro[0] = (float)res0;
        ro[1] = (float)res1;
        ro[2] = (float)res2;
        ro[3] = (float)res3;
    };

    // WS: solution, workspace and status of the lanes in `mask`, through the wavefront's staging.  CV: a converged exit — the
    // workspace's v, z are the parked previous ones and d is the previous backward pass's; otherwise (exit at max_iter) v, z
    // are the solution's and d is the backward pass's behind the last iteration (admm.cpp:195-205)
    auto store_ws = [&](unsigned long long mask, bool mine, auto conv_tag) {
        constexpr bool CV = decltype(conv_tag)::value;
        // (the lane's index opaque at each use of the store: left alone the compiler forms every store address once, outside
        // the iteration loop — the converged exit stores inside it — and spills a hundred registers for them)
        int td = tid;
        asm volatile("" : "+v"(td));
        const int ln = td & 63;
        const long bb = (long)blockIdx.x * 256 + td;
        float *so = s_stage[td >> 6];
        const long w0 = (long)blockIdx.x * 256 + (td & ~63);
        auto pair = [&](float *xo, float *uo, auto &&gx, auto &&gu) {
            if constexpr (SW != 0) store_wave_wide<EX, EU, SW>(so, xo, uo, ln, mask, gx, gu);
            else store_wave_coalesced<EX, EU>(so, xo, uo, ln, mask, gx, gu);
        };
        auto single = [&](float *uo, auto &&gu) {
            if constexpr (SW != 0) {
                if (mask == ~0ull) store_wave_u_wide<EU>(so, uo, ln, gu);
                else store_wave_u<EU, false>(so, uo, ln, mask, gu);
            } else {
                store_wave_u<EU, false>(so, uo, ln, mask, gu);
            }
        };
        auto getx = [&](auto ee) { constexpr int e = decltype(ee)::value; return vnew_at(std::integral_constant<int, e / NX>{}, std::integral_constant<int, e % NX>{}); };
        auto getu = [&](auto ee) { constexpr int e = decltype(ee)::value; return (float)Z[e / NU][e % NU]; };
        auto gety = [&](auto ee) { constexpr int e = decltype(ee)::value; return (float)Y[e / NU][e % NU]; };
        auto getd = [&](auto ee) { constexpr int e = decltype(ee)::value; return (float)D[e / NU][e % NU]; };
        pair(P.xout + w0 * EX, P.uout + w0 * EU, getx, getu);
        if (P.save_state) {
            if constexpr (CV) {
                pair(P.sv + w0 * EX, P.sz + w0 * EU, [&](auto ee) { return s_pv[td * PVS + decltype(ee)::value]; },
                     [&](auto ee) { return s_pz[td * PZS + decltype(ee)::value]; });
            } else {
                pair(P.sv + w0 * EX, P.sz + w0 * EU, getx, getu);
            }
            if constexpr (XB) pair(P.sg + w0 * EX, P.sy + w0 * EU, [&](auto ee) { constexpr int e = decltype(ee)::value; return (float)G[e / NX][e % NX]; }, gety);
            else single(P.sy + w0 * EU, gety);
            single(P.sd + w0 * EU, getd);
        }
        if (mine) {
            float *ro = P.res + bb * 4;
            P.iter[bb] = P.iter_offset + it;
            P.solved[bb] = CV ? 1 : 0;
            ro[0] = (float)res0, ro[1] = (float)res1, ro[2] = (float)res2, ro[3] = (float)res3;
        }
    };

    // Iterations whose termination check can matter carry the residual arithmetic (every check when the tolerances are
    // positive; otherwise nobody can converge and only the last check's values are ever reported); all others run in a
    // tight loop of their own, so that the two forms of the forward sweep never meet at a join (a join costs a copy per
    // loop-carried register and lets the compiler hoist their common parts above the branch, live across everything).
    const bool can_converge = P.abs_pri_tol > 0.f && P.abs_dua_tol > 0.f;
    const int max_iter = P.max_iter;
    // MPC, a step before the last: y, d (and g) of the lanes in `mask` to the workspace arrays, through the staging
    auto store_step = [&](unsigned long long mask) {
        int td = tid;
        asm volatile("" : "+v"(td));
        const int ln = td & 63;
        float *so = s_stage[td >> 6];
        const long w0 = (long)blockIdx.x * 256 + (td & ~63);
        auto single = [&](float *uo, auto &&gu) {
            if constexpr (SW != 0) {
                if (mask == ~0ull) store_wave_u_wide<EU>(so, uo, ln, gu);
                else store_wave_u<EU, false>(so, uo, ln, mask, gu);
            } else {
                store_wave_u<EU, false>(so, uo, ln, mask, gu);
            }
        };
        auto gety = [&](auto ee) { constexpr int e = decltype(ee)::value; return (float)Y[e / NU][e % NU]; };
        auto getd = [&](auto ee) { constexpr int e = decltype(ee)::value; return (float)D[e / NU][e % NU]; };
        if constexpr (XB) {
            auto getg = [&](auto ee) { constexpr int e = decltype(ee)::value; return (float)G[e / NX][e % NX]; };
            if constexpr (SW != 0) store_wave_wide<EX, EU, SW>(so, P.sg + w0 * EX, P.sy + w0 * EU, ln, mask, getg, gety);
            else store_wave_coalesced<EX, EU>(so, P.sg + w0 * EX, P.sy + w0 * EU, ln, mask, getg, gety);
        } else {
            single(P.sy + w0 * EU, gety);
        }
        single(P.sd + w0 * EU, getd);
    };
    // MPC: the plant step behind a solve and its log (plant_step_kernel, solver.hip: the same operations in the same order);
    // u0: the control the lane's exit left
    float u0c[MPC ? NU : 1];
    auto plant = [&](int step, bool final_step) {
        const double *ab = P.lean + L::O_S;                                     // the model's own A [nx][nx], B [nx][nu], row-major
        double xn[NX];
#pragma unroll
        for (int r = 0; r < NX; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < NX; ++j) acc = fma(ab[L::O_M + r * NX + j], X[0][j], acc);
#pragma unroll
            for (int a = 0; a < NU; ++a) acc = fma(ab[L::O_B + r * NU + a], (double)u0c[a], acc);
            xn[r] = acc;
        }
        int td = tid;
        asm volatile("" : "+v"(td));
        const long bb = (long)blockIdx.x * 256 + td;
        if (bb < P.batch) {
            const long so = bb * P.mpc_steps + step;
#pragma unroll
            for (int r = 0; r < NX; ++r) P.mpc_x[so * NX + r] = (float)xn[r];
#pragma unroll
            for (int a = 0; a < NU; ++a) P.mpc_u[so * NU + a] = u0c[a];
            P.mpc_iter[so] = conv ? P.iter_offset + it : -(P.iter_offset + it);
            if (final_step) {
#pragma unroll
                for (int r = 0; r < NX; ++r) P.x0_out[bb * NX + r] = (float)xn[r];
                // (the caller's fp64 plant state, read at entry: the loop's launch owns it, as plant_step_kernel does in the chain)
                if (double *xd = const_cast<double *>(P.x0d)) {
#pragma unroll
                    for (int r = 0; r < NX; ++r) xd[bb * NX + r] = xn[r];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < NX; ++r) X[0][r] = xn[r];
    };
    int step = 0;
#ifdef TMPC_LEAN_CLOCK_PROBE
    // MPC: core clocks of a step's phases, summed over the steps — the reload, the iteration loop, of which the stores at
    // convergence, and the step's end (rows, y / d store, plant step, log, the wait for the stores)
    unsigned long long probe_ph[4] = {0, 0, 0, 0}, probe_a = 0, probe_c = 0;
#endif
    do {   // (MPC: the steps of the closed loop; otherwise once)
#ifdef TMPC_LEAN_CLOCK_PROBE
    probe_a = __builtin_amdgcn_s_memtime();
#endif
    if constexpr (MPC) {
        // the step's start: v, z from the lane's row, y, d (g) from the arrays this wavefront wrote in the step before
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        int td = tid;
        asm volatile("" : "+v"(td));
        const int ln = td & 63;
        const long w0 = (long)blockIdx.x * 256 + (td & ~63);
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(w0 + ln < P.batch);
        float *so = s_stage[td >> 6];
        const float *rv = s_pv + td * PVS, *rz = s_pz + td * PZS;
        if constexpr (XB) {
            load_wave_x<EX>(so, P.sg + w0 * EX, ln, mask, [&](auto ee, float val) { constexpr int e = decltype(ee)::value; G[e / NX][e % NX] = val; });
            sfor<0, EX>([&](auto ee) { constexpr int e = decltype(ee)::value; QT[e / NX][e % NX] = rv[e] - G[e / NX][e % NX]; });
        } else {
            sfor<NX, EX>([&](auto ee) { constexpr int e = decltype(ee)::value; X[e / NX][e % NX] = (double)rv[e]; });
        }
        sfor<0, EU>([&](auto ee) { constexpr int e = decltype(ee)::value; Z[e / NU][e % NU] = rz[e]; });
        load_wave_u<EU>(so, P.sy + w0 * EU, ln, mask, [&](auto ee, float val) { constexpr int e = decltype(ee)::value; Y[e / NU][e % NU] = val; });
        load_wave_u<EU>(so, P.sd + w0 * EU, ln, mask, [&](auto ee, float val) { constexpr int e = decltype(ee)::value; D[e / NU][e % NU] = (DT)val; });
        it = 0, conv = 0;
        res0 = 0, res1 = 0, res2 = 0, res3 = 0;
    }
    const bool last_step = !MPC || step + 1 >= P.mpc_steps;
#ifdef TMPC_LEAN_CLOCK_PROBE
    probe_ph[0] += __builtin_amdgcn_s_memtime() - probe_a, probe_a = __builtin_amdgcn_s_memtime();
#endif
    int i = 0;
    while (i < max_iter) {
        int next_res = max_iter;                                                // 0-based index of the next iteration with residuals
        if (ct > 0) {
            if (LIVE && can_converge) next_res = (i / ct) * ct + ct - 1;
            else if (last_check_it - 1 >= i) next_res = last_check_it - 1;
        }
        const int n_plain = (next_res < max_iter ? next_res : max_iter) - i;
        for (int j = 0; j < n_plain; ++j) {
            forward(std::false_type{}, false);
            backward();
        }
        i += n_plain;
        if (!LIVE || !conv) it += n_plain;                                      // admm.cpp:143
        if (i >= max_iter) break;
        forward(std::true_type{}, i == 0);
        i += 1;
        if (!LIVE || !conv) {                                                   // termination_condition (admm.cpp:89-107)
            it += 1;
            res0 = XB ? pri_xf : (ST)0;                                         // (no active state bound: x - vnew = 0)
            res1 = (XB ? dua_xf : (ST)dua_x) * rho;
            res2 = pri_u;
            res3 = dua_u * rho;
        }
        if constexpr (LIVE) {
            const bool now = active && !conv && res0 < ptol && res2 < ptol && res1 < dtol && res3 < dtol;
            if constexpr (WS) {                                                 // returns before v = vnew and the backward pass (:181-193)
                const unsigned long long cm = __builtin_amdgcn_ballot_w64(now);
                if constexpr (MPC) {
#ifdef TMPC_LEAN_CLOCK_PROBE
                    probe_c = __builtin_amdgcn_s_memtime();
#endif
                    if (cm) {
                        if (last_step) store_ws(cm, now, std::true_type{});
                        else store_step(cm);                                    // (ahead of the backward pass below: the d of its exit)
                    }
#ifdef TMPC_LEAN_CLOCK_PROBE
                    probe_ph[2] += __builtin_amdgcn_s_memtime() - probe_c;
#endif
                    if (now) {
#pragma unroll
                        for (int a = 0; a < NU; ++a) u0c[a] = (float)Z[0][a];
                    }
                } else
                if (cm) store_ws(cm, now, std::true_type{});
                if (now) conv = 1;
            } else
            if (now) {                                                          // returns before v = vnew and the backward pass (:181-193)
                store(true);
                conv = 1;
            }
            if (!__builtin_amdgcn_ballot_w64(active && !conv)) break;           // every instance of this wavefront finished
        }
        // (after the last iteration its d is never read; the 256-register and state-bounded forms keep the unconditional call:
        // an exit before it costs them 2-50 spilled registers)
        // (WS: a saving solve leaves that d in the workspace, admm.cpp:195-205)
        if (!(ONE && !XB) || WS || i < max_iter) backward();
    }
    if constexpr (MPC) {
#ifdef TMPC_LEAN_CLOCK_PROBE
        probe_ph[1] += __builtin_amdgcn_s_memtime() - probe_a, probe_a = __builtin_amdgcn_s_memtime();
#endif
#pragma unroll
        for (int a = 0; a < NU; ++a)
            if (!conv) u0c[a] = (float)Z[0][a];
        if (last_step) break;                                                   // (the last step's exit at max_iter: the final store below)
        // the lanes that leave at max_iter: vnew, znew into their rows, y, d (g) — the d of the backward pass behind the last
        // iteration — to the arrays (admm.cpp:195-205)
        const bool mine = active && !conv;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(mine);
        if (mask) {
            if (mine) {
                int td = tid;
                asm volatile("" : "+v"(td));
                float *rv = s_pv + td * PVS, *rz = s_pz + td * PZS;
                sfor<0, EX>([&](auto ee) {
                    constexpr int e = decltype(ee)::value;
                    rv[e] = vnew_at(std::integral_constant<int, e / NX>{}, std::integral_constant<int, e % NX>{});
                });
                sfor<0, EU>([&](auto ee) { constexpr int e = decltype(ee)::value; rz[e] = (float)Z[e / NU][e % NU]; });
            }
            store_step(mask);
        }
        plant(step, false);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                        // this step's stores, before the next step re-reads them
#ifdef TMPC_LEAN_CLOCK_PROBE
        probe_ph[3] += __builtin_amdgcn_s_memtime() - probe_a;
#endif
        ++step;
    }
    } while (MPC);
    // ---- global status block: wavefront max of the residuals, count of unsolved instances; behind the final store, or
    // (TMPC_LEAN_FOLD_FIRST) ahead of it ----
    auto fold = [&]() {
        float m0 = active ? (float)res0 : 0.f, m1 = active ? (float)res1 : 0.f, m2 = active ? (float)res2 : 0.f, m3 = active ? (float)res3 : 0.f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            m0 = fmaxf(m0, __shfl_xor(m0, o, 64));
            m1 = fmaxf(m1, __shfl_xor(m1, o, 64));
            m2 = fmaxf(m2, __shfl_xor(m2, o, 64));
            m3 = fmaxf(m3, __shfl_xor(m3, o, 64));
        }
        const unsigned long long unsolved = __builtin_amdgcn_ballot_w64(active && !conv);
        // (one record and one ticket per workgroup; the workspace-keeping forms, at the edge of their registers and LDS, keep
        // the accumulator fold every other family has)
        if constexpr (WS) fold_status(P, m0, m1, m2, m3, __popcll(unsolved), tid);
        else fold_status_records(P, m0, m1, m2, m3, __popcll(unsolved), tid);
    };
#ifdef TMPC_LEAN_CLOCK_PROBE
    const unsigned long long probe_t1 = __builtin_amdgcn_s_memtime(), probe_r1 = __builtin_amdgcn_s_memrealtime();   // loop end
    unsigned long long probe_fold = 0;
#endif
    if constexpr (TMPC_LEAN_FOLD_FIRST) {
        fold();
#ifdef TMPC_LEAN_CLOCK_PROBE
        probe_fold = __builtin_amdgcn_s_memrealtime();
#endif
    }
    // ---- final store of every instance that has not stored at its convergence: through LDS, so that a store instruction
    // writes 1 KiB — consecutive lanes consecutive 16 bytes (store_wave_wide, admm_quad.hip.h) — or, where the shape does not
    // take the wide form, whole 64-byte pieces (X: 16 consecutive floats of 4 instances) / one contiguous 256 bytes (U),
    // instead of 64 scattered 16-byte / 4-byte ones — with every wavefront finishing at once the scattered form took 50 us
    // of a 300 us launch (26 MB at 0.5 TB/s) ----
    {
        const bool mine = active && !conv;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(mine);
        if (mask) {
            if constexpr (HB) load_T(Ts);
            if constexpr (SCL) load_Si();
            if constexpr (WS) {
                store_ws(mask, mine, std::false_type{});                    // ... and the workspace, when the solve saves it
            } else {
                const long w0 = (long)blockIdx.x * 256 + (tid & ~63);      // the wavefront's first instance
                auto getx = [&](auto ee) { constexpr int e = decltype(ee)::value; return vnew_at(std::integral_constant<int, e / NX>{}, std::integral_constant<int, e % NX>{}); };
                auto getu = [&](auto ee) { constexpr int e = decltype(ee)::value; return (float)Z[e / NU][e % NU]; };
                if constexpr (SW != 0) store_wave_wide<EX, EU, SW>(s_stage[tid >> 6], P.xout + w0 * EX, P.uout + w0 * EU, lane, mask, getx, getu);
                else store_wave_coalesced<EX, EU>(s_stage[tid >> 6], P.xout + w0 * EX, P.uout + w0 * EU, lane, mask, getx, getu);
                if (mine) {
                    float *ro = P.res + b * 4;
                    P.iter[b] = P.iter_offset + it;
                    P.solved[b] = 0;
                    ro[0] = (float)res0, ro[1] = (float)res1, ro[2] = (float)res2, ro[3] = (float)res3;
                }
            }
        }
    }
    if constexpr (MPC) plant(step, true);                                       // ... and the plant step behind the last solve
#ifdef TMPC_LEAN_CLOCK_PROBE
    if (active) P.iter[b] = (int)(__builtin_amdgcn_s_memrealtime() & 0xFFFFFFull);     // stores issued
    __builtin_amdgcn_s_waitcnt(0);
    if (active) P.solved[b] = (int)(__builtin_amdgcn_s_memrealtime() & 0xFFFFFFull);   // ... and acknowledged
#endif
    if constexpr (!TMPC_LEAN_FOLD_FIRST) {
        fold();
#ifdef TMPC_LEAN_CLOCK_PROBE
        probe_fold = __builtin_amdgcn_s_memrealtime();
#endif
    }
#ifdef TMPC_LEAN_CLOCK_PROBE
    if constexpr (MPC) {
        if (active)
            for (int q = 0; q < 4; ++q) P.res[b * 4 + q] = (float)probe_ph[q];  // (the last step's end is the final store: not in [3])
    } else
    if (active) {
        P.res[b * 4 + 0] = (float)(probe_t1 - probe_t0);                                // core clocks of the iteration loop
        P.res[b * 4 + 1] = (float)(probe_r1 - probe_r0);                                // ... in 100 MHz ticks
        P.res[b * 4 + 2] = (float)(probe_entry & 0xFFFFFFull);                          // kernel entry on the chip-wide 100 MHz counter
        P.res[b * 4 + 3] = (float)(probe_fold & 0xFFFFFFull);                           // after the status fold
    }
#endif
}

}  // namespace tmpc
