// Launcher of one lean-kernel instantiation (admm_lean.hip.h); one translation unit per shape (linst_*.hip).
#pragma once
#include <hip/hip_ext.h>

#include "admm_lean.hip.h"
#include "solver.h"

namespace tmpc {

// One dispatch.  ev0 / ev1 (a profiled solve): the kernel's start and end, carried by the dispatch packet itself instead of
// marker packets of their own before and behind it (Solver::launch_pass); null events: the plain launch.
template <class K>
inline void lean_dispatch(K kernel, int grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const AdmmParams &P) {
    if (ev0 || ev1) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, stream, ev0, ev1, 0, P);
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, stream, P);
}

// Every launcher here maps the variant bits lean_plan decided (solver.h, LV_*) onto the kernel of exactly those bits and
// decides nothing itself; hipErrorNotSupported: the unit has no such kernel.
#define TMPC_LEAN_ARGS const AdmmParams &P, int variant, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1

// The dense kernels of one (XB, REFS) pair, one-shot (24 per shape), workspace-keeping (WS) or the in-kernel closed loop (MPC).
// What is built: tolerance-terminated kernels in the 512-register form only (held to 256 registers they spill 73-187 of them
// and lose to 512-register wavefronts taking turns: batch 131 072, check live, 0.92 against 0.69 ms; with a state bound 2.95
// against 1.05 — scripts/lean_time.py "big"); WS kernels in the 512-register form only (held to 256 they spill 40-99); no
// fixed-iteration WS kernel with a state bound, shared references and per-knot input bounds (it keeps one value in an
// accumulation register across the loop, vgpr_spill_count 1: lean_plan sends that pattern to the tolerance-terminated one,
// which does the same arithmetic when no tolerance is positive); the loop as tolerance-terminated kernels only.
template <int NX, int NU, int N, bool XB, int REFS, bool WS = false, bool MPC = false>
hipError_t launch_lean_v(TMPC_LEAN_ARGS) {
    const int grid = (P.batch + 255) / 256;
    constexpr bool FIXED = !MPC, FIXED_KNOT = FIXED && !(WS && XB && REFS == REF_SHARED), TWO = !WS;
#define TMPC_LEAN_LAUNCH(LIVE_, UBK_, ONE_) \
    lean_dispatch(admm_lean_kernel<NX, NU, N, LIVE_, UBK_, ONE_, XB, REFS, float, 0, WS, MPC>, grid, stream, ev0, ev1, P)
    switch (variant & (LV_LIVE | LV_UBK | LV_ONE)) {
        case LV_LIVE | LV_UBK | LV_ONE: TMPC_LEAN_LAUNCH(true, true, true); break;
        case LV_LIVE | LV_ONE: TMPC_LEAN_LAUNCH(true, false, true); break;
        case LV_UBK | LV_ONE: if constexpr (FIXED) TMPC_LEAN_LAUNCH(false, true, true); else return hipErrorNotSupported; break;
        case LV_ONE: if constexpr (FIXED_KNOT) TMPC_LEAN_LAUNCH(false, false, true); else return hipErrorNotSupported; break;
        case LV_UBK: if constexpr (TWO) TMPC_LEAN_LAUNCH(false, true, false); else return hipErrorNotSupported; break;
        case 0: if constexpr (TWO) TMPC_LEAN_LAUNCH(false, false, false); else return hipErrorNotSupported; break;
        default: return hipErrorNotSupported;
    }
#undef TMPC_LEAN_LAUNCH
    return hipGetLastError();
}

// the dense one-shot kernels of a shape, by (XB, REFS)
template <int NX, int NU, int N>
hipError_t launch_lean(TMPC_LEAN_ARGS) {
    if (variant & (LV_F64 | LV_SPARSE | LV_WS | LV_MPC)) return hipErrorNotSupported;
    if (variant & LV_SHARED)
        return (variant & LV_XB) ? launch_lean_v<NX, NU, N, true, REF_SHARED>(P, variant, stream, ev0, ev1)
                                 : launch_lean_v<NX, NU, N, false, REF_SHARED>(P, variant, stream, ev0, ev1);
    return (variant & LV_XB) ? launch_lean_v<NX, NU, N, true, REF_ZERO>(P, variant, stream, ev0, ev1)
                             : launch_lean_v<NX, NU, N, false, REF_ZERO>(P, variant, stream, ev0, ev1);
}

// The sparse kernels of one (A, B) pattern SP (admm_lean.hip.h): zero references and input bounds that do not depend on the
// knot only, in the (LIVE, ONE) combinations of the dense ones, by XB — six one-shot kernels, four WS, two MPC
template <int NX, int NU, int N, uint64_t SP, bool WS = false, bool MPC = false>
hipError_t launch_lean_sparse(TMPC_LEAN_ARGS) {
    if ((variant & (LV_UBK | LV_SHARED)) != LV_UBK) return hipErrorNotSupported;
    const int grid = (P.batch + 255) / 256;
#define TMPC_LEAN_LAUNCH(LIVE_, ONE_, XB_) \
    lean_dispatch(admm_lean_kernel<NX, NU, N, LIVE_, true, ONE_, XB_, REF_ZERO, float, SP, WS, MPC>, grid, stream, ev0, ev1, P)
    switch (variant & (LV_LIVE | LV_ONE | LV_XB)) {
        case LV_LIVE | LV_ONE | LV_XB: TMPC_LEAN_LAUNCH(true, true, true); break;
        case LV_LIVE | LV_ONE: TMPC_LEAN_LAUNCH(true, true, false); break;
        case LV_ONE | LV_XB: if constexpr (!MPC) TMPC_LEAN_LAUNCH(false, true, true); else return hipErrorNotSupported; break;
        case LV_ONE: if constexpr (!MPC) TMPC_LEAN_LAUNCH(false, true, false); else return hipErrorNotSupported; break;
        case LV_XB: if constexpr (!WS) TMPC_LEAN_LAUNCH(false, false, true); else return hipErrorNotSupported; break;
        case 0: if constexpr (!WS) TMPC_LEAN_LAUNCH(false, false, false); else return hipErrorNotSupported; break;
        default: return hipErrorNotSupported;
    }
#undef TMPC_LEAN_LAUNCH
    return hipGetLastError();
}

// ---- one variant specialised at the first solve that needs it (jit.cpp: jit_lean_for) ----
// The headline kernel for a shape the library has no lean instantiation of (cartpole at another horizon, a smaller system):
// the reference accepts any (nx, nu, N) at run time (tiny_api.cpp:21-71).  A whole entry is 24 kernels and 45-90 s of compiler;
// one variant — the bits V the launch in hand needs — is a few seconds, so a unit carries exactly one.
// (ST = double: the fp64-state form, precision 2 — only ever built this way; SP: the model's exact pattern, the sparse sweeps)
template <int NX, int NU, int N, int V, class ST, uint64_t SP>
hipError_t launch_lean_exact(TMPC_LEAN_ARGS) {
    if (variant != V) return hipErrorNotSupported;
    lean_dispatch(admm_lean_kernel<NX, NU, N, (V & LV_LIVE) != 0, (V & LV_UBK) != 0, (V & LV_ONE) != 0, (V & LV_XB) != 0,
                                   (V & LV_SHARED) ? REF_SHARED : REF_ZERO, ST, SP, (V & LV_WS) != 0, (V & LV_MPC) != 0>,
                  (P.batch + 255) / 256, stream, ev0, ev1, P);
    return hipGetLastError();
}
#define TMPC_DEFINE_LEAN_JIT_VARIANT(NAME, NX, NU, NN, V, ST, SP)                                                       \
    namespace tmpc {                                                                                                     \
    const LeanEntry *lean_jit_entry() {                                                                                  \
        static const LeanEntry e = {NX, NU, NN, NAME, SP, 0, &launch_lean_exact<NX, NU, NN, (V), ST, SP>};               \
        return &e;                                                                                                       \
    }                                                                                                                    \
    }                                                                                                                    \
    extern "C" const void *tmpc_jit_entry() { return tmpc::lean_jit_entry(); }
// ... spelled flag by flag, as the assembly and compile tests write their units: the same one macro
#define TMPC_LEAN_BITS(LIVE, UBK, ONE, XB, REFS, ST, SP)                                                                 \
    ((LIVE ? tmpc::LV_LIVE : 0) | (UBK ? tmpc::LV_UBK : 0) | (ONE ? tmpc::LV_ONE : 0) | (XB ? tmpc::LV_XB : 0) |       \
     ((REFS) == tmpc::REF_SHARED ? tmpc::LV_SHARED : 0) | (sizeof(ST) == 8 ? tmpc::LV_F64 : 0) | ((SP) ? tmpc::LV_SPARSE : 0))
#define TMPC_DEFINE_LEAN_JIT_ENTRY_SP(NAME, NX, NU, NN, LIVE, UBK, ONE, XB, REFS, ST, SP) \
    TMPC_DEFINE_LEAN_JIT_VARIANT(NAME, NX, NU, NN, TMPC_LEAN_BITS(LIVE, UBK, ONE, XB, REFS, ST, SP), ST, SP)
#define TMPC_DEFINE_LEAN_JIT_ENTRY(NAME, NX, NU, NN, LIVE, UBK, ONE, XB, REFS, ST) \
    TMPC_DEFINE_LEAN_JIT_ENTRY_SP(NAME, NX, NU, NN, LIVE, UBK, ONE, XB, REFS, ST, 0)
#define TMPC_DEFINE_LEAN_JIT_ENTRY_WS(NAME, NX, NU, NN, LIVE, UBK, ONE, XB, REFS, SP) \
    TMPC_DEFINE_LEAN_JIT_VARIANT(NAME, NX, NU, NN, TMPC_LEAN_BITS(LIVE, UBK, ONE, XB, REFS, float, SP) | tmpc::LV_WS, float, SP)
#define TMPC_DEFINE_LEAN_JIT_ENTRY_MPC(NAME, NX, NU, NN, LIVE, UBK, ONE, XB, REFS, SP) \
    TMPC_DEFINE_LEAN_JIT_VARIANT(NAME, NX, NU, NN, TMPC_LEAN_BITS(LIVE, UBK, ONE, XB, REFS, float, SP) | tmpc::LV_WS | tmpc::LV_MPC, float, SP)

// ---- built-in entries ----
// the dense one-shot kernels only
#define TMPC_DEFINE_LEAN_ENTRY(NX, NU, NN)                                                                \
    const LeanEntry *lean_entry_##NX##_##NU##_##NN() {                                                    \
        static const LeanEntry e = {NX, NU, NN, "lean<" #NX "," #NU "," #NN ">", 0, 0, &launch_lean<NX, NU, NN>}; \
        return &e;                                                                                        \
    }

// The cartpole model's (A, B) (problems.py: cartpole, the benchmark's family), whose pattern the built-in sparse kernels carry.
// Only the zero / unit pattern is compiled in (admm_params.h: lean_pattern_rm): 8 nonzeros of A, two of them exactly 1, and
// 2 nonzeros of B; the values come from the pack.
constexpr double kCartpoleA[16] = {1.0, 0.01, 0.0, 0.0,
                                   0.0, 1.0, 0.039, 0.0,
                                   0.0, 0.0, 1.002, 0.01,
                                   0.0, 0.0, 0.458, 1.002};
constexpr double kCartpoleB[4] = {0.0, 0.02, 0.0, 0.067};
constexpr uint64_t kCartpolePattern = lean_pattern_rm(4, 1, kCartpoleA, kCartpoleB);
// ... and its scaled pattern (admm_params.h: lean_pattern_scaled): A01, A12, A23 and B3 become units beside A00 and A11 — the
// forward rows 2 and 3 get a free start, 25 fp64 per knot for 27
constexpr uint64_t kCartpolePatternScaled = lean_pattern_scaled(kCartpolePattern, 4, 1);
static_assert(lean_cost_scaled(kCartpolePatternScaled, 4, 1) == 25 && lean_cost_sparse(kCartpolePattern, 4, 1) == 27, "cartpole: 25 for 27");

// The scaled sparse kernels of a built-in entry (admm_lean.hip.h: SCL), in a translation unit of their own
// (linst_*_scaled.hip): the cases lean_runs_scaled (solver.h) names — one-shot, no state bound, uniform input bounds
template <int NX, int NU, int N, uint64_t SPZ>
hipError_t launch_lean_scaled(TMPC_LEAN_ARGS) {
    static_assert(lsp_scaled(SPZ), "a scaled pattern");
    const int grid = (P.batch + 255) / 256;
#define TMPC_LEAN_LAUNCH(LIVE_, ONE_) \
    lean_dispatch(admm_lean_kernel<NX, NU, N, LIVE_, true, ONE_, false, REF_ZERO, float, SPZ>, grid, stream, ev0, ev1, P)
    switch (variant & (LV_LIVE | LV_ONE)) {
        case LV_LIVE | LV_ONE: TMPC_LEAN_LAUNCH(true, true); break;
        case LV_ONE: TMPC_LEAN_LAUNCH(false, true); break;
        default: return hipErrorNotSupported;   // (the 256-register form spills 63 registers with these sweeps: not built)
    }
#undef TMPC_LEAN_LAUNCH
    return hipGetLastError();
}
#define TMPC_DEFINE_LEAN_SCALED(NX, NU, NN, SPZ)                                             \
    hipError_t lean_scaled_##NX##_##NU##_##NN(TMPC_LEAN_ARGS) {                              \
        return launch_lean_scaled<NX, NU, NN, (SPZ)>(P, variant, stream, ev0, ev1);          \
    }

// The workspace-keeping kernels (KIND ws) and the in-kernel closed loops (KIND mpc) of a built-in entry live in translation
// units of their own, one per (XB, REFS) pair of the dense kernels and one for the sparse ones (linst_ws_*.hip,
// linst_mpc_*.hip), so that the build stays parallel; the entry's unit declares them and forwards by kind, then by
// (XB, REFS) as launch_lean does.
#define TMPC_DECLARE_LEAN_PARTS(KIND, NX, NU, NN)                          \
    hipError_t lean_##KIND##_##NX##_##NU##_##NN##_z(TMPC_LEAN_ARGS);      \
    hipError_t lean_##KIND##_##NX##_##NU##_##NN##_zx(TMPC_LEAN_ARGS);     \
    hipError_t lean_##KIND##_##NX##_##NU##_##NN##_s(TMPC_LEAN_ARGS);      \
    hipError_t lean_##KIND##_##NX##_##NU##_##NN##_sx(TMPC_LEAN_ARGS);     \
    hipError_t lean_##KIND##_##NX##_##NU##_##NN##_sparse(TMPC_LEAN_ARGS);
#define TMPC_LEAN_PARTS(KIND, NX, NU, NN)                                                                              \
    {&lean_##KIND##_##NX##_##NU##_##NN##_z, &lean_##KIND##_##NX##_##NU##_##NN##_zx, &lean_##KIND##_##NX##_##NU##_##NN##_s, \
     &lean_##KIND##_##NX##_##NU##_##NN##_sx, &lean_##KIND##_##NX##_##NU##_##NN##_sparse}
#define TMPC_DEFINE_LEAN_PART(KIND, WS, MPC, NX, NU, NN, TAG, XB, REFS)                          \
    hipError_t lean_##KIND##_##NX##_##NU##_##NN##_##TAG(TMPC_LEAN_ARGS) {                         \
        return launch_lean_v<NX, NU, NN, XB, REFS, WS, MPC>(P, variant, stream, ev0, ev1);        \
    }
#define TMPC_DEFINE_LEAN_PART_SPARSE(KIND, WS, MPC, NX, NU, NN, SP)                               \
    hipError_t lean_##KIND##_##NX##_##NU##_##NN##_sparse(TMPC_LEAN_ARGS) {                        \
        return launch_lean_sparse<NX, NU, NN, (SP), WS, MPC>(P, variant, stream, ev0, ev1);       \
    }
#define TMPC_DEFINE_LEAN_WS_PART(NX, NU, NN, TAG, XB, REFS) TMPC_DEFINE_LEAN_PART(ws, true, false, NX, NU, NN, TAG, XB, REFS)
#define TMPC_DEFINE_LEAN_WS_SPARSE(NX, NU, NN, SP) TMPC_DEFINE_LEAN_PART_SPARSE(ws, true, false, NX, NU, NN, SP)
#define TMPC_DEFINE_LEAN_MPC_PART(NX, NU, NN, TAG, XB, REFS) TMPC_DEFINE_LEAN_PART(mpc, true, true, NX, NU, NN, TAG, XB, REFS)
#define TMPC_DEFINE_LEAN_MPC_SPARSE(NX, NU, NN, SP) TMPC_DEFINE_LEAN_PART_SPARSE(mpc, true, true, NX, NU, NN, SP)
// an entry with the sparse kernels of pattern SP, the workspace-keeping kernels and the in-kernel closed loop of both kinds
// ... and the scaled sparse kernels of pattern SPZ (0: none), which a one-shot sparse launch takes where lean_runs_scaled says so
#define TMPC_DEFINE_LEAN_ENTRY_FULL(NX, NU, NN, SP, SPZ)                                                               \
    TMPC_DECLARE_LEAN_PARTS(ws, NX, NU, NN)                                                                            \
    TMPC_DECLARE_LEAN_PARTS(mpc, NX, NU, NN)                                                                           \
    hipError_t lean_scaled_##NX##_##NU##_##NN(TMPC_LEAN_ARGS);                                                         \
    const LeanEntry *lean_entry_##NX##_##NU##_##NN();                                                                  \
    static hipError_t lean_launch_##NX##_##NU##_##NN(TMPC_LEAN_ARGS) {                                                 \
        static constexpr LeanLaunch ws[5] = TMPC_LEAN_PARTS(ws, NX, NU, NN), mpc[5] = TMPC_LEAN_PARTS(mpc, NX, NU, NN); \
        if (variant & LV_F64) return hipErrorNotSupported;                                                             \
        const int part = (variant & LV_SPARSE) ? 4 : ((variant & LV_SHARED) ? 2 : 0) + ((variant & LV_XB) ? 1 : 0);    \
        if (variant & LV_MPC) return mpc[part](P, variant, stream, ev0, ev1);                                          \
        if (variant & LV_WS) return ws[part](P, variant, stream, ev0, ev1);                                            \
        if (lean_runs_scaled(lean_entry_##NX##_##NU##_##NN(), variant, P.host_flags))                                  \
            return lean_scaled_##NX##_##NU##_##NN(P, variant, stream, ev0, ev1);                                       \
        return part == 4 ? launch_lean_sparse<NX, NU, NN, (SP)>(P, variant, stream, ev0, ev1)                          \
                         : launch_lean<NX, NU, NN>(P, variant, stream, ev0, ev1);                                      \
    }                                                                                                                  \
    const LeanEntry *lean_entry_##NX##_##NU##_##NN() {                                                                 \
        static const LeanEntry e = {NX, NU, NN, "lean<" #NX "," #NU "," #NN ">", (SP), LK_ALL, &lean_launch_##NX##_##NU##_##NN, (SPZ)}; \
        return &e;                                                                                                     \
    }

}  // namespace tmpc
