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

// (WS: the workspace-keeping kernels, admm_lean.hip.h — same choices)
template <int NX, int NU, int N, bool XB, int REFS, bool WS = false>
hipError_t launch_lean_v(const AdmmParams &P, bool live, bool knot_bounds, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
    const int grid = (P.batch + 255) / 256;
    // (lean_one_form, solver.h)  The 512-register variant when the launch has at most one workgroup per CU (= one wavefront per SIMD), and — at any batch —
    // for tolerance-terminated solves: held to 256 registers the LIVE variants spill (73-187 registers) and lose to 512-register
    // wavefronts taking turns (batch 131 072, check live: 0.92 against 0.69 ms; with a state bound 2.95 against 1.05;
    // fixed-iteration solves: 0.47 / 0.61 against 0.46 / 0.69 — scripts/lean_time.py "big").  TINYMPC_HIP_LEAN_ONE: always (tuning aid).
    // WS: the 512-register form at any batch — held to 256 registers the workspace-keeping kernels spill 40-99 of them, and
    // 512-register wavefronts taking turns are within a few per cent of two sharing a SIMD (above).  Its fixed-iteration
    // kernel with a state bound, shared references and per-knot input bounds keeps one value in an accumulation register
    // across the loop (vgpr_spill_count 1); that calling pattern runs the tolerance-terminated kernel of the same flags
    // instead, which does the same arithmetic when no tolerance is positive and reports none.
    const bool one = WS || lean_one_form(P.batch, live, (P.host_flags & HF_LEAN_ONE) != 0);
    if (WS && XB && REFS == REF_SHARED && knot_bounds) live = true;
#define TMPC_LEAN_LAUNCH(LIVE_, UBK_, ONE_) \
    lean_dispatch(admm_lean_kernel<NX, NU, N, LIVE_, UBK_, ONE_, XB, REFS, float, 0, WS>, grid, stream, ev0, ev1, P)
#define TMPC_LEAN_LAUNCH2(LIVE_, UBK_) \
    do { if (WS || one) TMPC_LEAN_LAUNCH(LIVE_, UBK_, true); else if constexpr (!WS) TMPC_LEAN_LAUNCH(LIVE_, UBK_, false); } while (0)
    if (live) {   // (always the 512-register variant: the 256-register LIVE kernels are not even built)
        if (knot_bounds) TMPC_LEAN_LAUNCH(true, false, true); else TMPC_LEAN_LAUNCH(true, true, true);
    } else {
        if constexpr (WS && XB && REFS == REF_SHARED) TMPC_LEAN_LAUNCH2(false, true);   // (per-knot bounds: above)
        else if (knot_bounds) TMPC_LEAN_LAUNCH2(false, false); else TMPC_LEAN_LAUNCH2(false, true);
    }
#undef TMPC_LEAN_LAUNCH2
#undef TMPC_LEAN_LAUNCH
    return hipGetLastError();
}

// live: positive tolerances (residuals at every check, per-instance exits); knot_bounds: the input bounds depend on the knot;
// state_bounds: some enabled state bound is finite; P.ref_mode: REF_ZERO or REF_SHARED
template <int NX, int NU, int N>
hipError_t launch_lean(const AdmmParams &P, bool live, bool knot_bounds, bool state_bounds, hipStream_t stream, hipEvent_t ev0,
                       hipEvent_t ev1) {
    if (P.ref_mode == REF_SHARED)
        return state_bounds ? launch_lean_v<NX, NU, N, true, REF_SHARED>(P, live, knot_bounds, stream, ev0, ev1)
                            : launch_lean_v<NX, NU, N, false, REF_SHARED>(P, live, knot_bounds, stream, ev0, ev1);
    return state_bounds ? launch_lean_v<NX, NU, N, true, REF_ZERO>(P, live, knot_bounds, stream, ev0, ev1)
                        : launch_lean_v<NX, NU, N, false, REF_ZERO>(P, live, knot_bounds, stream, ev0, ev1);
}

// The sparse kernels of one (A, B) pattern SP (admm_lean.hip.h): zero references and input bounds that do not depend on the
// knot only, in the (LIVE, ONE, XB) combinations launch_lean_v picks — six kernels (the routing, Solver::launch_pass, sends
// nothing else here)
template <int NX, int NU, int N, uint64_t SP, bool WS = false>
hipError_t launch_lean_sparse(const AdmmParams &P, bool live, bool knot_bounds, bool state_bounds, hipStream_t stream, hipEvent_t ev0,
                              hipEvent_t ev1) {
    if (P.ref_mode != REF_ZERO || knot_bounds) return hipErrorInvalidValue;
    const int grid = (P.batch + 255) / 256;
    const bool one = WS || lean_one_form(P.batch, live, (P.host_flags & HF_LEAN_ONE) != 0);   // (WS: launch_lean_v)
#define TMPC_LEAN_LAUNCH(LIVE_, ONE_, XB_) \
    lean_dispatch(admm_lean_kernel<NX, NU, N, LIVE_, true, ONE_, XB_, REF_ZERO, float, SP, WS>, grid, stream, ev0, ev1, P)
#define TMPC_LEAN_LAUNCH2(LIVE_, ONE_) \
    do { if (state_bounds) TMPC_LEAN_LAUNCH(LIVE_, ONE_, true); else TMPC_LEAN_LAUNCH(LIVE_, ONE_, false); } while (0)
    if (live) TMPC_LEAN_LAUNCH2(true, true);
    else if (WS || one) TMPC_LEAN_LAUNCH2(false, true);
    else if constexpr (!WS) TMPC_LEAN_LAUNCH2(false, false);
#undef TMPC_LEAN_LAUNCH2
#undef TMPC_LEAN_LAUNCH
    return hipGetLastError();
}

// ---- one variant specialised at the first solve that needs it (jit.cpp: jit_lean_for) ----
// The headline kernel for a shape the library has no lean instantiation of (cartpole at another horizon, a smaller system):
// the reference accepts any (nx, nu, N) at run time (tiny_api.cpp:21-71).  A whole entry is 24 kernels and 45-90 s of compiler;
// one variant — the (LIVE, UBK, ONE, XB, REFS) the launch in hand needs — is a few seconds, so a unit carries exactly one.
// (ST = double: the fp64-state form, precision 2 — only ever built this way; SP: the model's exact pattern, the sparse sweeps)
template <int NX, int NU, int N, bool LIVE, bool UBK, bool ONE, bool XB, int REFS, class ST, uint64_t SP = 0, bool WS = false, bool MPC = false>
hipError_t launch_lean_exact(const AdmmParams &P, bool, bool, bool, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
    lean_dispatch(admm_lean_kernel<NX, NU, N, LIVE, UBK, ONE, XB, REFS, ST, SP, WS, MPC>, (P.batch + 255) / 256, stream, ev0, ev1, P);
    return hipGetLastError();
}
// ... its workspace-keeping form (LV_WS): the one variant is the entry's launch_ws
#define TMPC_DEFINE_LEAN_JIT_ENTRY_WS(NAME, NX, NU, NN, LIVE, UBK, ONE, XB, REFS, SP)                                    \
    namespace tmpc {                                                                                                     \
    const LeanEntry *lean_jit_entry() {                                                                                  \
        static const LeanEntry e = {NX, NU, NN, NAME, nullptr, SP, nullptr,                                              \
                                    &launch_lean_exact<NX, NU, NN, LIVE, UBK, ONE, XB, REFS, float, SP, true>};          \
        return &e;                                                                                                       \
    }                                                                                                                    \
    }                                                                                                                    \
    extern "C" const void *tmpc_jit_entry() { return tmpc::lean_jit_entry(); }
// ... and the in-kernel closed loop (LV_MPC): the one variant is the entry's launch_mpc
#define TMPC_DEFINE_LEAN_JIT_ENTRY_MPC(NAME, NX, NU, NN, LIVE, UBK, ONE, XB, REFS, SP)                                   \
    namespace tmpc {                                                                                                     \
    const LeanEntry *lean_jit_entry() {                                                                                  \
        static const LeanEntry e = {NX, NU, NN, NAME, nullptr, SP, nullptr, nullptr, nullptr,                            \
                                    &launch_lean_exact<NX, NU, NN, LIVE, UBK, ONE, XB, REFS, float, SP, true, true>};    \
        return &e;                                                                                                       \
    }                                                                                                                    \
    }                                                                                                                    \
    extern "C" const void *tmpc_jit_entry() { return tmpc::lean_jit_entry(); }
#define TMPC_DEFINE_LEAN_JIT_ENTRY_SP(NAME, NX, NU, NN, LIVE, UBK, ONE, XB, REFS, ST, SP)                                  \
    namespace tmpc {                                                                                                     \
    const LeanEntry *lean_jit_entry() {                                                                                  \
        static const LeanEntry e = {NX, NU, NN, NAME, &launch_lean_exact<NX, NU, NN, LIVE, UBK, ONE, XB, REFS, ST, SP>, SP}; \
        return &e;                                                                                                       \
    }                                                                                                                    \
    }                                                                                                                    \
    extern "C" const void *tmpc_jit_entry() { return tmpc::lean_jit_entry(); }
#define TMPC_DEFINE_LEAN_JIT_ENTRY(NAME, NX, NU, NN, LIVE, UBK, ONE, XB, REFS, ST) \
    TMPC_DEFINE_LEAN_JIT_ENTRY_SP(NAME, NX, NU, NN, LIVE, UBK, ONE, XB, REFS, ST, 0)

#define TMPC_DEFINE_LEAN_ENTRY(NX, NU, NN)                                                          \
    const LeanEntry *lean_entry_##NX##_##NU##_##NN() {                                              \
        static const LeanEntry e = {NX, NU, NN, "lean<" #NX "," #NU "," #NN ">", &launch_lean<NX, NU, NN>}; \
        return &e;                                                                                  \
    }
// ... with the sparse kernels of one (A, B) pattern beside it (lean_pattern_rm, admm_params.h)
#define TMPC_DEFINE_LEAN_ENTRY_SP(NX, NU, NN, SP)                                                                  \
    const LeanEntry *lean_entry_##NX##_##NU##_##NN() {                                                             \
        static const LeanEntry e = {NX, NU, NN, "lean<" #NX "," #NU "," #NN ">", &launch_lean<NX, NU, NN>, (SP),   \
                                    &launch_lean_sparse<NX, NU, NN, (SP)>};                                          \
        return &e;                                                                                                 \
    }

// The workspace-keeping kernels of a built-in entry live in translation units of their own, one per (XB, REFS) pair of the
// dense kernels and one for the sparse ones (linst_ws_*.hip), so that the build stays parallel; the entry's unit declares
// them and picks among them as launch_lean does.
#define TMPC_LEAN_WS_ARGS const AdmmParams &P, bool live, bool knot_bounds, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1
#define TMPC_DECLARE_LEAN_WS_PARTS(NX, NU, NN)                                                                          \
    hipError_t lean_ws_##NX##_##NU##_##NN##_z(TMPC_LEAN_WS_ARGS);                                                      \
    hipError_t lean_ws_##NX##_##NU##_##NN##_zx(TMPC_LEAN_WS_ARGS);                                                     \
    hipError_t lean_ws_##NX##_##NU##_##NN##_s(TMPC_LEAN_WS_ARGS);                                                      \
    hipError_t lean_ws_##NX##_##NU##_##NN##_sx(TMPC_LEAN_WS_ARGS);                                                     \
    hipError_t lean_ws_##NX##_##NU##_##NN##_sparse(const AdmmParams &, bool, bool, bool, hipStream_t, hipEvent_t, hipEvent_t); \
    inline hipError_t lean_ws_##NX##_##NU##_##NN(const AdmmParams &P, bool live, bool knot_bounds, bool state_bounds,   \
                                                 hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {                  \
        if (P.ref_mode == REF_SHARED)                                                                                   \
            return state_bounds ? lean_ws_##NX##_##NU##_##NN##_sx(P, live, knot_bounds, stream, ev0, ev1)               \
                                : lean_ws_##NX##_##NU##_##NN##_s(P, live, knot_bounds, stream, ev0, ev1);               \
        return state_bounds ? lean_ws_##NX##_##NU##_##NN##_zx(P, live, knot_bounds, stream, ev0, ev1)                   \
                            : lean_ws_##NX##_##NU##_##NN##_z(P, live, knot_bounds, stream, ev0, ev1);                   \
    }
#define TMPC_DEFINE_LEAN_WS_PART(NX, NU, NN, TAG, XB, REFS)                                                             \
    hipError_t lean_ws_##NX##_##NU##_##NN##_##TAG(TMPC_LEAN_WS_ARGS) {                                                  \
        return launch_lean_v<NX, NU, NN, XB, REFS, true>(P, live, knot_bounds, stream, ev0, ev1);                       \
    }
#define TMPC_DEFINE_LEAN_WS_SPARSE(NX, NU, NN, SP)                                                                      \
    hipError_t lean_ws_##NX##_##NU##_##NN##_sparse(const AdmmParams &P, bool live, bool knot_bounds, bool state_bounds, \
                                                   hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {                \
        return launch_lean_sparse<NX, NU, NN, (SP), true>(P, live, knot_bounds, state_bounds, stream, ev0, ev1);        \
    }
// an entry with the sparse kernels and the workspace-keeping kernels of both kinds
#define TMPC_DEFINE_LEAN_ENTRY_SP_WS(NX, NU, NN, SP)                                                               \
    TMPC_DECLARE_LEAN_WS_PARTS(NX, NU, NN)                                                                         \
    const LeanEntry *lean_entry_##NX##_##NU##_##NN() {                                                             \
        static const LeanEntry e = {NX, NU, NN, "lean<" #NX "," #NU "," #NN ">", &launch_lean<NX, NU, NN>, (SP),   \
                                    &launch_lean_sparse<NX, NU, NN, (SP)>, &lean_ws_##NX##_##NU##_##NN,            \
                                    &lean_ws_##NX##_##NU##_##NN##_sparse};                                          \
        return &e;                                                                                                 \
    }

// The in-kernel closed loop (admm_lean.hip.h, MPC) of a built-in entry, in translation units of their own like the WS kernels
// (linst_mpc_*.hip): the tolerance-terminated kernels only — they do the fixed-iteration arithmetic when no tolerance is
// positive, so a fixed-iteration rollout runs them too (as launch_lean_v does for one WS pattern) — by (XB, REFS) and the
// kind of input bounds; the sparse ones by XB.
template <int NX, int NU, int N, bool XB, int REFS>
hipError_t launch_lean_mpc_v(const AdmmParams &P, bool knot_bounds, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
    const int grid = (P.batch + 255) / 256;
    if (knot_bounds) lean_dispatch(admm_lean_kernel<NX, NU, N, true, false, true, XB, REFS, float, 0, true, true>, grid, stream, ev0, ev1, P);
    else lean_dispatch(admm_lean_kernel<NX, NU, N, true, true, true, XB, REFS, float, 0, true, true>, grid, stream, ev0, ev1, P);
    return hipGetLastError();
}
template <int NX, int NU, int N, uint64_t SP>
hipError_t launch_lean_mpc_sparse(const AdmmParams &P, bool, bool knot_bounds, bool state_bounds, hipStream_t stream, hipEvent_t ev0,
                                  hipEvent_t ev1) {
    if (P.ref_mode != REF_ZERO || knot_bounds) return hipErrorInvalidValue;
    const int grid = (P.batch + 255) / 256;
    if (state_bounds) lean_dispatch(admm_lean_kernel<NX, NU, N, true, true, true, true, REF_ZERO, float, SP, true, true>, grid, stream, ev0, ev1, P);
    else lean_dispatch(admm_lean_kernel<NX, NU, N, true, true, true, false, REF_ZERO, float, SP, true, true>, grid, stream, ev0, ev1, P);
    return hipGetLastError();
}
#define TMPC_LEAN_MPC_ARGS const AdmmParams &P, bool knot_bounds, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1
#define TMPC_DECLARE_LEAN_MPC_PARTS(NX, NU, NN)                                                                         \
    hipError_t lean_mpc_##NX##_##NU##_##NN##_z(TMPC_LEAN_MPC_ARGS);                                                    \
    hipError_t lean_mpc_##NX##_##NU##_##NN##_zx(TMPC_LEAN_MPC_ARGS);                                                   \
    hipError_t lean_mpc_##NX##_##NU##_##NN##_s(TMPC_LEAN_MPC_ARGS);                                                    \
    hipError_t lean_mpc_##NX##_##NU##_##NN##_sx(TMPC_LEAN_MPC_ARGS);                                                   \
    hipError_t lean_mpc_##NX##_##NU##_##NN##_sparse(const AdmmParams &, bool, bool, bool, hipStream_t, hipEvent_t, hipEvent_t); \
    inline hipError_t lean_mpc_##NX##_##NU##_##NN(const AdmmParams &P, bool, bool knot_bounds, bool state_bounds,       \
                                                  hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {                 \
        if (P.ref_mode == REF_SHARED)                                                                                   \
            return state_bounds ? lean_mpc_##NX##_##NU##_##NN##_sx(P, knot_bounds, stream, ev0, ev1)                    \
                                : lean_mpc_##NX##_##NU##_##NN##_s(P, knot_bounds, stream, ev0, ev1);                    \
        return state_bounds ? lean_mpc_##NX##_##NU##_##NN##_zx(P, knot_bounds, stream, ev0, ev1)                        \
                            : lean_mpc_##NX##_##NU##_##NN##_z(P, knot_bounds, stream, ev0, ev1);                        \
    }
#define TMPC_DEFINE_LEAN_MPC_PART(NX, NU, NN, TAG, XB, REFS)                                                            \
    hipError_t lean_mpc_##NX##_##NU##_##NN##_##TAG(TMPC_LEAN_MPC_ARGS) {                                                \
        return launch_lean_mpc_v<NX, NU, NN, XB, REFS>(P, knot_bounds, stream, ev0, ev1);                               \
    }
#define TMPC_DEFINE_LEAN_MPC_SPARSE(NX, NU, NN, SP)                                                                     \
    hipError_t lean_mpc_##NX##_##NU##_##NN##_sparse(const AdmmParams &P, bool live, bool knot_bounds, bool state_bounds, \
                                                    hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {               \
        return launch_lean_mpc_sparse<NX, NU, NN, (SP)>(P, live, knot_bounds, state_bounds, stream, ev0, ev1);          \
    }
// an entry with the sparse kernels, the workspace-keeping kernels and the in-kernel closed loop of both kinds
#define TMPC_DEFINE_LEAN_ENTRY_SP_WS_MPC(NX, NU, NN, SP)                                                           \
    TMPC_DECLARE_LEAN_WS_PARTS(NX, NU, NN)                                                                         \
    TMPC_DECLARE_LEAN_MPC_PARTS(NX, NU, NN)                                                                        \
    const LeanEntry *lean_entry_##NX##_##NU##_##NN() {                                                             \
        static const LeanEntry e = {NX, NU, NN, "lean<" #NX "," #NU "," #NN ">", &launch_lean<NX, NU, NN>, (SP),   \
                                    &launch_lean_sparse<NX, NU, NN, (SP)>, &lean_ws_##NX##_##NU##_##NN,            \
                                    &lean_ws_##NX##_##NU##_##NN##_sparse, &lean_mpc_##NX##_##NU##_##NN,             \
                                    &lean_mpc_##NX##_##NU##_##NN##_sparse};                                         \
        return &e;                                                                                                 \
    }

}  // namespace tmpc
