// lean kernel instantiation for nx=4 nu=1 N=20 (one lane per instance, one-shot solves without an active state bound), with
// the sparse kernels of the cartpole model's (A, B) pattern (problems.py: cartpole, the benchmark's family) beside it
// (the workspace-keeping kernels of both kinds come from linst_ws_4_1_20_*.hip, the in-kernel closed loops from
// linst_mpc_4_1_20_*.hip; both are only declared here)
#include "lean_entry.hip.h"
namespace tmpc {
namespace {
// only the zero / unit pattern is compiled in (admm_params.h: lean_pattern_rm): 8 nonzeros of A, two of them exactly 1, and
// 2 nonzeros of B; the values come from the pack
constexpr double kCartpoleA[16] = {1.0, 0.01, 0.0, 0.0,
                                   0.0, 1.0, 0.039, 0.0,
                                   0.0, 0.0, 1.002, 0.01,
                                   0.0, 0.0, 0.458, 1.002};
constexpr double kCartpoleB[4] = {0.0, 0.02, 0.0, 0.067};
}  // namespace
TMPC_DEFINE_LEAN_ENTRY_SP_WS_MPC(4, 1, 20, lean_pattern_rm(4, 1, kCartpoleA, kCartpoleB))
}
