// in-kernel closed loop of the lean kernel for nx=4 nu=1 N=20 (admm_lean.hip.h, MPC): the sparse kernels of the cartpole model's (A, B) pattern (linst_4_1_20.hip)
#include "lean_entry.hip.h"
namespace tmpc {
namespace {
constexpr double kCartpoleA[16] = {1.0, 0.01, 0.0, 0.0,
                                   0.0, 1.0, 0.039, 0.0,
                                   0.0, 0.0, 1.002, 0.01,
                                   0.0, 0.0, 0.458, 1.002};
constexpr double kCartpoleB[4] = {0.0, 0.02, 0.0, 0.067};
}  // namespace
TMPC_DEFINE_LEAN_MPC_SPARSE(4, 1, 20, lean_pattern_rm(4, 1, kCartpoleA, kCartpoleB))
}
