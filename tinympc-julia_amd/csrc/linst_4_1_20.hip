// lean kernel instantiation for nx=4 nu=1 N=20 (one lane per instance, one-shot solves without an active state bound), with
// the sparse kernels of the cartpole model's (A, B) pattern (lean_entry.hip.h: kCartpolePattern) beside it
// (the workspace-keeping kernels of both kinds come from linst_ws_4_1_20_*.hip, the in-kernel closed loops from
// linst_mpc_4_1_20_*.hip, the scaled sparse kernels from linst_4_1_20_scaled.hip; all are only declared here)
#include "lean_entry.hip.h"
namespace tmpc {
TMPC_DEFINE_LEAN_ENTRY_FULL(4, 1, 20, kCartpolePattern, kCartpolePatternScaled)
}
