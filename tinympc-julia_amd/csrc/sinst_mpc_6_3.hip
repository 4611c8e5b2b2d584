// stream kernel, in-kernel closed loop, 4 lanes per instance, for (nx, nu) = (6, 3): EXT x {fp32 state, fp32 state with one
// family per instance, fp64 state} less the one that spills (streamg_mpc_built), eight kernels
#include "streamg_entry.hip.h"
namespace tmpc {
TMPC_DEFINE_STREAMG_MPC(6, 3, 4)
}
