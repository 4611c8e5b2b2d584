// stream kernel, in-kernel closed loop, 4 lanes per instance, for (nx, nu) = (4, 1): EXT x {fp32 state, fp32 state with one
// family per instance, fp64 state}, nine kernels
#include "streamg_entry.hip.h"
namespace tmpc {
TMPC_DEFINE_STREAMG_MPC(4, 1, 4)
}
