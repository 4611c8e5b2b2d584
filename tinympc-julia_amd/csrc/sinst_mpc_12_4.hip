// stream kernel, in-kernel closed loop, 4 lanes per instance, for (nx, nu) = (12, 4): EXT x fp64 state, three kernels (the fp32-state
// forms spill at three wavefronts per SIMD and stay with the chain: streamg_mpc_built)
#include "streamg_entry.hip.h"
namespace tmpc {
TMPC_DEFINE_STREAMG_MPC(12, 4, 4)
}
