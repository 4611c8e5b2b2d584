// workspace-keeping lean kernels for nx=4 nu=1 N=20 (admm_lean.hip.h, WS): the sparse kernels of the cartpole model's (A, B) pattern (lean_entry.hip.h: kCartpolePattern)
#include "lean_entry.hip.h"
namespace tmpc {
TMPC_DEFINE_LEAN_WS_SPARSE(4, 1, 20, kCartpolePattern)
}
