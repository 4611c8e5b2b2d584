// in-kernel closed loop of the lean kernel for nx=4 nu=1 N=20 (admm_lean.hip.h, MPC): the sparse kernels of the cartpole model's (A, B) pattern (lean_entry.hip.h: kCartpolePattern)
#include "lean_entry.hip.h"
namespace tmpc {
TMPC_DEFINE_LEAN_MPC_SPARSE(4, 1, 20, kCartpolePattern)
}
