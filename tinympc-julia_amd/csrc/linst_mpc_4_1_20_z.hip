// in-kernel closed loop of the lean kernel for nx=4 nu=1 N=20 (admm_lean.hip.h, MPC): zero references, no state bound
#include "lean_entry.hip.h"
namespace tmpc {
TMPC_DEFINE_LEAN_MPC_PART(4, 1, 20, z, false, REF_ZERO)
}
