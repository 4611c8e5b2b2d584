// workspace-keeping lean kernels for nx=4 nu=1 N=20 (admm_lean.hip.h, WS): zero references, a finite state bound
#include "lean_entry.hip.h"
namespace tmpc {
TMPC_DEFINE_LEAN_WS_PART(4, 1, 20, zx, true, REF_ZERO)
}
