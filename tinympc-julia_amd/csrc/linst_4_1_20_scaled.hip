// scaled sparse lean kernels for nx=4 nu=1 N=20 (admm_lean.hip.h, SCL): the sweeps on the diagonally scaled cartpole model
// (lean_entry.hip.h: kCartpolePatternScaled), 25 fp64 per knot for 27 — one-shot solves without a state bound
#include "lean_entry.hip.h"
namespace tmpc {
TMPC_DEFINE_LEAN_SCALED(4, 1, 20, kCartpolePatternScaled)
}
