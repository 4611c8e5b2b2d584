// stream kernel, per-instance-cones form, 4 lanes per instance, for (nx, nu) = (12, 4): cones / linear rows as run-time
// flags x {one family, one per instance} x OS, four kernels
#include "streamg_entry.hip.h"
namespace tmpc {
TMPC_DEFINE_STREAMG_IC(12, 4, 4)
}
