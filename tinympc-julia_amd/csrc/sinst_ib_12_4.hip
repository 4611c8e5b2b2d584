// stream kernel, per-instance-bounds form, 4 lanes per instance, for (nx, nu) = (12, 4): {box, + cones / linear rows} x
// {one family, one per instance} x OS, eight kernels
#include "streamg_entry.hip.h"
namespace tmpc {
TMPC_DEFINE_STREAMG_IB(12, 4, 4)
}
