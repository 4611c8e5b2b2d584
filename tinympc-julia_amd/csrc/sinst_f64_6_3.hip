// stream kernel, fp64-state form (precision 2), 4 lanes per instance, for (nx, nu) = (6, 3): EXT x OS, six kernels
#include "streamg_entry.hip.h"
namespace tmpc {
TMPC_DEFINE_STREAMG_F64(6, 3, 4)
}
