// bp_pick_token: token selection on the device for the decode loops, one row of logits in, one token out.  The kernel is
// pick_core.h's (contract, passes and layout are described there); this code object holds its plain instantiations.
#include "pick_core.h"

namespace bp {

hipError_t launch_pick_token(const PickParams &p, int dtype, hipStream_t stream) { return launch_pick<Plain>(p, 0, dtype, stream); }

}  // namespace bp
