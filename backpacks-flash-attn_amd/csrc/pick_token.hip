// bp_pick_token: token selection on the device for the decode loops, one row of logits in, one token out.  The kernel is
// pick_core.h's (contract, passes and layout are described there); this code object holds its plain instantiations.
#include "pick_core.h"

namespace bp {

hipError_t launch_pick_token(const PickParams &p, int dtype, hipStream_t stream) {
    auto go = [&](auto et) {
        hipLaunchKernelGGL((pick_token_kernel<decltype(et)>), dim3((unsigned)p.batch), dim3(kPickThreads), 0, stream, p);
        return hipGetLastError();
    };
    if (dtype == BP_DTYPE_F32) return go(float{});
    return with_dtype(dtype, go);
}

}  // namespace bp
