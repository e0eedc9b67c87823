// Backward of the fused Backpack sense combination, fixed-length batches (bp_sense_mix_dc, bp_sense_dq_dk): the plain
// instantiations of the kernels of sense_mix_bwd_kernel.h (see there for the algebra and the schedule).  The packed forms
// are a code object of their own, sense_mix_bwd_varlen.hip; this one is not built differently for them.
#include <atomic>

#include "sense_mix_bwd_kernel.h"

namespace bp {

hipError_t launch_sense_mix_dc(const MixBwdParams &params, int dtype, hipStream_t stream) {
    return launch_sense_mix_dc_as<Fixed>(params, dtype, stream);
}

hipError_t launch_sense_dq_dk(const SenseGradParams &p, int dtype, hipStream_t stream) {
    return launch_sense_dq_dk_as<Fixed>(p, dtype, stream);
}

}  // namespace bp
