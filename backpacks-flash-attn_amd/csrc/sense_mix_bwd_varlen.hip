// Backward of the fused Backpack sense combination on PACKED batches (bp_sense_mix_dc_varlen, bp_sense_dq_dk_varlen): the
// Varlen<ET> instantiations of sense_mix_dc_kernel, sense_dq_kernel and sense_dk_kernel (sense_mix_bwd_kernel.h) as a code
// object of their own -- the fixed-length kernels of sense_mix_bwd.hip are not rebuilt differently for them.  The dP^T
// slab these read is written by sense_dp_slab_varlen.hip.
//
// Requires: p.cu != NULL, d_k % 8 == 0, d_out % 8 == 0, all bases 16-byte aligned, all strides multiples of 8 (dk_acc:
// of 4), n_ktiles <= 256, p.s = max_seqlen.
#include "sense_mix_bwd_kernel.h"

namespace bp {

hipError_t launch_sense_mix_dc_varlen(const MixBwdParams &params, int dtype, hipStream_t stream) {
    return launch_sense_mix_dc_as<Varlen>(params, dtype, stream);
}

hipError_t launch_sense_dq_dk_varlen(const SenseGradParams &p, int dtype, hipStream_t stream) {
    return launch_sense_dq_dk_as<Varlen>(p, dtype, stream);
}

}  // namespace bp
