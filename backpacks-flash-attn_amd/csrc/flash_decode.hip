// bp_flash_decode: trunk attention of ONE new query row per (sample, head) against the KV cache of the reference's
// generation contract ((max_batch, max_seqlen, 2, nheads, head_dim), flash_attn/modules/mha.py _update_kv_cache),
// with the new token's K/V appended in the same launch.  The kernels are in decode_core.h (shared with sense_decode.hip).
#include "decode_core.h"

namespace bp {

int decode_nsplit(int batch, int groups, int max_seqlen) { return decode_nsplit_impl(batch, groups, max_seqlen); }

hipError_t launch_flash_decode(const DecodeParams &p, int dtype, hipStream_t stream) {
    const int nout = p.b * p.groups;
    return dtype == 1 ? launch_decode_dtype<BF16, false>(p, nout, stream) : launch_decode_dtype<F16, false>(p, nout, stream);
}

}  // namespace bp
