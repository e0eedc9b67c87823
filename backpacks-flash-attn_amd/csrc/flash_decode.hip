// bp_flash_decode: trunk attention of ONE new query row per (sample, head) against the KV cache of the reference's
// generation contract ((max_batch, max_seqlen, 2, nheads, head_dim), flash_attn/modules/mha.py _update_kv_cache),
// with the new token's K/V appended in the same launch.  The kernels are in decode_core.h (shared with sense_decode.hip).
#include "decode_core.h"

namespace bp {

int decode_nsplit(int batch, int groups, int max_seqlen) { return decode_nsplit_impl(batch, groups, max_seqlen); }

hipError_t launch_flash_decode(const DecodeParams &p, int dtype, hipStream_t stream) {
    return launch_decode<false>(p, dtype, p.b * p.groups, stream);
}

}  // namespace bp
