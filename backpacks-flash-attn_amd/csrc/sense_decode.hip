// bp_sense_decode: the Backpack contraction for ONE new position per sample,
//   o_t = sum_l sum_{j<=t} softmax_j(scale q_l(t).k_l(j)) C_l(x_j),
// against a cache of sense keys, with the sense vectors read from a row table through a cached row index (the whole-
// vocabulary sense table indexed by token ids, or a per-position content cache).  The new position's key and row index
// are appended in the same launch.  The kernels are in decode_core.h (shared with flash_decode.hip).
#include "decode_core.h"

namespace bp {

hipError_t launch_sense_decode(const DecodeParams &p, int dtype, hipStream_t stream) {
    return launch_decode<true>(p, dtype, p.b, stream);
}

hipError_t launch_sense_decode_combine(const DecodeParams &p, int dtype, hipStream_t stream) {
    return with_dtype(dtype, [&](auto et) { return launch_decode_combine<decltype(et), true>(p, p.b, stream); });
}

}  // namespace bp
