// bp_sense_decode_weighted: bp_sense_decode with a per-(sample, sense, key) fp32 weight on the probabilities,
//   o_t = sum_l sum_{j<=t} softmax_j(scale q_l(t).k_l(j)) w[l, j] C_l(x_j)
// (the intervened Backpacks of src/models/intervened_models.py on a KV cache).  The split kernel is decode_core.h's with
// its weighted flag, in a code object of its own: sense_decode.hip's stays what it was.  The combine does not know about
// weights and is the one of sense_decode.hip.
#include "decode_core.h"

namespace bp {

hipError_t launch_sense_decode_weighted(const DecodeParams &p, int dtype, hipStream_t stream) {
    // the senses' width buckets, as launch_decode
    const hipError_t e = with_dtype(dtype, [&](auto et) {
        return with_bound<1, 2, 4, 8, 16, 32, 64, 128>(p.dk >> 3, hipErrorNotSupported, [&](auto qc) {
            constexpr int G = qc < 64 ? int(qc) : 64;
            hipLaunchKernelGGL((decode_split_kernel<Weighted<decltype(et)>, G, qc / G, true>), dim3(p.nsplit, p.groups, p.b),
                               dim3(DEC_THREADS), 0, stream, p);
            return hipGetLastError();
        });
    });
    return e != hipSuccess ? e : launch_sense_decode_combine(p, dtype, stream);
}

}  // namespace bp
