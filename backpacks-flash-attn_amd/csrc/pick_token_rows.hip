// bp_pick_token_lim_rows: bp_pick_token_lim with penalty_begin and min_length per row, for a batch whose prompts differ in length
// (src/utils/generation.py: prompt_lengths).  The kernel is pick_core.h's with its row-limited flag, in a code object of its
// own: pick_token.hip's, pick_token_ctl.hip's and pick_token_lim.hip's stay what they were.
#include "pick_core.h"

namespace bp {

hipError_t launch_pick_token_rows(const PickParams &p, int dtype, hipStream_t stream) {
    const size_t lds = (size_t)LimLayout(p).total_words * 4;   // the limited form's: the arrays add nothing to it
    auto go = [&](auto et) {
        auto kernel = pick_token_kernel<RowLimited<decltype(et)>>;
        if (lds > 48 * 1024) {   // ask for the large dynamic allocation by name
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kernel, dim3((unsigned)p.batch), dim3(kPickThreads), lds, stream, p);
        return hipGetLastError();
    };
    if (dtype == BP_DTYPE_F32) return go(float{});
    return with_dtype(dtype, go);
}

}  // namespace bp
