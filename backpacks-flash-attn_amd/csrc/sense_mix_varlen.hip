// Fused Backpack sense combination on PACKED batches (bp_sense_mix_varlen, bp_sense_mix_gather_varlen): the
// Varlen<ET> instantiations of sense_mix_dma_kernel (sense_mix_dma_kernel.h), plain and gathering, as a code object of
// their own -- the fixed-length kernels of sense_mix_dma.hip are not rebuilt differently for them.  The queue record is
// armed by arm_mix_queues (sense_mix_dma.hip).
#include "bp_common.h"
#include "bp_dma.h"
#include "bp_kernels.h"
#include "mix_ring.h"
#undef BP_MIX_PROFILE   // development builds: the phase counters belong to the fixed-length object (sense_mix_dma.hip)
#include "sense_mix_dma_kernel.h"

namespace bp {

// Requires: p.cu != NULL, d_k % 8 == 0, d_out % 8 == 0, all bases 16-byte aligned, all strides multiples of 8,
// n_qtiles <= 256; the gathering form (row_index != NULL) max_seqlen <= kMixGatherMaxKeys and at most kMixGatherMaxRows
// table rows.
// p.cu lives in the slot of p.kw (the union in bp_kernels.h), so p.kw is non-NULL in EVERY packed launch: nothing here, and
// nothing that receives these params, may pick a weighted form from `p.kw != nullptr` (launch_sense_mix_dma does, for the
// fixed-length launches only).
hipError_t launch_sense_mix_varlen(const MixParams &params, int dtype, hipStream_t stream) {
    return launch_mix_persistent(params, params.n_qtiles, params.dout, dtype, stream,
                                 [&](auto et, auto kd, auto full, dim3 g, dim3 t, const MixParams &p) {
        using TAG = Varlen<decltype(et)>;
        if (p.row_index != nullptr) hipLaunchKernelGGL((sense_mix_dma_kernel<TAG, kd, full, false, true>), g, t, 0, stream, p);
        else hipLaunchKernelGGL((sense_mix_dma_kernel<TAG, kd, full, false>), g, t, 0, stream, p);
    });
}

}  // namespace bp
