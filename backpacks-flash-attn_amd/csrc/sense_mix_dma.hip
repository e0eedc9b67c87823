// Fused Backpack sense combination, LDS-DMA ring version (the fast path for 16-byte-aligned shapes): the fixed-length
// instantiations of sense_mix_dma_kernel (sense_mix_dma_kernel.h: the kernel and its description) -- plain, key-weighted
// and gathering -- and the queue records every persistent sense-mix launch of the library arms (this file's forward, its
// packed form in sense_mix_varlen.hip, dC in sense_mix_bwd.hip).
#include <atomic>

#include "bp_common.h"
#include "bp_dma.h"
#include "bp_kernels.h"
#include "mix_ring.h"

#ifdef BP_MIX_PROFILE
namespace bp {
__device__ unsigned long long g_mix_prof[256][8][12];   // [workgroup][wave][phase 0..5, 6 = clean steps, 7 = job ticks]
}  // namespace bp
#endif

#include "sense_mix_dma_kernel.h"

namespace bp {

// Queue state of a persistent launch: one 64-byte record of device memory, zeroed by a one-wave kernel enqueued right in
// front of the kernel (stream-ordered, so it is captured into a HIP graph with the launch and a launch that died
// cannot leave a stale record behind).  The record belongs to ONE launch until that launch has completed:
//   * callers that capture graphs or run launches concurrently on several streams pass their own record
//     (`queue_ws` of the C ABI; the Python binding always does -- a graph then owns the record it replays);
//   * queue_ws == NULL takes the next record of a small ring owned by the library: enough for eager launches, which
//     can only meet on one record if 64 of them are in flight at once.
constexpr int kMixQueueRing = 64;
__device__ MixQueues g_mix_queues[kMixQueueRing];

static MixQueues *next_queue_record() {
    static std::atomic<unsigned> counter{0};
    thread_local int cached_dev = -1;
    thread_local MixQueues *base = nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    if (dev != cached_dev) {
        void *ptr = nullptr;
        if (hipGetSymbolAddress(&ptr, HIP_SYMBOL(g_mix_queues)) != hipSuccess) return nullptr;
        base = static_cast<MixQueues *>(ptr);
        cached_dev = dev;
    }
    return base + (counter.fetch_add(1u, std::memory_order_relaxed) % kMixQueueRing);
}

__global__ void arm_mix_queues_kernel(MixQueues *queues) {
    if (threadIdx.x < 16) reinterpret_cast<unsigned int *>(queues)[threadIdx.x] = 0u;
}

// shared with the packed launch (sense_mix_varlen.hip) and the dC launch (sense_mix_bwd.hip).  A one-wave KERNEL, not
// hipMemsetAsync: captured into a HIP graph the latter becomes a memset node, and replaying graphs of memset +
// persistent-kernel nodes faulted sporadically on ROCm 7.2 (r03_f: graph replays alone, no eager launch in flight); a
// kernel node in front of a kernel node does not.
hipError_t arm_mix_queues(MixQueues *&queues, hipStream_t stream) {
    if (queues == nullptr) queues = next_queue_record();
    if (queues == nullptr) return hipErrorInvalidDevice;
    hipLaunchKernelGGL(arm_mix_queues_kernel, dim3(1), dim3(64), 0, stream, queues);
    return hipGetLastError();
}

#ifdef BP_MIX_PROFILE
extern "C" int bp_dev_mix_prof(unsigned long long *host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_mix_prof), sizeof(g_mix_prof)) == hipSuccess ? 0 : -1;
}
#endif

// Requires: d_k % 8 == 0, d_out % 8 == 0, all bases 16-byte aligned, all strides multiples of 8, n_qtiles <= 256.
hipError_t launch_sense_mix_dma(const MixParams &params, int dtype, hipStream_t stream) {
    return launch_mix_persistent(params, params.n_qtiles, params.dout, dtype, stream,
                                 [&](auto et, auto kd, auto full, dim3 g, dim3 t, const MixParams &p) {
        using ET = decltype(et);
        if (p.row_index != nullptr)   // (bp_api.hip: never together with key weights)
            hipLaunchKernelGGL((sense_mix_dma_kernel<ET, kd, full, false, true>), g, t, 0, stream, p);
        else if (p.kw != nullptr) hipLaunchKernelGGL((sense_mix_dma_kernel<ET, kd, full, true>), g, t, 0, stream, p);
        else hipLaunchKernelGGL((sense_mix_dma_kernel<ET, kd, full, false>), g, t, 0, stream, p);
    });
}

}  // namespace bp
