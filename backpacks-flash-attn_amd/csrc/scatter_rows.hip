// bp_scatter_packed_rows: the rows of a packed batch land in (batch, positions, ...) buffers -- the prefill of the KV caches
// from packed prompts -- in ONE launch for up to 32 "row sets" (source base, source row stride, destination base, its batch
// and position strides, bytes per row; passed by value in the kernel arguments -- under graph capture they are baked in,
// which is right because neither the caches nor a captured call's inputs move).  For every set, every sample b and every
// position j < min(len_b, max_seqlen, max_positions), len_b = cu_seqlens[b + 1] - cu_seqlens[b], row cu_seqlens[b] + j of
// the source is copied to [b][j] of the destination.  No other byte of a destination is written.
//
// cu_seqlens is read here and nowhere on the host, and it is not trusted: a negative length counts as 0, a length is clamped
// as above, and a source row outside [0, total_rows) is skipped -- whatever it holds, nothing is read outside the sources
// and nothing is written outside [b][0, max_positions).
//
// Grid (position chunks, batch, sets): a workgroup owns kScatterPositions positions of one sample of one set and leaves at
// once when the sample ends in front of them (workgroup-uniform), so no packed row has to search for its sample.  A row is
// copied by the next power of two of lanes at or above its words (at most the workgroup), 256 / lanes rows side by side:
// 16-byte words where the set's bases, strides and row size allow it (the `wide` bit of the set, worked out by the host),
// dwords otherwise (the int32 row index of the Backpack caches is a 4-byte row).  Plain vector loads and stores only.
#include "bp_common.h"
#include "bp_kernels.h"

namespace bp {

namespace {
constexpr int kScatterThreads = 256;

template <typename Word>
__device__ __forceinline__ void scatter_chunk(const char *src, char *dst, int64_t src_stride, int64_t dst_stride,
                                              int64_t row_bytes, int64_t first_row, int64_t total_rows, int npos) {
    const int64_t words = row_bytes / (int64_t)sizeof(Word);
    // lanes of a row: the power of two at or above `words`, at most the workgroup (workgroup-uniform)
    const int shift = words >= kScatterThreads ? 8 : 32 - __clz((int)words - 1);   // words == 1: __clz(0) == 32
    const int lanes = 1 << shift, lane = (int)threadIdx.x & (lanes - 1);
    for (int j = (int)threadIdx.x >> shift; j < npos; j += kScatterThreads >> shift) {
        const int64_t row = first_row + j;
        if (row < 0 || row >= total_rows) continue;
        const Word *from = reinterpret_cast<const Word *>(src + row * src_stride);
        Word *to = reinterpret_cast<Word *>(dst + (int64_t)j * dst_stride);
        for (int64_t w = lane; w < words; w += lanes) to[w] = from[w];
    }
}
}  // namespace

__global__ __launch_bounds__(kScatterThreads) void scatter_packed_rows_kernel(const ScatterRowsParams p) {
    const int b = blockIdx.y, set = blockIdx.z;
    const int64_t begin = p.cu_seqlens[b];
    int64_t len = (int64_t)p.cu_seqlens[b + 1] - begin;
    len = len < p.limit ? len : p.limit;                  // limit = min(max_seqlen, max_positions) >= 0
    const int64_t p0 = (int64_t)blockIdx.x * kScatterPositions;
    if (len <= p0) return;                                // workgroup-uniform: also every negative length
    const int npos = len - p0 < kScatterPositions ? (int)(len - p0) : kScatterPositions;
    const int64_t dst_stride = p.dst_pos_stride[set];
    const char *src = static_cast<const char *>(p.src[set]);
    char *dst = static_cast<char *>(p.dst[set]) + (int64_t)b * p.dst_batch_stride[set] + p0 * dst_stride;
    if ((p.wide >> set) & 1u)
        scatter_chunk<u32x4>(src, dst, p.src_row_stride[set], dst_stride, p.row_bytes[set], begin + p0, p.total_rows, npos);
    else
        scatter_chunk<uint32_t>(src, dst, p.src_row_stride[set], dst_stride, p.row_bytes[set], begin + p0, p.total_rows, npos);
}

hipError_t launch_scatter_packed_rows(const ScatterRowsParams &p, hipStream_t stream) {
    if (p.limit <= 0) return hipSuccess;                  // nothing may be written
    const unsigned chunks = (unsigned)((p.limit + kScatterPositions - 1) / kScatterPositions);
    hipLaunchKernelGGL(scatter_packed_rows_kernel, dim3(chunks, (unsigned)p.batch, (unsigned)p.nsets), dim3(kScatterThreads), 0,
                       stream, p);
    return hipGetLastError();
}

}  // namespace bp
