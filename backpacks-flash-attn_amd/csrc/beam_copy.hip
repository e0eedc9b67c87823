// bp_beam_copy_rows: the caches follow the hypotheses of a beam-search step, ONE launch for all of them.  For every row set
// (base, row stride in bytes, bytes per position; up to 32, passed by value in the kernel arguments -- under graph capture
// they are baked in, which is right because the caches never move) and every row r with parent[r] != r, the bytes of
// positions [first_position, lengths[r]) of row parent[r] are copied to row r.  Rows with parent[r] == r are not touched,
// nor is any byte outside the copied range; a length outside [0, max_positions] is clamped.
//
// The CALLER guarantees parent[parent[r]] == parent[r] (bp_beam_pick's slot rule does): a row that is read is a row that
// names itself, so no source is ever written and a plain copy is correct in place, whatever order the workgroups run in.
//
// Grid (kCopyBlocks, rows, sets): the copied range of a (set, row) is one contiguous run of bytes, at the same offset in
// both rows, so both ends share their alignment: dwords up to the first 16-byte boundary, a 16-byte body strided over the
// workgroups of the run, a dword tail.  Plain vector loads and stores only.
#include "bp_common.h"
#include "bp_kernels.h"

namespace bp {

namespace {
constexpr int kCopyThreads = 256;
constexpr int kCopyBlocks = 8;
}  // namespace

__global__ __launch_bounds__(kCopyThreads) void beam_copy_rows_kernel(const BeamCopyParams p) {
    const int r = blockIdx.y, set = blockIdx.z;
    const int src_row = p.parent[r];
    if (src_row == r || src_row < 0 || src_row >= p.rows) return;   // workgroup-uniform
    int len = p.lengths[r];
    len = len < 0 ? 0 : (len > p.max_positions ? p.max_positions : len);
    if (len <= p.first_position) return;
    const int64_t pos_bytes = p.pos_bytes[set], stride = p.row_stride[set];
    const int64_t begin = (int64_t)p.first_position * pos_bytes, end = (int64_t)len * pos_bytes;   // multiples of 4
    char *dst = static_cast<char *>(p.base[set]) + (int64_t)r * stride;
    const char *src = static_cast<const char *>(p.base[set]) + (int64_t)src_row * stride;
    int64_t body = (begin + 15) & ~(int64_t)15;     // rows start on 16-byte boundaries: offsets align like addresses
    if (body > end) body = end;
    const int64_t tail = body + ((end - body) & ~(int64_t)15);
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {   // at most three dwords on either side
        const int64_t head = begin + 4 * (int64_t)tid;
        if (head < body) *reinterpret_cast<uint32_t *>(dst + head) = *reinterpret_cast<const uint32_t *>(src + head);
        const int64_t t = tail + 4 * (int64_t)tid;
        if (t < end) *reinterpret_cast<uint32_t *>(dst + t) = *reinterpret_cast<const uint32_t *>(src + t);
    }
    for (int64_t o = body + 16 * ((int64_t)blockIdx.x * kCopyThreads + tid); o < tail; o += 16 * (int64_t)kCopyBlocks * kCopyThreads)
        *reinterpret_cast<u32x4 *>(dst + o) = *reinterpret_cast<const u32x4 *>(src + o);
}

hipError_t launch_beam_copy_rows(const BeamCopyParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(beam_copy_rows_kernel, dim3(kCopyBlocks, (unsigned)p.rows, (unsigned)p.nsets), dim3(kCopyThreads), 0,
                       stream, p);
    return hipGetLastError();
}

}  // namespace bp
