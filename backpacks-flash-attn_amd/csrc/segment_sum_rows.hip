// bp_segment_sum_rows: acc[u, :] (= or +=) the sum of the 16-bit rows order[seg_begin[u]] .. order[seg_begin[u + 1] - 1], in
// fp32 -- the gradient of a table row is the sum of the gradients of every position that read it (the training order that
// runs the content network once per distinct token).  A pure stream: every row is read once with 16-byte loads, nothing is
// reused, and there is no atomic: every (segment, column) has ONE owner, and the association of its sum is fixed by the
// segment's length alone -- not by the grid, the schedule, or where the segment stands among the others.
//
// Segment lengths are very skewed (most tokens of a batch occur once, a few thousands of times), so there are two roles:
//   short (fewer than kSegLongRows rows, the empty ones too): one workgroup per segment, striding over the segments; a
//     thread owns 8 columns per pass of 2048 and adds the rows in ascending order.
//   long: the segment is cut into column slabs of 128 and every slab goes to a workgroup of its own (96 at k d = 12288), so a
//     long segment is streamed by many CUs at once.  Inside the workgroup 16 row lanes take rows r, r + 16, ... in
//     ascending order each, and the 16 partial sums are added in ascending r through LDS.  Long segments are dealt round
//     robin to kSegLongTeams teams of slab workgroups; every team finds them by scanning seg_begin (256 segments per step).
// Both read up to kSegUnroll rows ahead per thread.  The long workgroups come first in the grid: they carry the most bytes.
//
// Nothing is trusted that lies on the device: seg_begin is clamped to [0, n_rows] (a decreasing pair is an empty segment),
// order unsigned to n_rows - 1, so no read leaves `rows` / `order` and no write leaves rows [0, n_segments) of acc.
#include "bp_common.h"
#include "bp_kernels.h"

namespace bp {

namespace {
constexpr int kSegThreads = 256;
constexpr int kSegUnroll = 8;                                  // rows a thread has in flight
constexpr int kSegColLanes = kSegSlabCols / 8;                 // 16 threads across a slab
constexpr int kSegRowLanes = kSegThreads / kSegColLanes;       // 16 row lanes
constexpr int kSegLongTeams = 8;
static_assert(kSegRowLanes * kSegColLanes == kSegThreads && kSegSlabCols * 2 == kSegThreads, "long-role layout");

template <class ET> BP_DEV void add_row(float (&a)[8], u32x4 w) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t wj = w[j];   // by value, see as_f32
        a[2 * j] += Elem<ET>::lo_f32(wj);
        a[2 * j + 1] += Elem<ET>::hi_f32(wj);
    }
}

BP_DEV u32x4 row_piece(const SegmentSumParams &p, int i, int col) {
    const uint32_t last = (uint32_t)(p.n_rows - 1), given = (uint32_t)p.order[i];
    const int64_t row = given < last ? given : last;
    return ld_global_16B(p.rows + row * p.rows_stride + col);
}

// a += rows order[first], order[first + step], ... (below `end`) at columns [col, col + 8), in that order
template <class ET> BP_DEV void sum_rows(const SegmentSumParams &p, int col, int first, int end, int step, float (&a)[8]) {
    const int n = first < end ? (end - first - 1) / step + 1 : 0;   // counted: no index passes `end`, none overflows
    int t = 0;
    for (; t + kSegUnroll <= n; t += kSegUnroll) {
        u32x4 w[kSegUnroll];
#pragma unroll
        for (int u = 0; u < kSegUnroll; ++u) w[u] = row_piece(p, first + (t + u) * step, col);
#pragma unroll
        for (int u = 0; u < kSegUnroll; ++u) add_row<ET>(a, w[u]);
    }
    for (; t < n; ++t) add_row<ET>(a, row_piece(p, first + t * step, col));
}

BP_DEV void segment_bounds(const SegmentSumParams &p, int u, int &begin, int &end) {
    const int b = p.seg_begin[u], e = p.seg_begin[u + 1];
    begin = b < 0 ? 0 : b > p.n_rows ? p.n_rows : b;
    end = e < begin ? begin : e > p.n_rows ? p.n_rows : e;
}

template <class ET> BP_DEV void short_segments(const SegmentSumParams &p, int first, int stride) {
    for (int u = first; u < p.n_segments; u += stride) {
        int begin, end;
        segment_bounds(p, u, begin, end);
        if (end - begin >= kSegLongRows || (end == begin && p.accumulate)) continue;   // workgroup-uniform
        float *dst = p.acc + (int64_t)u * p.acc_stride;
        for (int col = (int)threadIdx.x * 8; col < p.cols; col += kSegThreads * 8) {
            float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            sum_rows<ET>(p, col, begin, end, 1, a);
            f32x4 lo = {a[0], a[1], a[2], a[3]}, hi = {a[4], a[5], a[6], a[7]};
            f32x4 *out = reinterpret_cast<f32x4 *>(dst + col);
            if (p.accumulate) {
                lo += out[0];
                hi += out[1];
            }
            out[0] = lo;
            out[1] = hi;
        }
    }
}

template <class ET> BP_DEV void long_segment_slab(const SegmentSumParams &p, int u, int slab, float (*part)[kSegSlabCols]) {
    int begin, end;
    segment_bounds(p, u, begin, end);
    const int r = (int)threadIdx.x / kSegColLanes, c = (int)threadIdx.x % kSegColLanes;
    const int col = slab * kSegSlabCols + c * 8;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (col < p.cols) sum_rows<ET>(p, col, begin + r, end, kSegRowLanes, a);
#pragma unroll
    for (int j = 0; j < 8; ++j) part[r][c * 8 + j] = a[j];
    __syncthreads();
    const int mine = slab * kSegSlabCols + (int)threadIdx.x;
    if ((int)threadIdx.x < kSegSlabCols && mine < p.cols) {
        float sum = part[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < kSegRowLanes; ++k) sum += part[k][threadIdx.x];
        float *dst = p.acc + (int64_t)u * p.acc_stride + mine;
        *dst = p.accumulate ? *dst + sum : sum;
    }
    __syncthreads();
}

template <class ET> BP_DEV void long_segments(const SegmentSumParams &p, int team, int slab) {
    __shared__ float part[kSegRowLanes][kSegSlabCols];
    __shared__ uint32_t found[kSegThreads / 64][2];
    int nlong = 0;
    for (int base = 0; base < p.n_segments; base += kSegThreads) {
        const int u = base + (int)threadIdx.x;
        bool is_long = false;
        if (u < p.n_segments) {
            int begin, end;
            segment_bounds(p, u, begin, end);
            is_long = end - begin >= kSegLongRows;
        }
        const uint64_t mask = __ballot(is_long);
        if ((threadIdx.x & 63) == 0) {
            found[threadIdx.x >> 6][0] = (uint32_t)mask;
            found[threadIdx.x >> 6][1] = (uint32_t)(mask >> 32);
        }
        __syncthreads();
        for (int w = 0; w < kSegThreads / 32; ++w) {
            // the same in every lane: made scalar, so that the barriers below stand in uniform control flow
            uint32_t bits = __builtin_amdgcn_readfirstlane(found[w >> 1][w & 1]);
            while (bits) {
                const int bit = __builtin_ctz(bits);
                bits &= bits - 1;
                if (nlong++ % kSegLongTeams == team) long_segment_slab<ET>(p, base + w * 32 + bit, slab, part);
            }
        }
        __syncthreads();   // `found` is rewritten by the next step
    }
}
}  // namespace

template <class ET> __global__ __launch_bounds__(kSegThreads) void segment_sum_rows_kernel(const SegmentSumParams p) {
    const int n_long = kSegLongTeams * p.n_slabs, block = (int)blockIdx.x;
    if (block < n_long)
        long_segments<ET>(p, block / p.n_slabs, block % p.n_slabs);
    else
        short_segments<ET>(p, block - n_long, (int)gridDim.x - n_long);
}

hipError_t launch_segment_sum_rows(SegmentSumParams p, int dtype, hipStream_t stream) {
    if (p.n_segments <= 0) return hipSuccess;
    p.n_slabs = (p.cols + kSegSlabCols - 1) / kSegSlabCols;
    const int short_wgs = p.n_segments < 2048 ? p.n_segments : 2048;
    const dim3 grid((unsigned)(kSegLongTeams * p.n_slabs + short_wgs));
    if (dtype == 1)
        hipLaunchKernelGGL(segment_sum_rows_kernel<BF16>, grid, dim3(kSegThreads), 0, stream, p);
    else
        hipLaunchKernelGGL(segment_sum_rows_kernel<F16>, grid, dim3(kSegThreads), 0, stream, p);
    return hipGetLastError();
}

}  // namespace bp
