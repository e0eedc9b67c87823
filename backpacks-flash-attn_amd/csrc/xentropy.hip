// Fused softmax cross-entropy over vocabulary-sized rows for gfx950 (the
// loss side of the LM head).  Takes the place of the reference's xentropy_cuda_lib.forward / .backward
// (csrc/xentropy/interface.cpp + xentropy_kernel.cu, bound at flash_attn/losses/cross_entropy.py:9,37,54,103):
//
//   forward   lse_i  = log sum_j exp(x_ij)
//             loss_i = (1 - s) (lse_i - x_i[y_i]) + s (lse_i - sum_j x_ij / total_classes)      (s = smoothing)
//             (a label outside [0, cols) contributes no x_i[y_i] term: the vocabulary-parallel caller
//              passes shifted labels, cross_entropy.py:41-63; ignored rows are zeroed by the caller, :39)
//   backward  dx_ij  = g_i (exp(x_ij - lse_i) - (1 - s) [j == y_i] - s / total_classes)
//
// Both are one streaming pass over the logits (HBM-bound: 2 or 4 bytes per element read in forward, read +
// write in backward -- optionally in place, as upstream's inplace_backward).  One 256-thread workgroup per
// row; a thread walks the row in 16-byte chunks with an online (max, sum-of-exp) pair, so there is one
// exp per element and no second pass; the four waves combine through LDS.  The element loads, the strided walk of the row
// (RowSplit) and the two-term merge of (max, sum) partials are vocab_row.h's.
#include "bp_common.h"
#include "bp_kernels.h"
#include "vocab_row.h"

namespace bp {

template <class ET>
__global__ __launch_bounds__(256) void xentropy_fwd_kernel(const XentParams p) {
    using L = RowElem<ET>;
    constexpr int EB = L::EB;
    __shared__ float red[3][4];
    const int64_t row = blockIdx.x;
    const char *x = static_cast<const char *>(p.logits) + row * p.row_stride * EB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // head (elements before the first 16-byte boundary) and tail are walked element-wise by thread 0's wave
    const RowSplit<ET> sp(x, p.cols);   // (in front of the running sums: behind them hipcc allocates the registers differently)
    float m = -INFINITY, s = 0.f, sx = 0.f;
    for (int c = tid; c < sp.nvec; c += 256) {
        float v[8];
        L::load_f32(x + (int64_t)sp.col0(c) * EB, v);
        float cm = v[0];
#pragma unroll
        for (int i = 1; i < L::N; ++i) cm = fmaxf(cm, v[i]);
        if (cm > m) {   // rescale the running sum only when the maximum moves
            s *= fast_exp2((m - cm) * kLog2e);   // m = -inf: s is 0, exp2(-inf) = 0
            m = cm;
        }
        const float mb = (m == -INFINITY) ? 0.f : m * kLog2e;   // a chunk of -inf logits before any finite one
#pragma unroll
        for (int i = 0; i < L::N; ++i) {
            s += fast_exp2(fmaf(v[i], kLog2e, -mb));
            sx += v[i];
        }
    }
    for (int c = tid; c < sp.loose(p.cols); c += 256) {
        const float v = L::one_f32(x + (int64_t)sp.loose_col(c) * EB);
        merge_ms(m, s, v, 1.f);
        sx += v;
    }
    // wave reduction, then across the four waves through LDS
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        merge_ms(m, s, m2, s2);
        sx += __shfl_xor(sx, o);
    }
    if (lane == 0) { red[0][wave] = m; red[1][wave] = s; red[2][wave] = sx; }
    __syncthreads();
    if (tid == 0) {
        m = red[0][0]; s = red[1][0]; sx = red[2][0];
        for (int w = 1; w < 4; ++w) {
            merge_ms(m, s, red[0][w], red[1][w]);
            sx += red[2][w];
        }
        const float lse = m + fast_log2(s) * kLn2;
        const int64_t y = p.labels[row];
        float loss = p.smoothing * (lse - sx / (float)p.total_classes);
        if (y >= 0 && y < p.cols) loss += (1.f - p.smoothing) * (lse - L::one_f32(x + y * EB));
        else if (p.smoothing == 0.f) loss = 0.f;
        p.losses[row] = loss;
        p.lse[row] = lse;
    }
}

template <class ET>
__global__ __launch_bounds__(256) void xentropy_bwd_kernel(const XentParams p) {
    using L = RowElem<ET>;
    constexpr int EB = L::EB;
    const int64_t row = blockIdx.x;
    const char *x = static_cast<const char *>(p.logits) + row * p.row_stride * EB;
    char *dx = static_cast<char *>(p.grad_logits) + row * p.grad_row_stride * EB;
    const int tid = threadIdx.x;
    const float g = p.grad_losses[row];
    const float lse2 = p.lse[row] * kLog2e;
    const int64_t y = p.labels[row];
    const float smooth = p.smoothing / (float)p.total_classes;
    const float hit = 1.f - p.smoothing;

    // x and dx share their alignment when they alias or have equal strides; otherwise go element-wise
    const bool same_phase = ((reinterpret_cast<uintptr_t>(x) ^ reinterpret_cast<uintptr_t>(dx)) & 15) == 0;
    const RowSplit<ET> sp(x, p.cols, same_phase);
    for (int c = tid; c < sp.nvec; c += 256) {
        const int col0 = sp.col0(c);
        float v[8];
        L::load_f32(x + (int64_t)col0 * EB, v);
#pragma unroll
        for (int i = 0; i < L::N; ++i) {
            float d = fast_exp2(fmaf(v[i], kLog2e, -lse2)) - smooth;
            if (col0 + i == y) d -= hit;
            v[i] = g * d;
        }
        L::store_f32(dx + (int64_t)col0 * EB, v);
    }
    for (int c = tid; c < sp.loose(p.cols); c += 256) {
        const int col = sp.loose_col(c);
        float d = fast_exp2(fmaf(L::one_f32(x + (int64_t)col * EB), kLog2e, -lse2)) - smooth;
        if (col == y) d -= hit;
        L::store_one_f32(dx + (int64_t)col * EB, g * d);
    }
}

hipError_t launch_xentropy_fwd(const XentParams &p, int dtype, hipStream_t stream) {
    return with_row_dtype(dtype, [&](auto et) {
        hipLaunchKernelGGL((xentropy_fwd_kernel<decltype(et)>), dim3((unsigned)p.rows), dim3(256), 0, stream, p);
        return hipGetLastError();
    });
}

hipError_t launch_xentropy_bwd(const XentParams &p, int dtype, hipStream_t stream) {
    return with_row_dtype(dtype, [&](auto et) {
        hipLaunchKernelGGL((xentropy_bwd_kernel<decltype(et)>), dim3((unsigned)p.rows), dim3(256), 0, stream, p);
        return hipGetLastError();
    });
}

}  // namespace bp
