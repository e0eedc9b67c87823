// Scoring of vocabulary-sized rows for gfx950: everything an evaluation keeps of a row of logits, in ONE streaming pass.
// Takes the place of the torch composition behind the reference's evaluation metrics (training/src/metrics/perplexity.py,
// accuracy.py, tasks/seq.py; the p(' he') / p(' she') readout of training/src/test_genderbias.py:187-203): an fp32
// log_softmax over (tokens, vocab), a gather, an argmax, a comparison count and an entropy pass.  The contract is the comment
// of bp_score_rows in include/bp_hip.h; _eager_score_rows (src/utils/scoring.py) and tests/score_ref.py restate it.
//
// One 256-thread workgroup per row, as xentropy_fwd_kernel: a thread walks the row in 16-byte chunks (head and tail
// element-wise; vocab_row.h: RowSplit), ascending in the column.  It keeps
//   (m, s, t)   the online maximum, s = sum e^(x - m), t = sum e^(x - m) x, rescaled only when the maximum moves
//   best        the column of the first maximum it met (found inside the chunk only when the maximum moves; a thread that met
//               only -inf answers with the first column it walked)
//   nan_col     the column of the first NaN it met (looked for only in a chunk whose sum of exponentials is a NaN)
//   cnt[M]      per target, the elements that precede it in the order of the ranks: x > x_t, or x == x_t at a lower column.
//               A chunk wholly below the target's column counts x >= x_t, one wholly above it x > x_t: one comparison an
//               element; only the chunk that holds the column compares twice.  With one target the loop over the body is split
//               at that chunk into three loops without a branch in their bodies.
// The target values are uniform loads in front of the loop.  The waves combine through shuffles, the four waves through LDS.
// Algorithmic bytes: the row, once.  M = 1 is an instantiation of its own; 2 .. 8 targets share the general form.
#include <climits>

#include "bp_common.h"
#include "bp_kernels.h"
#include "vocab_row.h"

namespace bp {

namespace {

constexpr int kNoCol = INT_MAX;
constexpr int kAny = 0, kBelow = 1, kAbove = 2;   // ScoreState::absorb

// What a thread, a wave and the row know.  M targets: tc[] their columns (-1: out of range), xt[] their values (NaN then).
template <int MT> struct ScoreState {
    float m = -INFINITY, s = 0.f, t = 0.f;   // rescaled only when the maximum moves
    int best = kNoCol, nan_col = kNoCol;
    int cnt[MT];

    // NE elements v[0 .. NE) at the columns col0 .. col0 + NE - 1, all inside the row.  MODE: how the chunk lies to the target
    // columns -- kBelow: wholly below every one of them, kAbove: wholly above, kAny: looked at per target
    template <int NE, int MODE>
    BP_DEV void absorb(const float (&v)[8], int col0, int ntargets, const int (&tc)[MT], const float (&xt)[MT]) {
        float cm = v[0];
#pragma unroll
        for (int i = 1; i < NE; ++i) cm = fmaxf(cm, v[i]);
        if (cm > m) {   // the maximum moves: rescale, and find its first column in the chunk
            online_rescale(m, s, t, cm);
            int at = NE - 1;
#pragma unroll
            for (int i = NE - 2; i >= 0; --i) at = v[i] == cm ? i : at;
            best = col0 + at;
        }
        // straight-line from here to the NaN check: the comparisons fill the issue slots behind the exponentials
        const float ms = online_shift(m);
        float cs = 0.f, ct = 0.f;
#pragma unroll
        for (int i = 0; i < NE; ++i) online_term(v[i], ms, cs, ct);
#pragma unroll
        for (int k = 0; k < MT; ++k) {
            if (MT > 1 && k >= ntargets) break;
            const int tp = tc[k] - col0;   // where the target sits in the chunk
            const float x = xt[k];
            int c = 0;
            if (MODE == kBelow || (MODE == kAny && tp >= NE)) {
#pragma unroll
                for (int i = 0; i < NE; ++i) c += v[i] >= x ? 1 : 0;
            } else if (MODE == kAbove || tp < 0) {
#pragma unroll
                for (int i = 0; i < NE; ++i) c += v[i] > x ? 1 : 0;
            } else {
#pragma unroll
                for (int i = 0; i < NE; ++i) c += (v[i] > x || (v[i] == x && i < tp)) ? 1 : 0;
            }
            cnt[k] += c;
        }
        s += cs;
        t += ct;
        if (cs != cs && nan_col == kNoCol) {   // a NaN element, or a +inf one (then the row is degenerate anyway)
#pragma unroll
            for (int i = NE - 1; i >= 0; --i) nan_col = v[i] != v[i] ? col0 + i : nan_col;
        }
    }

    // first: the first column this thread walked (kNoCol: none).  A thread that met nothing above -inf holds a maximum there.
    BP_DEV u64 key(int first) const {
        if (nan_col != kNoCol) return ((u64)0xffffffffu << 32) | (uint32_t)~(uint32_t)nan_col;
        return ((u64)order_key(m) << 32) | (uint32_t)~(uint32_t)(best == kNoCol ? first : best);
    }
};

}  // namespace

template <class ET, int MT>
__global__ __launch_bounds__(256) void score_rows_kernel(const ScoreParams p) {
    using L = RowElem<ET>;
    constexpr int EB = L::EB, N = L::N;
    __shared__ float red_f[3][4];
    __shared__ u64 red_k[4];
    __shared__ int red_c[MT][4];
    const int64_t row = blockIdx.x;
    const char *x = static_cast<const char *>(p.logits) + row * p.row_stride * EB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntargets = MT == 1 ? 1 : p.ntargets;
    const RowSplit<ET> sp(x, p.cols);   // (in front of the running state: behind it hipcc allocates the registers differently)

    // the targets: uniform loads, before the row is touched
    int tc[MT];
    float xt[MT];
    ScoreState<MT> st;
#pragma unroll
    for (int k = 0; k < MT; ++k) {
        st.cnt[k] = 0;
        tc[k] = -1;
        xt[k] = __builtin_nanf("");
        if (k < ntargets) {
            const int64_t y = p.targets[row * p.target_stride + k];
            if (y >= 0 && y < (int64_t)p.cols) {
                tc[k] = (int)y;
                xt[k] = L::one_f32(x + y * EB);
            }
        }
    }

    // head: the elements before the first 16-byte boundary; then the vector body; then the tail -- ascending for every thread
    const int nhead = sp.nhead, nvec = sp.nvec, tail0 = sp.tail0;
    float v[8];
    if (tid < nhead) {
        v[0] = L::one_f32(x + (int64_t)tid * EB);
        st.template absorb<1, kAny>(v, tid, ntargets, tc, xt);
    }
    int c = tid;
    if constexpr (MT == 1) {
        // One target: a thread's chunks ascend, so they lie below the target's chunk, then (for one thread) on it, then above
        // it -- three loops whose bodies are straight-line code with one comparison an element.
        const int at = tc[0] >= nhead ? (tc[0] - nhead) / N : -1;   // the body chunk of the target; nvec or more: it is in the tail
        const int below = min(at, nvec);
        for (; c < below; c += 256) {
            const int col0 = sp.col0(c);
            L::load_f32(x + (int64_t)col0 * EB, v);
            st.template absorb<N, kBelow>(v, col0, ntargets, tc, xt);
        }
        if (c == at && c < nvec) {
            const int col0 = sp.col0(c);
            L::load_f32(x + (int64_t)col0 * EB, v);
            st.template absorb<N, kAny>(v, col0, ntargets, tc, xt);
            c += 256;
        }
        for (; c < nvec; c += 256) {
            const int col0 = sp.col0(c);
            L::load_f32(x + (int64_t)col0 * EB, v);
            st.template absorb<N, kAbove>(v, col0, ntargets, tc, xt);
        }
    } else {
        for (; c < nvec; c += 256) {
            const int col0 = sp.col0(c);
            L::load_f32(x + (int64_t)col0 * EB, v);
            st.template absorb<N, kAny>(v, col0, ntargets, tc, xt);
        }
    }
    if (tid < p.cols - tail0) {
        v[0] = L::one_f32(x + (int64_t)(tail0 + tid) * EB);
        st.template absorb<1, kAny>(v, tail0 + tid, ntargets, tc, xt);
    }

    // wave reduction, then across the four waves through LDS
    float m = st.m, s = st.s, t = st.t;
    const int first = tid < nhead ? tid : tid < nvec ? nhead + tid * N : tid < p.cols - tail0 ? tail0 + tid : kNoCol;
    u64 key = st.key(first);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o), t2 = __shfl_xor(t, o);
        merge_mst(m, s, t, m2, s2, t2);
        const u64 k2 = shfl_xor_u64(key, o);
        key = k2 > key ? k2 : key;
#pragma unroll
        for (int k = 0; k < MT; ++k) st.cnt[k] += __shfl_xor(st.cnt[k], o);
    }
    if (lane == 0) {
        red_f[0][wave] = m; red_f[1][wave] = s; red_f[2][wave] = t;
        red_k[wave] = key;
#pragma unroll
        for (int k = 0; k < MT; ++k) red_c[k][wave] = st.cnt[k];
    }
    __syncthreads();
    if (tid >= ntargets && tid != 0) return;
    m = red_f[0][0]; s = red_f[1][0]; t = red_f[2][0];
    key = red_k[0];
    for (int w = 1; w < 4; ++w) {
        merge_mst(m, s, t, red_f[0][w], red_f[1][w], red_f[2][w]);
        key = red_k[w] > key ? red_k[w] : key;
    }
    // The degenerate rows, by the arithmetic of the definitions: a NaN makes all three NaN; +inf gives lse = +inf and
    // exp(inf - inf) = NaN in the entropy; a row of -inf gives lse = -inf and again a NaN entropy.
    const bool has_nan = (uint32_t)(key >> 32) == 0xffffffffu;
    const float nan = __builtin_nanf("");
    float lse = m + logf(s), entropy = lse - t / s;   // once a row: the library's logarithm, not v_log_f32
    if (has_nan) { lse = nan; entropy = nan; }
    else if (m == INFINITY || m == -INFINITY) { lse = m; entropy = nan; }
    if (tid == 0) {
        if (p.lse) p.lse[row] = lse;
        if (p.entropy) p.entropy[row] = entropy;
        if (p.top1) p.top1[row] = (int)~(uint32_t)key;
    }
    if (tid < ntargets) {
        // this thread's target: a select chain over registers (no indexed private array)
        int col = tc[0], count = 0;
        float xv = xt[0];
#pragma unroll
        for (int k = 0; k < MT; ++k) {
            const int c = red_c[k][0] + red_c[k][1] + red_c[k][2] + red_c[k][3];
            if (k == tid) { col = tc[k]; xv = xt[k]; count = c; }
        }
        const int64_t o = row * p.out_stride + tid;
        if (p.logprob) p.logprob[o] = col < 0 ? 0.f : xv - lse;
        if (p.rank) p.rank[o] = col < 0 ? -1 : count;
    }
}

hipError_t launch_score_rows(const ScoreParams &p, int dtype, hipStream_t stream) {
    auto go = [&](auto et) {
        using ET = decltype(et);
        if (p.ntargets == 1)
            hipLaunchKernelGGL((score_rows_kernel<ET, 1>), dim3((unsigned)p.rows), dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL((score_rows_kernel<ET, kScoreMaxTargets>), dim3((unsigned)p.rows), dim3(256), 0, stream, p);
        return hipGetLastError();
    };
    return with_row_dtype(dtype, go);
}

}  // namespace bp
