// bp_pick_report: what the model thought of the token a decode step just picked -- its log-probability and rank, the
// entropy of the row, and the n most likely tokens with their log-probabilities -- written into column counters[b] of
// per-row record buffers, the column contract of the pick kernels (pick_core.h).  Takes the place of the host-side
// log_softmax / topk readouts of the reference's scripts (training/src/interactive.py and modulate_generate.py: print_topk;
// training/src/test_topic.py: the likelihood of a generation), which need a row of logits on the host that the captured
// decode step never produces.  The contract is the comment of bp_pick_report in include/bp_hip.h; _eager_report
// (src/utils/generation.py) and tests/pick_report_ref.py restate it.  The row reader (RowView, RowElem), the argmax key
// (greedy_key) and the (m, s, t) statistics are vocab_row.h's.
//
// One 1024-thread workgroup per row, 16-byte loads, a row whose counter lies outside [0, rec_cols) returns at once.
//   pass 1    the statistics of bp_score_rows with one target, per lane and online: (m, s, t) = the maximum, sum e^(x - m) and
//             sum e^(x - m) x, rescaled only when the maximum moves; the count of elements in front of the token in the order
//             of the ranks (x > x_t, or x == x_t at a lower column); and the maximum of the 64-bit key
//             (greedy_key(x) << 32) | ~column -- the greedy token, top position 0, and the NaN flag of the row.
//             Lanes combine through shuffles, the 16 waves through LDS, every thread in the same fixed order.
//   pass i    for i = 1 .. n_top - 1: the maximum of the keys strictly below the key of position i - 1.  The keys are
//             distinct (the columns are), so position i is unique; thread i keeps it.
// Then thread 0 stores the three scalars and thread i < n_top the i-th alternative: its column, and float(x) - lse with x
// read again from the row (the key does not tell -0 from +0).
// Algorithmic bytes: the row max(1, n_top) times -- once from wherever the LM-head GEMM left it, the rest from L2 -- plus at
// most 12 + 8 n_top bytes of stores per row.  No global workspace, no global atomics, vector stores only; every loop is
// bounded by the row's steps or by n_top; no register array is indexed by a variable.
#include "bp_kernels.h"
#include "vocab_row.h"

namespace bp {

namespace {

struct ReportShared {
    float m[kPickWaves], s[kPickWaves], t[kPickWaves];
    int cnt[kPickWaves];
    u64 key[2][kPickWaves];   // by the parity of the pass: a pass writes while a slow wave may still read the previous one
};

// the maximum over the workgroup of a 64-bit key, to every thread; `slot` alternates between consecutive calls
BP_DEV u64 report_block_max(ReportShared &sh, int slot, u64 v, int lane, int wave) {
    v = wave_max_u64(v);
    if (lane == 0) sh.key[slot][wave] = v;
    __syncthreads();
    v = sh.key[slot][0];
#pragma unroll
    for (int w = 1; w < kPickWaves; ++w) v = sh.key[slot][w] > v ? sh.key[slot][w] : v;
    return v;
}

}  // namespace

template <class ET>
__global__ __launch_bounds__(kPickThreads) void pick_report_kernel(const PickReportParams p) {
    using E = RowElem<ET>;
    __shared__ ReportShared sh;
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = p.counters[b];
    if (c < 0 || c >= p.rec_cols) return;   // workgroup-uniform: no column of the record, as for `sequences` in the pick
    const char *base = static_cast<const char *>(p.logits) + (int64_t)b * p.row_stride * E::EB;
    const RowView<ET> row(base, p.vocab);

    // the token: a uniform load, before the row is walked
    int tc = -1;
    float xt = __builtin_nanf("");
    const int64_t y = p.tokens[(int64_t)b * p.tokens_stride];
    if (y >= 0 && y < (int64_t)p.vocab) {
        tc = (int)y;
        xt = E::to_f32(E::one(base + y * E::EB));
    }

    // ---- pass 1
    float m = -INFINITY, s = 0.f, t = 0.f;
    int cnt = 0;
    u64 best = 0;
    for (int st = 0; st < row.steps(); ++st) {
        const int ch = row.chunk(wave, st, lane);
        if (ch < 0) continue;
        uint32_t raw[8], mask;
        const int col0 = row.load(ch, raw, mask);
        float v[E::N];
        float cm = -INFINITY;
#pragma unroll
        for (int i = 0; i < E::N; ++i) {
            v[i] = ((mask >> i) & 1u) ? E::to_f32(raw[i]) : -INFINITY;   // outside the row: adds nothing to s and t
            cm = fmaxf(cm, v[i]);
        }
        if (cm > m) online_rescale(m, s, t, cm);   // the maximum moves
        const float ms = online_shift(m);
        float cs = 0.f, ct = 0.f;
#pragma unroll
        for (int i = 0; i < E::N; ++i) {
            online_term(v[i], ms, cs, ct);
            const bool valid = (mask >> i) & 1u;
            cnt += (valid && (v[i] > xt || (v[i] == xt && col0 + i < tc))) ? 1 : 0;
            const u64 k = ((u64)greedy_key(v[i]) << 32) | (uint32_t)~(uint32_t)(col0 + i);
            if (valid && k > best) best = k;
        }
        s += cs;
        t += ct;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o), t2 = __shfl_xor(t, o);
        merge_mst(m, s, t, m2, s2, t2);
        cnt += __shfl_xor(cnt, o);
    }
    if (lane == 0) { sh.m[wave] = m; sh.s[wave] = s; sh.t[wave] = t; sh.cnt[wave] = cnt; }
    best = report_block_max(sh, 0, best, lane, wave);   // (its barrier also publishes m, s, t, cnt)
    m = sh.m[0]; s = sh.s[0]; t = sh.t[0]; cnt = sh.cnt[0];
#pragma unroll
    for (int w = 1; w < kPickWaves; ++w) {
        merge_mst(m, s, t, sh.m[w], sh.s[w], sh.t[w]);
        cnt += sh.cnt[w];
    }
    // The degenerate rows, by the arithmetic of the definitions (bp_score_rows): a NaN makes everything NaN; +inf gives
    // lse = +inf and a NaN entropy; a row of -inf gives lse = -inf and again a NaN entropy.
    const bool has_nan = (uint32_t)(best >> 32) == 0xffffffffu;
    const float nan = __builtin_nanf("");
    float lse = m + logf(s), entropy = lse - t / s;   // once a row: the library's logarithm
    if (has_nan) { lse = nan; entropy = nan; }
    else if (m == INFINITY || m == -INFINITY) { lse = m; entropy = nan; }

    // ---- passes 2 .. n_top: the largest key strictly below the last one found
    u64 mine = best, bound = best;
    for (int i = 1; i < p.n_top; ++i) {
        u64 next = 0;
        for (int st = 0; st < row.steps(); ++st) {
            const int ch = row.chunk(wave, st, lane);
            if (ch < 0) continue;
            uint32_t raw[8], mask;
            const int col0 = row.load(ch, raw, mask);
#pragma unroll
            for (int j = 0; j < E::N; ++j) {
                const u64 k = ((u64)greedy_key(E::to_f32(raw[j])) << 32) | (uint32_t)~(uint32_t)(col0 + j);
                if (((mask >> j) & 1u) && k < bound && k > next) next = k;
            }
        }
        bound = report_block_max(sh, i & 1, next, lane, wave);
        if (tid == i) mine = bound;
    }

    const int64_t at = (int64_t)b * p.rec_stride + c;
    if (tid == 0) {
        if (p.logprob) p.logprob[at] = tc < 0 ? 0.f : xt - lse;
        if (p.rank) p.rank[at] = tc < 0 ? -1 : cnt;
        if (p.entropy) p.entropy[at] = entropy;
    }
    if (tid < p.n_top) {
        const int col = (int)~(uint32_t)mine;
        if (col < 0 || col >= p.vocab) return;   // cannot happen (n_top <= vocab distinct keys); never read outside the row
        if (p.top_idx) p.top_idx[at * p.n_top + tid] = col;
        if (p.top_logprob) p.top_logprob[at * p.n_top + tid] = E::to_f32(E::one(base + (int64_t)col * E::EB)) - lse;
    }
}

hipError_t launch_pick_report(const PickReportParams &p, int dtype, hipStream_t stream) {
    auto go = [&](auto et) {
        hipLaunchKernelGGL((pick_report_kernel<decltype(et)>), dim3((unsigned)p.rows), dim3(kPickThreads), 0, stream, p);
        return hipGetLastError();
    };
    return with_row_dtype(dtype, go);
}

}  // namespace bp
