// bp_row_extremes: the n largest and the n smallest elements of every row of a (rows, cols) matrix, values and columns, in
// order.  Built for the vocabulary projections of sense vectors (src/utils/sense_vocab.py): a chunk of C_l(v) @ E^T is
// reduced to its two ends the moment the GEMM has written it, so the (V k, V) matrix never exists as a whole.  The row
// reader (RowView, RowElem) and the wave helpers are vocab_row.h's.
//
// Contract (restated by _eager_row_extremes, src/utils/sense_vocab.py, and by tests/sense_vocab_ref.py):
//   key       the order-preserving integer key of an element's RAW bits (RowElem<ET>::key): -0 < +0, NaNs at the ends by sign
//   largest   ranked by (key descending, column ascending); smallest by (key ascending, column ascending)
//   outputs   (rows, n) dense: *_val = float(element) fp32, *_idx = its column int32; an end whose two pointers are NULL is
//             skipped.  A total order on integers: the answer is unique and two calls give the same bits.
//
// One 1024-thread workgroup per row; the first pass reads the row from HBM, the later ones find it in L2.
//   n == 1    ONE pass, four chunks in flight per lane: the lane's extremes on 32-bit keys, then the maximum of (key, ~column)
//             and of (~key, ~column) as 64-bit integers over the wave and over the 16 waves
//   n >= 2    1  radix select, 8 bits a round from the top of the key (two rounds for 16-bit rows, four for fp32), BOTH ends
//                in the same pass: round 0 fills one histogram (32 copies of 256 bins, copy stride 257, as the pick's) that
//                the top end reads downwards and the bottom end upwards; later rounds fill one histogram per end (16 copies
//                each) with the elements of that end's bucket.  Wave 0 finds the top digit, wave 1 the bottom one.  Result
//                per end: the threshold key K and the count beyond it, which is < n.
//             2  one collecting pass: an element strictly beyond K takes a slot of the end's list by an LDS counter (fewer
//                than n of them, their order does not matter); the ties at K are taken in VOCABULARY order -- wave w owns a
//                contiguous run of chunks, so a wave numbers its ties with a prefix count over its lanes per step and parks the
//                columns of its first (n - beyond) ones; the waves' counts then give every parked tie its rank in the row
//             3  wave 0 (top) and wave 1 (bottom) rank the n held (key, ~column) values by counting and store them in order
// No global workspace, no global atomics, vector stores only.  Every loop is bounded by the row's steps, by n or by a
// constant; no register array is indexed by a variable.
#include "bp_kernels.h"
#include "vocab_row.h"

namespace bp {

namespace {

constexpr int kExtMax = kRowExtremesMaxN;

struct ExtShared {
    uint32_t hist[kHistCopies * kHistStride];
    uint32_t bins[2][256];
    u64 items[2][kExtMax];
    uint32_t tie_col[2][kPickWaves][kExtMax];
    uint32_t tie_cnt[2][kPickWaves];
    u64 wave64[2][kPickWaves];
    uint32_t n_items[2];
    uint32_t sel_digit[2], sel_above[2];
};

// an element strictly beyond the threshold: any free slot of the end's list (fewer than n <= kExtMax reach here)
BP_DEV void ext_push(ExtShared &sh, int e, uint32_t ordered, int col) {
    const uint32_t slot = atomicAdd(&sh.n_items[e], 1u);
    if (slot < (uint32_t)kExtMax) sh.items[e][slot] = ((u64)ordered << 32) | (uint32_t)~(uint32_t)col;
}

// The ties of one step, `tmask` a bit per element of this lane's chunk: the wave's ties so far are `seen` (wave-uniform);
// the ones ranked below `need` (<= kExtMax) within the wave park their column.  Returns the new `seen`.
template <int N>
BP_DEV uint32_t ext_take(ExtShared &sh, int e, int wave, int lane, uint32_t tmask, int col0, uint32_t seen, uint32_t need) {
    if (seen >= need || __ballot(tmask != 0u) == 0ull) return seen;   // wave-uniform
    const uint32_t cnt = (uint32_t)__popc(tmask);
    const uint32_t incl = wave_scan_u32(cnt, lane);
    uint32_t rank = seen + incl - cnt;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if ((tmask >> i) & 1u) {
            if (rank < need) sh.tie_col[e][wave][rank] = (uint32_t)(col0 + i);
            ++rank;
        }
    }
    return seen + __shfl(incl, 63);
}

}  // namespace

template <class ET>
__global__ __launch_bounds__(kPickThreads) void row_extremes_kernel(const RowExtremesParams p) {
    using E = RowElem<ET>;
    __shared__ ExtShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    const uint32_t n = (uint32_t)p.n;
    const bool do_top = p.top_val != nullptr || p.top_idx != nullptr;
    const bool do_bot = p.bot_val != nullptr || p.bot_idx != nullptr;
    const RowView<ET> row(static_cast<const char *>(p.logits) + r * p.row_stride * E::EB, p.cols);

    if (n == 1u) {
        // ---- one pass.  A lane meets its columns in ascending order, so its own extremes need 32-bit compares only (a strict
        // one keeps the lowest column); four chunks are loaded before the first is looked at, to keep that many loads in flight.
        // Across lanes: the maxima of (key, ~column) and (~key, ~column) as 64-bit integers, 0 = the lane saw nothing
        uint32_t tk = 0, bk = 0;
        int tc = -1, bc = -1;
        auto look = [&](const uint32_t (&raw)[8], uint32_t mask, int col0) {
#pragma unroll
            for (int i = 0; i < E::N; ++i) {
                const uint32_t k = E::key(raw[i]);
                const bool valid = (mask >> i) & 1u;
                if (valid && (k > tk || tc < 0)) { tk = k; tc = col0 + i; }
                if (valid && (k < bk || bc < 0)) { bk = k; bc = col0 + i; }
            }
        };
        for (int s = 0; s < row.steps(); s += 4) {
            // (a step past the wave's run has no chunk: RowView::chunk returns -1)
            const int c0 = row.chunk(wave, s, lane), c1 = row.chunk(wave, s + 1, lane);
            const int c2 = row.chunk(wave, s + 2, lane), c3 = row.chunk(wave, s + 3, lane);
            uint32_t r0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, r1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            uint32_t r2[8] = {0, 0, 0, 0, 0, 0, 0, 0}, r3[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            uint32_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
            int col0 = 0, col1 = 0, col2 = 0, col3 = 0;
            if (c0 >= 0) col0 = row.load(c0, r0, m0);
            if (c1 >= 0) col1 = row.load(c1, r1, m1);
            if (c2 >= 0) col2 = row.load(c2, r2, m2);
            if (c3 >= 0) col3 = row.load(c3, r3, m3);
            look(r0, m0, col0);
            look(r1, m1, col1);
            look(r2, m2, col2);
            look(r3, m3, col3);
        }
        u64 hi = tc < 0 ? 0ull : ((u64)tk << 32) | (uint32_t)~(uint32_t)tc;
        u64 lo = bc < 0 ? 0ull : ((u64)~bk << 32) | (uint32_t)~(uint32_t)bc;
        hi = wave_max_u64(hi);
        lo = wave_max_u64(lo);
        if (lane == 0) { sh.wave64[0][wave] = hi; sh.wave64[1][wave] = lo; }
        __syncthreads();
        if (tid < 2 && (tid == 0 ? do_top : do_bot)) {
            u64 v = sh.wave64[tid][0];
#pragma unroll
            for (int w = 1; w < kPickWaves; ++w) v = sh.wave64[tid][w] > v ? sh.wave64[tid][w] : v;
            const uint32_t ordered = (uint32_t)(v >> 32);
            const float x = E::to_f32(E::unkey(tid == 0 ? ordered : ~ordered));
            float *val = tid == 0 ? p.top_val : p.bot_val;
            int32_t *idx = tid == 0 ? p.top_idx : p.bot_idx;
            if (val) val[r] = x;
            if (idx) idx[r] = (int32_t)~(uint32_t)v;
        }
        return;
    }

    // ---- 1: radix select of both thresholds.  pre_*: the key prefix found so far; beyond_*: elements strictly beyond it
    if (tid < 2) sh.n_items[tid] = 0u;
    uint32_t pre_t = 0, pre_b = 0, beyond_t = 0, beyond_b = 0;
    constexpr int ROUNDS = E::KEY_BITS / 8;
    for (int rd = 0; rd < ROUNDS; ++rd) {
        const int shift = E::KEY_BITS - 8 * (rd + 1);
        for (int i = tid; i < kHistCopies * kHistStride; i += kPickThreads) sh.hist[i] = 0u;
        __syncthreads();
        uint32_t *mine_t = sh.hist + (rd == 0 ? (lane & 31) : (lane & 15)) * kHistStride;
        uint32_t *mine_b = sh.hist + (rd == 0 ? (lane & 31) : 16 + (lane & 15)) * kHistStride;
        for (int s = 0; s < row.steps(); ++s) {
            const int c = row.chunk(wave, s, lane);
            if (c < 0) continue;
            uint32_t raw[8], mask;
            row.load(c, raw, mask);
#pragma unroll
            for (int i = 0; i < E::N; ++i) {
                const uint32_t k = E::key(raw[i]), d = (k >> shift) & 255u;
                const bool valid = (mask >> i) & 1u;
                if (rd == 0) {
                    if (valid) atomicAdd(&mine_t[d], 1u);
                } else {
                    const uint32_t head = k >> ((shift + 8) & 31);
                    if (valid && do_top && head == pre_t) atomicAdd(&mine_t[d], 1u);
                    if (valid && do_bot && head == pre_b) atomicAdd(&mine_b[d], 1u);
                }
            }
        }
        __syncthreads();
        if (tid < 512) {
            const int e = tid >> 8, d = tid & 255;
            const int first = rd == 0 ? 0 : 16 * e, copies = rd == 0 ? kHistCopies : 16;
            uint32_t t = 0;
            for (int cp = 0; cp < copies; ++cp) t += sh.hist[(first + cp) * kHistStride + d];
            sh.bins[e][d] = t;
        }
        __syncthreads();
        if (wave < 2) {
            // wave 0, the top end: lane l holds the digits 255 - 4 l ... 252 - 4 l; wave 1, the bottom end: 4 l ... 4 l + 3
            uint32_t c4[4], tot = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c4[j] = sh.bins[wave][wave == 0 ? 255 - 4 * lane - j : 4 * lane + j];
                tot += c4[j];
            }
            const uint32_t incl = wave_scan_u32(tot, lane);
            uint32_t run = (wave == 0 ? beyond_t : beyond_b) + incl - tot;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (run < n && run + c4[j] >= n) {
                    sh.sel_digit[wave] = (uint32_t)(wave == 0 ? 255 - 4 * lane - j : 4 * lane + j);
                    sh.sel_above[wave] = run;
                }
                run += c4[j];
            }
        }
        __syncthreads();
        pre_t = (pre_t << 8) | sh.sel_digit[0];
        pre_b = (pre_b << 8) | sh.sel_digit[1];
        beyond_t = sh.sel_above[0];
        beyond_b = sh.sel_above[1];
        __syncthreads();   // sel_* are rewritten by the next round
    }

    // ---- 2: collect.  Every lane stays in the loop: the ties are numbered with wave-wide operations
    const uint32_t need_t = do_top ? n - beyond_t : 0u, need_b = do_bot ? n - beyond_b : 0u;
    uint32_t seen_t = 0, seen_b = 0;
    for (int s = 0; s < row.steps(); ++s) {
        const int c = row.chunk(wave, s, lane);
        uint32_t raw[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mask = 0;
        int col0 = 0;
        if (c >= 0) col0 = row.load(c, raw, mask);
        uint32_t ties_t = 0, ties_b = 0;
#pragma unroll
        for (int i = 0; i < E::N; ++i) {
            if (!((mask >> i) & 1u)) continue;
            const uint32_t k = E::key(raw[i]);
            if (do_top) {
                if (k > pre_t) ext_push(sh, 0, k, col0 + i);
                else if (k == pre_t) ties_t |= 1u << i;
            }
            if (do_bot) {
                if (k < pre_b) ext_push(sh, 1, ~k, col0 + i);
                else if (k == pre_b) ties_b |= 1u << i;
            }
        }
        seen_t = ext_take<E::N>(sh, 0, wave, lane, ties_t, col0, seen_t, need_t);
        seen_b = ext_take<E::N>(sh, 1, wave, lane, ties_b, col0, seen_b, need_b);
    }
    if (lane == 0) {
        sh.tie_cnt[0][wave] = seen_t < need_t ? seen_t : need_t;
        sh.tie_cnt[1][wave] = seen_b < need_b ? seen_b : need_b;
    }
    __syncthreads();
    // a parked tie's rank among the row's ties: the counts of the waves in front of it (capped at `need`, which ends the
    // taking just the same) plus its rank in the wave
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const uint32_t need = e == 0 ? need_t : need_b, beyond = e == 0 ? beyond_t : beyond_b;
        const uint32_t ordered = e == 0 ? pre_t : ~pre_b;
        uint32_t base = 0;
#pragma unroll
        for (int w = 0; w < kPickWaves; ++w) base += w < wave ? sh.tie_cnt[e][w] : 0u;
        const uint32_t at = base + (uint32_t)lane;
        if ((uint32_t)lane < sh.tie_cnt[e][wave] && at < need)
            sh.items[e][beyond + at] = ((u64)ordered << 32) | (uint32_t)~sh.tie_col[e][wave][lane];
    }
    __syncthreads();

    // ---- 3: rank the n held values of an end by counting (they are distinct: the columns are) and store them in order
    if (wave < 2 && (wave == 0 ? do_top : do_bot) && (uint32_t)lane < n) {
        const u64 v = sh.items[wave][lane];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) rank += sh.items[wave][j] > v ? 1u : 0u;
        const uint32_t ordered = (uint32_t)(v >> 32);
        const float x = E::to_f32(E::unkey(wave == 0 ? ordered : ~ordered));
        float *val = wave == 0 ? p.top_val : p.bot_val;
        int32_t *idx = wave == 0 ? p.top_idx : p.bot_idx;
        const int64_t at = r * (int64_t)n + rank;
        if (val) val[at] = x;
        if (idx) idx[at] = (int32_t)~(uint32_t)v;
    }
}

hipError_t launch_row_extremes(const RowExtremesParams &p, int dtype, hipStream_t stream) {
    auto go = [&](auto et) {
        hipLaunchKernelGGL((row_extremes_kernel<decltype(et)>), dim3((unsigned)p.rows), dim3(kPickThreads), 0, stream, p);
        return hipGetLastError();
    };
    return with_row_dtype(dtype, go);
}

}  // namespace bp
