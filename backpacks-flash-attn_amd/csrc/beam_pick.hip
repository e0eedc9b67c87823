// bp_beam_pick: one decode step of beam search for `groups` prompts x `beam_width` (W <= 8) beams, rows r = g W + w.  No host
// value enters, so one captured launch pair serves every step.  The row reader (RowView, RowElem) and the 40-bit
// fixed-point masses are vocab_row.h's.
//
// Contract per group g (restated by _eager_beam_pick, src/utils/generation.py, and by tests/beam_ref.py):
//   candidates  a live row w (finished == NULL or finished[gW+w] == 0): m = max_v float(x_v), lse = m + log sum_v exp(float(x_v) - m)
//               in fp32; candidate (w, v) scores s_w + (float(x_v) - lse), the two fp32 operations in that order.  A live row
//               with a NaN or +inf logit, or without a finite one, has all its candidates at -inf.  A finished row has ONE
//               candidate, (w, pad_token_id), at s_w: the frozen hypothesis.  A NaN score counts, and is written, as -inf;
//               -0 as +0.
//   selection   rank by (score descending, w ascending, v ascending), take the first W (vocab >= W: they exist)
//   slots       a surviving hypothesis never moves: the W winners in rank order take slot w, their parent's, when it is still
//               free; the rest, in rank order, the lowest free slot.  So a slot that another slot names as parent names
//               itself: parent[parent[r]] == parent[r], which is what lets bp_beam_copy_rows copy in place.
//   writes      slot t holding (w, v, score): parent[gW+t] = gW+w (a GLOBAL row), tokens, column counters[gW+t] of sequences
//               (skipped outside [0, seq_cols)), beam_scores[gW+t] = score, finished[gW+t] = old finished[gW+w] | (w live
//               and v == eos_token_id).  Every old score and flag of the group is read before any is written.
//   first step  beam_scores = {0, -inf, ...}: all W winners come from beam 0, no special mode.
//
// Stage 1, one 1024-thread workgroup per live row, three passes over the row (it stays in L2): the maximum; the sum of
// exp(x - m) as 64-bit integers of 2^-40, so its value does not depend on the order of the additions; the W best
// (score, v) as 64-bit keys -- ordered score above ~v -- eight sorted per lane (static indices only: compare-exchange
// chains, no register array is indexed by a variable), merged per wave by W rounds of a wave maximum, then across the
// 16 waves by wave 0.  W keys per row go to `ws`.  Stage 2, one wave per group: lane 8 w + i holds candidate i of row w,
// W rounds of a wave maximum on (score, 7 - w, ~v) pick the winners, every lane runs the slot walk on two bit masks, and
// lane j stores winner j.  Integer keys and integer sums: the result is bit-identical across calls.
#include "bp_kernels.h"
#include "vocab_row.h"

namespace bp {

namespace {

constexpr int kBeamMax = 8;
constexpr uint32_t kTokMask = (1u << 23) - 1u;

// ordered key of a score: NaN as -inf, -0 as +0
BP_DEV uint32_t score_key(float s) { return greedy_key(s != s ? -INFINITY : s); }

BP_DEV void cmp_swap(u64 &hi, u64 &lo) {
    const u64 a = hi, b = lo;
    hi = a > b ? a : b;
    lo = a > b ? b : a;
}

}  // namespace

template <class ET>
__global__ __launch_bounds__(kPickThreads) void beam_rows_kernel(const BeamPickParams p) {
    using E = RowElem<ET>;
    __shared__ u64 sh_wave[kPickWaves];
    __shared__ u64 sh_best[kPickWaves * kBeamMax];
    const int r = blockIdx.x, W = p.beam_width;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (p.finished && p.finished[r] != 0) return;   // workgroup-uniform: stage 2 makes the frozen candidate
    const RowView<ET> row(static_cast<const char *>(p.logits) + (int64_t)r * p.row_stride * E::EB, p.vocab);
    const float s = p.beam_scores[r];

    // ---- pass 1: the maximum, a NaN above everything
    uint32_t best = 0;
    for (int st = 0; st < row.steps(); ++st) {
        const int c = row.chunk(wave, st, lane);
        if (c < 0) continue;
        uint32_t raw[8], mask;
        row.load(c, raw, mask);
#pragma unroll
        for (int i = 0; i < E::N; ++i) {
            const uint32_t k = greedy_key(E::to_f32(raw[i]));
            if (((mask >> i) & 1u) && k > best) best = k;
        }
    }
    best = (uint32_t)wave_max_u64((u64)best);
    if (lane == 0) sh_wave[wave] = best;
    __syncthreads();
    best = (uint32_t)sh_wave[0];
#pragma unroll
    for (int w = 1; w < kPickWaves; ++w) best = (uint32_t)sh_wave[w] > best ? (uint32_t)sh_wave[w] : best;
    __syncthreads();   // sh_wave is reused by the sum
    const float xmax = greedy_unkey(best);   // garbage for a NaN, which is caught first
    const bool degenerate = best == 0xffffffffu || !(fabsf(xmax) < INFINITY);

    // ---- pass 2: sum of exp(x - max) in fixed point, lse
    float lse = 0.f;
    if (!degenerate) {
        u64 acc = 0;
        for (int st = 0; st < row.steps(); ++st) {
            const int c = row.chunk(wave, st, lane);
            if (c < 0) continue;
            uint32_t raw[8], mask;
            row.load(c, raw, mask);
#pragma unroll
            for (int i = 0; i < E::N; ++i)
                if ((mask >> i) & 1u) acc += fixed_mass(E::to_f32(raw[i]), xmax);
        }
        acc = wave_sum_u64(acc);
        if (lane == 0) sh_wave[wave] = acc;
        __syncthreads();
        u64 total = 0;
#pragma unroll
        for (int w = 0; w < kPickWaves; ++w) total += sh_wave[w];
        lse = xmax + logf((float)total * (1.f / kFixedOne));   // total >= 2^40: the maximum itself
    }

    // ---- pass 3: the lane's eight best keys, sorted, q0 the largest; 0 = none (no key of an element is 0)
    u64 q0 = 0, q1 = 0, q2 = 0, q3 = 0, q4 = 0, q5 = 0, q6 = 0, q7 = 0;
    for (int st = 0; st < row.steps(); ++st) {
        const int c = row.chunk(wave, st, lane);
        if (c < 0) continue;
        uint32_t raw[8], mask;
        const int col0 = row.load(c, raw, mask);
#pragma unroll
        for (int i = 0; i < E::N; ++i) {
            const float sc = degenerate ? -INFINITY : s + (E::to_f32(raw[i]) - lse);
            const u64 k = ((u64)score_key(sc) << 32) | (uint32_t)~(uint32_t)(col0 + i);
            if (((mask >> i) & 1u) && k > q7) {
                q7 = k;
                cmp_swap(q6, q7); cmp_swap(q5, q6); cmp_swap(q4, q5); cmp_swap(q3, q4);
                cmp_swap(q2, q3); cmp_swap(q1, q2); cmp_swap(q0, q1);
            }
        }
    }
    // the wave's W best: W rounds of a maximum over the lanes' heads; the owner pops
    u64 mine = 0;
    for (int j = 0; j < W; ++j) {
        const u64 m = wave_max_u64(q0);
        if (q0 == m) { q0 = q1; q1 = q2; q2 = q3; q3 = q4; q4 = q5; q5 = q6; q6 = q7; q7 = 0; }
        if (lane == j) mine = m;
    }
    if (lane < kBeamMax) sh_best[wave * kBeamMax + lane] = mine;   // lanes W .. 7 hold 0
    __syncthreads();
    if (wave != 0) return;
    // the row's W best of the 16 x 8 wave results: two keys per lane
    u64 a = sh_best[lane], b = sh_best[64 + lane];
    cmp_swap(a, b);
    u64 out = 0;
    for (int j = 0; j < W; ++j) {
        const u64 m = wave_max_u64(a);
        if (a == m) { a = b; b = 0; }
        if (lane == j) out = m;
    }
    if (lane < W) reinterpret_cast<u64 *>(p.ws)[(int64_t)r * kBeamMax + lane] = out;
}

__global__ __launch_bounds__(64) void beam_merge_kernel(const BeamPickParams p) {
    const int g = blockIdx.x, W = p.beam_width;
    const int lane = threadIdx.x, w = lane >> 3, i = lane & 7;
    const int64_t row0 = (int64_t)g * W;
    // every old score and flag of the group, before anything is written
    bool fin = false;
    float s = 0.f;
    if (w < W) {
        fin = p.finished && p.finished[row0 + w] != 0;
        s = p.beam_scores[row0 + w];
    }
    u64 key = 0;   // (ordered score, 7 - w, 2^23 - 1 - v): the maximum is the best score at its lowest w, then lowest v
    if (w < W && i < W) {
        const uint32_t wbits = (uint32_t)(7 - w) << 23;
        if (fin) {
            if (i == 0) key = ((u64)score_key(s) << 32) | wbits | (kTokMask - (uint32_t)p.pad);
        } else {
            const u64 k = reinterpret_cast<const u64 *>(p.ws)[(row0 + w) * kBeamMax + i];
            const uint32_t v = ~(uint32_t)k & kTokMask;
            key = (k & 0xffffffff00000000ull) | wbits | (kTokMask - v);
        }
    }
    const u64 finmask = __ballot(fin && i == 0);   // bit 8 w: row w was finished on entry
    u64 mine = 0;
    for (int j = 0; j < W; ++j) {
        const u64 m = wave_max_u64(key);
        if (key == m) key = 0;
        if (lane == j) mine = m;
    }
    // the slot walk, on every lane alike: `free` has a bit per free slot, `slots` four bits per rank
    uint32_t free_slots = (1u << W) - 1u, slots = 0, placed = 0;
    uint32_t parents = 0;   // three bits per rank
#pragma unroll
    for (int j = 0; j < kBeamMax; ++j) {
        const uint32_t pw = 7u - (((uint32_t)shfl_u64(mine, j) >> 23) & 7u);
        parents |= pw << (3 * j);
        if (j < W && ((free_slots >> pw) & 1u)) {
            free_slots &= ~(1u << pw);
            slots |= pw << (4 * j);
            placed |= 1u << j;
        }
    }
#pragma unroll
    for (int j = 0; j < kBeamMax; ++j) {
        if (j < W && !((placed >> j) & 1u)) {
            const uint32_t t = (uint32_t)__ffs((int)free_slots) - 1u;
            free_slots &= free_slots - 1u;
            slots |= t << (4 * j);
        }
    }
    if (lane < W) {
        const int pw = (int)((parents >> (3 * lane)) & 7u);
        const int64_t t = row0 + ((slots >> (4 * lane)) & 15u);
        const int v = (int)(kTokMask - ((uint32_t)mine & kTokMask));
        const bool was_fin = (finmask >> (8 * pw)) & 1ull;
        p.parent[t] = (int32_t)(row0 + pw);
        p.tokens[t * p.tokens_stride] = v;
        if (p.sequences) {
            const int c = p.counters ? p.counters[t] : 0;
            if (c >= 0 && c < p.seq_cols) p.sequences[t * p.seq_stride + c] = v;
        }
        p.beam_scores[t] = greedy_unkey((uint32_t)(mine >> 32));
        if (p.finished) p.finished[t] = (was_fin || (p.eos >= 0 && v == p.eos)) ? 1 : 0;
    }
}

hipError_t launch_beam_pick(const BeamPickParams &p, int dtype, hipStream_t stream) {
    auto go = [&](auto et) {
        hipLaunchKernelGGL((beam_rows_kernel<decltype(et)>), dim3((unsigned)(p.groups * p.beam_width)), dim3(kPickThreads), 0,
                           stream, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(beam_merge_kernel, dim3((unsigned)p.groups), dim3(64), 0, stream, p);
        return hipGetLastError();
    };
    return with_row_dtype(dtype, go);
}

}  // namespace bp
