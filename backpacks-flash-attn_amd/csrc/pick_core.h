// Token selection on the device for the decode loops: one row of logits in, one token out.  The shared body of
// bp_pick_token (csrc/pick_token.hip), bp_pick_token_ctl (csrc/pick_token_ctl.hip), bp_pick_token_lim (csrc/pick_token_lim.hip) and
// bp_pick_token_lim_rows (csrc/pick_token_rows.hip) and bp_pick_token_phrases (csrc/pick_token_phrases.hip).
//
// Replaces the host-driven picks of the generation loops (src/utils/generation.py: torch.argmax, and
// torch.distributions.Categorical, whose argument validation reads a device value on the host) and adds the sampling
// options of the reference's control baseline (training/run_pplm.py:80,347-348,569-581: temperature, top_k with ties
// kept).  The contract, restated by _eager_pick (src/utils/generation.py) and by the tests:
//
//   greedy    lowest index of the maximal logit; a NaN counts as larger than every number (torch.argmax)
//   sampling  z_i = float(x_i) * (1 / T)
//             top-k   tau = k-th largest z with multiplicity, keep z_i >= tau (ties kept); off for k <= 0 or k >= vocab
//             top-p   on the probabilities renormalised over what top-k kept: keep i iff the mass of kept tokens with
//                     z_j > z_i is < p (equal logits share a fate)
//             u       ((r0 >> 8) + 0.5) 2^-24, (r0, _) = philox2x32(counters[b], salt, key), (key, salt) the stream of row b
//             token   lowest index t, in vocabulary order, whose cumulative kept probability through t exceeds u
//             degenerate rows (a NaN or +inf, or nothing finite) take the greedy answer
//
// One 1024-thread workgroup per row, 16-byte loads, every pass re-reads the row (it stays in L2).  All masses are FIXED POINT:
// w_i = trunc(exp(z_i - max z) 2^40) as a 64-bit integer, so sums do not depend on their order -- histogram atomics on LDS,
// wave reductions and the vocabulary-order scan all give the same bits on every call -- and the comparisons of the
// contract (mass above < p S, cumulative mass > u S) are exact integer comparisons.  The quantisation (2^-40 per term against a
// total >= 1) is far below the fp32 rounding of the exponentials themselves.
//
// Passes over the row:
//   1  argmax on a 64-bit (ordered value, ~index) key: the greedy token, max z, and the degenerate cases
//   2  top-k: radix select of the k-th largest element on the order-preserving integer key of x (x -> z is monotone), 8 bits
//      a round: two rounds for 16-bit logits, four for fp32; rounds after the first only touch the selected bucket
//   3  top-p: the same select with the fixed-point masses as weights; its first round also yields the mass top-k kept
//   4  the scan: per-lane sums in a wave-contiguous layout (wave w owns a contiguous run of chunks, lane l of step s the chunk
//      64 s + l of it), the total, then the ONE wave that holds the target walks its run again with a wave prefix sum
// The histograms are 32 copies (lane & 31) of 256 bins, a copy stride of 257 words: a wave's lanes that hit one bin land in
// different banks, and at most two lanes share an address.
//
// Controlled form (bp_pick_token_ctl, pick_token_ctl.hip): pick_token_kernel<Controlled<ET>> adds a repetition penalty over
// the row's history, an EOS mask below min_length and the finished flags (contract in include/bp_hip.h).  The flag rides on
// the element tag, in a code object of its own, so the plain instantiations keep their names and their code.  What it changes:
//   0  before pass 1: a row finished on entry writes the pad and returns; otherwise the history sequences[b, 0 : min(c, cols)]
//      becomes a bitmap in dynamic LDS, one bit per vocabulary entry (atomicOr on LDS words; ids outside [0, vocab) dropped)
//   *  every pass takes its value from ONE helper (Logits::x / Logits::z): pen(float(x) [* 1/T]) with the EOS entry as -inf.
//      pen multiplies a member of the history by theta (negative) or 1/theta (otherwise): one fp32 multiplication
//   1  also the maximum of z: pen(x * 1/T) and pen(x) * 1/T round differently, so max z is not xmax * 1/T any more
//   2, 3  select on the 32-bit key of the fp32 z itself (four rounds for every element type): pen is not monotone across the
//      two classes, so the key of the raw element no longer orders the row; the threshold is the z the key stands for
//   5  after the token is written: finished[b] = 1 by that one lane when the token is the EOS id
//
// Limited form (bp_pick_token_lim, pick_token_lim.hip): pick_token_kernel<Limited<ET>> is the controlled form with n-gram
// blocking, frequency / presence penalties and a list of suppressed ids (contract in include/bp_hip.h).  Again a tag and a
// code object of its own.  What it adds, all of it in dynamic LDS (LimLayout) and built before pass 1 (Logits<Limited>::build):
//   members  the history bitmap of the controlled form, also built when a frequency / presence penalty is on
//   banned   a second bitmap of the same shape: the suppressed ids (thread-strided over the list), then the n-gram scan --
//            thread-strided start positions i, each comparing at most n - 1 int64 pairs of the row of `sequences` against its
//            last n - 1 entries and setting the bit of the id behind a match
//   counts   an open-addressing table of 32-bit entries, id in the low 19 bits and count in the high 13, empty = all ones,
//            slots = the power of two >= 2 seq_cols (load <= 0.5), slot of an id = lim_hash(id) then linear probing.  Every
//            in-vocabulary id of the history is inserted (atomicCAS claims a slot), positions >= penalty_begin add 1 << 19:
//            integer counts, so the result does not depend on which thread came first.  Only members are looked up, and a
//            member's probe always ends on its id.  Every probe loop is bounded by the slot count.
//   the helper applies, in this order: pen, v -= fmaf(frequency, count, presence) for a count > 0, -inf for a banned id or
//   the masked EOS.  Everything behind the helper is the controlled form's.
//
// Row-limited form (bp_pick_token_lim_rows, pick_token_rows.hip): pick_token_kernel<RowLimited<ET>> is the limited form whose
// penalty_begin and min_length may come from per-row device arrays (prompts of different lengths in one batch).  A third
// tag and code object.  The two values of a row are resolved before pass 1 (row_params: a uniform load each, negative entries
// clamped to 0, the scalar when the array is NULL) and are dead behind it: the first only feeds the `counted` flag of the
// table build, the second only the choice of the masked column.  Nothing else differs from the limited form.
//
// Phrased form (bp_pick_token_phrases, pick_token_phrases.hip): pick_token_kernel<Phrased<ET>> is the row-limited form with two
// lists of phrases (ids + offsets on the device, never read by the host, so every entry is checked here).  A fifth tag and
// code object.  What it adds:
//   ban   in `build`, behind the suppressed ids: thread-strided over the phrases, each comparing at most L - 1 int64 entries
//         of the end of the history against its first L - 1 ids and setting the `banned` bit of its last id on a match.  The
//         bitmap is on when n_ban > 0 (the second argument of LimLayout: the other forms never read the field)
//   stop  behind the token's write, by the whole workgroup: the writing lane leaves the token in sel_digit and ~0 in sel_above
//         (both dead behind the selects, whose last barrier every thread has passed), a barrier, thread-strided over the phrases
//         each compares BACKWARDS from the new token and leaves at the first mismatch, atomicMin of the matching index on
//         sel_above, a barrier, and thread 0 writes the flag, `ends` and `reasons` -- for the EOS id too, which wins
#pragma once
#include <type_traits>

#include "bp_kernels.h"
#include "bp_philox.h"
#include "vocab_row.h"

namespace bp {

// Plain form: the tag is the element type itself
template <class ET> using Plain = ET;
// Controlled form: the flag rides on the element tag (as Weighted<ET> in decode_core.h)
template <class ET> struct Controlled {};
// Limited form: the controlled one with the row limits of bp_pick_token_lim
template <class ET> struct Limited {};
// Row-limited form: the limited one with penalty_begin and min_length per row (bp_pick_token_lim_rows)
template <class ET> struct RowLimited {};
// Phrased form: the row-limited one with banned and stop phrases (bp_pick_token_phrases)
template <class ET> struct Phrased {};
template <class T> struct PickTag { using elem = T; static constexpr bool ctl = false, lim = false, rows = false, phrases = false; };
template <class T> struct PickTag<Controlled<T>> { using elem = T; static constexpr bool ctl = true, lim = false, rows = false, phrases = false; };
template <class T> struct PickTag<Limited<T>> { using elem = T; static constexpr bool ctl = true, lim = true, rows = false, phrases = false; };
template <class T> struct PickTag<RowLimited<T>> { using elem = T; static constexpr bool ctl = true, lim = true, rows = true, phrases = false; };
template <class T> struct PickTag<Phrased<T>> { using elem = T; static constexpr bool ctl = true, lim = true, rows = true, phrases = true; };

// Dynamic LDS of the limited form, in 32-bit words: [members][banned][count table], each only when its control is on.  The
// switches depend on the arguments alone, never on a row, so the host sizes the allocation from the same struct.  `phrase_ban`
// is the phrased form's own switch of the ban bitmap (n_ban > 0): a constant false everywhere else.
constexpr uint32_t kLimIdBits = 19, kLimIdMask = (1u << kLimIdBits) - 1u, kLimEmpty = 0xffffffffu;
constexpr int kLimMaxCols = (1 << (32 - kLimIdBits)) - 1;   // 8191: what the 13 count bits hold
// slot of an id in a table of 2^(32 - shift) slots: a multiplicative (Fibonacci) hash, tests/pick_lim_ref.py restates it
__host__ __device__ inline uint32_t lim_hash(uint32_t id, int shift) { return (id * 2654435761u) >> shift; }
struct LimLayout {
    bool members_on, banned_on, counts_on;
    int ban_at, table_at, slots, total_words;
    __host__ __device__ explicit LimLayout(const PickParams &p, bool phrase_ban = false) {
        counts_on = p.freq_pen != 0.f || p.pres_pen != 0.f;
        members_on = p.theta != 1.f || counts_on;
        banned_on = p.ngram > 0 || p.n_suppress > 0 || phrase_ban;
        const int words = (p.vocab + 31) / 32 + 1;
        ban_at = members_on ? words : 0;
        table_at = ban_at + (banned_on ? words : 0);
        slots = counts_on ? 1 << (32 - p.table_shift) : 0;
        total_words = table_at + slots;
    }
};

namespace {

struct PickShared {
    u64 hist[kHistCopies * kHistStride];
    u64 bins[256];
    u64 wave64[kPickWaves];
    float wavef[kPickWaves];
    int wavei[kPickWaves];
    u64 sel_above;
    uint32_t sel_digit;
};

// The value of an element as every pass sees it.  Plain rows: x = float(raw), z = x * (1 / T).
template <class TAG> struct Logits {
    using E = RowElem<typename PickTag<TAG>::elem>;
    float inv_t;
    BP_DEV Logits(const PickParams &p, int, const uint32_t *) : inv_t(p.inv_t) {}
    struct Chunk {};
    BP_DEV Chunk chunk(const RowView<typename PickTag<TAG>::elem> &, int) const { return Chunk{}; }
    BP_DEV float x(uint32_t raw, Chunk, int) const { return E::to_f32(raw); }
    BP_DEV float z(uint32_t raw, Chunk, int) const { return E::to_f32(raw) * inv_t; }
};
// Controlled rows: pen() on the members of the history, then the EOS entry as -inf.  A Chunk is the column of element 0
// of chunk c and the membership bits of its elements, bit i for column col0 + i (the bitmap carries one spare word: two
// words cover any chunk).
template <class ET> struct Logits<Controlled<ET>> {
    using E = RowElem<ET>;
    const uint32_t *bitmap;   // NULL: no history (theta == 1, no sequences, or nothing in front of the position)
    float inv_t, theta, inv_theta;
    int eos;                  // the masked column, -1 for none
    BP_DEV Logits(const PickParams &p, int counter, const uint32_t *bitmap_)
        : bitmap(bitmap_), inv_t(p.inv_t), theta(p.theta), inv_theta(p.inv_theta),
          eos(p.eos >= 0 && counter < p.min_length ? p.eos : -1) {}
    struct Chunk { int col0; uint32_t members; };
    BP_DEV Chunk chunk(const RowView<ET> &row, int c) const {
        const int col0 = (c < 0 ? 0 : c) * E::N - row.head;
        if (bitmap == nullptr) return Chunk{col0, 0u};
        const int base = col0 < 0 ? 0 : col0;
        const u64 two = (u64)bitmap[base >> 5] | ((u64)bitmap[(base >> 5) + 1] << 32);
        return Chunk{col0, (uint32_t)(two >> (base & 31)) << (base - col0)};
    }
    BP_DEV float ctl(float v, Chunk ck, int i) const {
        if ((ck.members >> i) & 1u) v = v < 0.f ? v * theta : v * inv_theta;
        return ck.col0 + i == eos ? -INFINITY : v;
    }
    // element i of the chunk
    BP_DEV float x(uint32_t raw, Chunk ck, int i) const { return ctl(E::to_f32(raw), ck, i); }
    BP_DEV float z(uint32_t raw, Chunk ck, int i) const { return ctl(E::to_f32(raw) * inv_t, ck, i); }
};

// Limited rows: the controlled value, then the count penalty, then the ban (layout and build: header comment, LimLayout).
template <class ET> struct Logits<Limited<ET>> {
    using E = RowElem<ET>;
    const uint32_t *members, *banned, *table;   // dynamic LDS; NULL: that control is off
    float inv_t, theta, inv_theta, freq, pres;
    int eos, shift;
    // phrase_ban: LimLayout's, true only from the phrased form
    BP_DEV Logits(const PickParams &p, int counter, const uint32_t *lds, bool phrase_ban = false)
        : inv_t(p.inv_t), theta(p.theta), inv_theta(p.inv_theta), freq(p.freq_pen), pres(p.pres_pen),
          eos(p.eos >= 0 && counter < p.min_length ? p.eos : -1), shift(p.table_shift) {
        const LimLayout lay(p, phrase_ban);
        members = lay.members_on ? lds : nullptr;
        banned = lay.banned_on ? lds + lay.ban_at : nullptr;
        table = lay.counts_on ? lds + lay.table_at : nullptr;
    }
    // counts: 16 bits per element of the chunk, looked up once per chunk in ONE loop over the members' bits (a probe loop per
    // element of the unrolled passes costs a saved exec mask each, more scalar registers than there are)
    struct Chunk { int col0; uint32_t members, banned; u64 counts[E::N / 4]; };
    static BP_DEV uint32_t bits(const uint32_t *bitmap, int base, int col0) {
        const u64 two = (u64)bitmap[base >> 5] | ((u64)bitmap[(base >> 5) + 1] << 32);
        return (uint32_t)(two >> (base & 31)) << (base - col0);
    }
    BP_DEV Chunk chunk(const RowView<ET> &row, int c) const {
        const int col0 = (c < 0 ? 0 : c) * E::N - row.head;
        const int base = col0 < 0 ? 0 : col0;
        Chunk ck{col0, members ? bits(members, base, col0) : 0u, banned ? bits(banned, base, col0) : 0u, {}};
        if (eos >= col0 && eos < col0 + E::N) ck.banned |= 1u << (eos - col0);   // the masked EOS is one more banned id
        if (table != nullptr) {
            uint32_t todo = ck.members & ((1u << E::N) - 1u);   // bits of columns inside the row only: the rest of the bitmap is 0
            while (todo) {
                const int i = __ffs(todo) - 1;
                todo &= todo - 1u;
                const u64 n = (u64)count((uint32_t)(col0 + i)) << (16 * (i & 3));
                if (E::N == 4 || i < 4) ck.counts[0] |= n; else ck.counts[E::N / 4 - 1] |= n;
            }
        }
        return ck;
    }
    // count of a member of the history: its probe ends on its id (the trip bound is the slot count)
    BP_DEV uint32_t count(uint32_t col) const {
        const uint32_t mask = (1u << (32 - shift)) - 1u;
        uint32_t slot = lim_hash(col, shift);
        for (uint32_t t = 0; t <= mask; ++t) {
            const uint32_t e = table[slot];
            if (e == kLimEmpty) return 0u;
            if ((e & kLimIdMask) == col) return e >> kLimIdBits;
            slot = (slot + 1u) & mask;
        }
        return 0u;
    }
    BP_DEV float lim(float v, Chunk ck, int i) const {
#pragma clang fp contract(off)   // pen's product is rounded before the subtraction: no fma of the two
        if ((ck.members >> i) & 1u) {
            v = v < 0.f ? v * theta : v * inv_theta;   // theta == 1: both factors are 1
            const uint32_t n = (uint32_t)(ck.counts[i >> 2] >> (16 * (i & 3))) & 0xffffu;   // 0 without a table
            if (n > 0u) v = v - __builtin_fmaf(freq, (float)n, pres);
        }
        return ((ck.banned >> i) & 1u) ? -INFINITY : v;
    }
    BP_DEV float x(uint32_t raw, Chunk ck, int i) const { return lim(E::to_f32(raw), ck, i); }
    BP_DEV float z(uint32_t raw, Chunk ck, int i) const { return lim(E::to_f32(raw) * inv_t, ck, i); }

    // One entry per in-vocabulary id of the history; counted: the position is at or behind penalty_begin
    static BP_DEV void insert(uint32_t *table, uint32_t id, bool counted, int shift) {
        const uint32_t mask = (1u << (32 - shift)) - 1u;
        uint32_t slot = lim_hash(id, shift);
        for (uint32_t t = 0; t <= mask; ++t) {
            uint32_t e = table[slot];
            if (e == kLimEmpty) e = atomicCAS(&table[slot], kLimEmpty, id);   // returns what was there: empty, or an owner
            if (e == kLimEmpty || (e & kLimIdMask) == id) {
                if (counted) atomicAdd(&table[slot], 1u << kLimIdBits);
                return;
            }
            slot = (slot + 1u) & mask;
        }
    }
    // Before pass 1, by the whole workgroup: hist = min(counter, seq_cols), possibly <= 0.  PHRASES: the phrased form's ban list
    template <bool PHRASES = false> static BP_DEV void build(const PickParams &p, int b, int hist, uint32_t *lds) {
        const int tid = threadIdx.x;
        const LimLayout lay(p, PHRASES && p.n_ban > 0);
        for (int i = tid; i < lay.total_words; i += kPickThreads) lds[i] = i >= lay.table_at ? kLimEmpty : 0u;
        __syncthreads();
        uint32_t *members = lds, *banned = lds + lay.ban_at, *table = lds + lay.table_at;
        for (int i = tid; i < p.n_suppress; i += kPickThreads) {
            const int32_t id = p.suppress[i];
            if (id >= 0 && id < p.vocab) atomicOr(&banned[id >> 5], 1u << (id & 31));
        }
        if constexpr (PHRASES) {
            // phrase j = ban_ids[lo : hi]; one whose offsets leave [0, ban_total] or whose length leaves 1 .. kMaxPhraseLen is
            // ignored.  Its first L - 1 ids against the last L - 1 entries of the history, raw values; L = 1 always matches
            if (p.sequences != nullptr) {
                const int64_t *seq = p.sequences + (int64_t)b * p.seq_stride;
                const int len = hist < 0 ? 0 : hist;
                for (int j = tid; j < p.n_ban; j += kPickThreads) {
                    const int lo = p.ban_offsets[j], hi = p.ban_offsets[j + 1];
                    if (lo < 0 || hi > p.ban_total || hi <= lo || hi - lo > kMaxPhraseLen || len < hi - lo - 1) continue;
                    const int n = hi - lo;
                    const int32_t *w = p.ban_ids + lo;
                    const int64_t *suffix = seq + (len - n + 1);   // the last n - 1 entries
                    bool match = true;
                    for (int t = 0; t < n - 1 && match; ++t) match = suffix[t] == (int64_t)w[t];
                    const int32_t id = w[n - 1];
                    if (match && id >= 0 && id < p.vocab) atomicOr(&banned[id >> 5], 1u << (id & 31));
                }
            }
        }
        if (p.sequences && hist > 0) {
            const int64_t *seq = p.sequences + (int64_t)b * p.seq_stride;
            if (lay.members_on) {
                for (int j = tid; j < hist; j += kPickThreads) {
                    const int64_t id = seq[j];
                    if (id >= 0 && id < (int64_t)p.vocab) {
                        atomicOr(&members[id >> 5], 1u << (id & 31));
                        if (lay.counts_on) insert(table, (uint32_t)id, j >= p.penalty_begin, p.table_shift);
                    }
                }
            }
            const int n = p.ngram;
            if (n > 0 && hist >= n) {
                const int64_t *suffix = seq + (hist - n + 1);   // the last n - 1 entries
                for (int i = tid; i <= hist - n; i += kPickThreads) {
                    bool match = true;
                    for (int t = 0; t < n - 1 && match; ++t) match = seq[i + t] == suffix[t];
                    const int64_t id = seq[i + n - 1];
                    if (match && id >= 0 && id < (int64_t)p.vocab) atomicOr(&banned[id >> 5], 1u << (id & 31));
                }
            }
        }
        __syncthreads();
    }
};

// Row-limited rows: the limited form on the parameters of ITS row -- penalty_begin and min_length taken from the arrays where
// they are given, one uniform load each, before pass 1 (both are dead behind it: the first feeds the `counted` flag of the
// table build, the second the choice of the masked column).  The host never reads the arrays, so a negative entry is
// clamped here.  The copy is of kernel arguments, i.e. of scalar registers that are loaded on use: no memory is involved.
template <class TAG> BP_DEV PickParams row_params(const PickParams &p, int b) {
    PickParams q = p;
    if constexpr (PickTag<TAG>::rows) {
        if (p.penalty_begins != nullptr) q.penalty_begin = p.penalty_begins[b] < 0 ? 0 : p.penalty_begins[b];
        if (p.min_lengths != nullptr) q.min_length = p.min_lengths[b] < 0 ? 0 : p.min_lengths[b];
    }
    return q;
}
template <class ET> struct Logits<RowLimited<ET>> : Logits<Limited<ET>> {
    BP_DEV Logits(const PickParams &p, int counter, const uint32_t *lds)
        : Logits<Limited<ET>>(row_params<RowLimited<ET>>(p, blockIdx.x), counter, lds) {}
    static BP_DEV void build(const PickParams &p, int b, int hist, uint32_t *lds) {
        Logits<Limited<ET>>::build(row_params<RowLimited<ET>>(p, b), b, hist, lds);
    }
};
// Phrased rows: the row-limited form whose ban bitmap is also on for a ban list, and whose build scans that list
template <class ET> struct Logits<Phrased<ET>> : Logits<Limited<ET>> {
    BP_DEV Logits(const PickParams &p, int counter, const uint32_t *lds)
        : Logits<Limited<ET>>(row_params<Phrased<ET>>(p, blockIdx.x), counter, lds, p.n_ban > 0) {}
    static BP_DEV void build(const PickParams &p, int b, int hist, uint32_t *lds) {
        Logits<Limited<ET>>::template build<true>(row_params<Phrased<ET>>(p, b), b, hist, lds);
    }
};

// Where a limited row's results go, worked out before pass 1 and parked in vector registers: the limited passes need every
// scalar register the controlled ones leave, and these addresses are not read again before the last lines of the kernel.
struct LimOutputs {
    int64_t *token, *column;   // column: NULL when there is no column counters[b] of sequences
    int32_t *flag;             // NULL without flags or without an EOS id
    float *stats;
    LimOutputs() = default;
    BP_DEV LimOutputs(const PickParams &p, int b, int counter) {
        token = p.tokens + (int64_t)b * p.tokens_stride;
        column = p.sequences && counter >= 0 && counter < p.seq_cols ? p.sequences + (int64_t)b * p.seq_stride + counter : nullptr;
        flag = p.finished && p.eos >= 0 ? p.finished + b : nullptr;
        stats = p.stats ? p.stats + (int64_t)b * 4 : nullptr;
        asm volatile("" : "+v"(token), "+v"(column), "+v"(flag), "+v"(stats));   // no instruction: pins them to vector registers
    }
};

// What the tail of a phrased row reads, worked out before pass 1 and parked in vector registers like LimOutputs: the flag,
// `ends` and `reasons` of the row, the stop list, and the row's own begin.  n == 0: the row cannot end at a phrase in this call --
// no list, or no column for the token (so the history would be clamped), or the EOS id still masked (c < the row's minimum).
struct PhraseTail {
    int32_t *flag, *ends, *reasons;   // NULL: not given
    const int32_t *ids, *offsets;
    int n, total, begin, eos, c;
    PhraseTail() = default;
    BP_DEV PhraseTail(const PickParams &p, const PickParams &q, int b, int counter) {   // q: row_params of the row
        flag = p.finished ? p.finished + b : nullptr;
        ends = p.ends ? p.ends + b : nullptr;
        reasons = p.reasons ? p.reasons + b : nullptr;
        ids = p.stop_ids; offsets = p.stop_offsets; total = p.stop_total;
        n = p.finished && p.sequences && counter >= 0 && counter < p.seq_cols && counter >= q.min_length ? p.n_stop : 0;
        begin = q.penalty_begin; eos = p.eos; c = counter;
        asm volatile("" : "+v"(flag), "+v"(ends), "+v"(reasons), "+v"(ids), "+v"(offsets));   // no instruction, as in LimOutputs
        asm volatile("" : "+v"(n), "+v"(total), "+v"(begin), "+v"(eos), "+v"(c));
    }
    // By the whole workgroup behind the token's write (header comment).  `token` sits at column c of the row, `column` points
    // at it: the columns in front are read, never column c itself (another lane has just written it).  Phrase j matches when
    // it lies in [begin, c] and equals the text that ends with the token; the lowest matching j goes into `low`.
    BP_DEV void scan(const int64_t *column, int token, u64 *low) const {
        for (int j = threadIdx.x; j < n; j += kPickThreads) {
            const int lo = offsets[j], hi = offsets[j + 1];
            if (lo < 0 || hi > total || hi <= lo || hi - lo > kMaxPhraseLen) continue;
            const int len = hi - lo;
            const int32_t *w = ids + lo;
            if (c + 1 - len < begin || w[len - 1] != token) continue;
            bool match = true;
            for (int k = 1; k < len && match; ++k) match = column[-k] == (int64_t)w[len - 1 - k];
            if (match) atomicMin(low, (u64)j);
        }
    }
};

// Key source of the radix select.  Plain rows: the order-preserving key of the RAW element (x -> z is monotone), 16 or 32
// bits.  Controlled rows: the 32-bit key of the fp32 z, whose threshold is z itself.
template <class TAG> struct SelectKey {
    using E = RowElem<typename PickTag<TAG>::elem>;
    static constexpr int BITS = E::KEY_BITS;
    static BP_DEV uint32_t key(uint32_t raw, float) { return E::key(raw); }
    static BP_DEV float threshold(uint32_t k, float inv_t) { return E::to_f32(E::unkey(k)) * inv_t; }
};
template <class ET> struct SelectKey<Controlled<ET>> {
    static constexpr int BITS = 32;
    static BP_DEV uint32_t key(uint32_t, float z) { return RowElem<float>::key(as_u32(z)); }
    static BP_DEV float threshold(uint32_t k, float) { return as_f32(RowElem<float>::unkey(k)); }
};
template <class ET> struct SelectKey<Limited<ET>> : SelectKey<Controlled<ET>> {};
template <class ET> struct SelectKey<RowLimited<ET>> : SelectKey<Controlled<ET>> {};
template <class ET> struct SelectKey<Phrased<ET>> : SelectKey<Controlled<ET>> {};

// Radix select, 8 bits a round from the top of the key: among the elements with z >= lo, the key K with
//   weight{key > K} < target <= weight{key >= K}
// weight = 1 (top-k: target = k) or the fixed-point mass (top-p: target = ceil(p total), `total` from the first round).
// Returns K to every thread.
template <class TAG, bool WEIGHTED>
BP_DEV uint32_t radix_select(const RowView<typename PickTag<TAG>::elem> &row, PickShared &sh, const Logits<TAG> &lg, float zmax,
                             float lo, u64 target, float top_p) {
    using E = RowElem<typename PickTag<TAG>::elem>;
    using KEY = SelectKey<TAG>;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t prefix = 0;
    u64 above = 0;
    constexpr int ROUNDS = KEY::BITS / 8;
    for (int r = 0; r < ROUNDS; ++r) {
        const int shift = KEY::BITS - 8 * (r + 1);
        for (int i = tid; i < kHistCopies * kHistStride; i += kPickThreads) sh.hist[i] = 0;
        __syncthreads();
        u64 *mine = sh.hist + (lane & (kHistCopies - 1)) * kHistStride;
        for (int s = 0; s < row.steps(); ++s) {
            const int c = row.chunk(wave, s, lane);
            if (c < 0) continue;
            uint32_t raw[8], mask;
            row.load(c, raw, mask);
            const auto ck = lg.chunk(row, c);
#pragma unroll
            for (int i = 0; i < E::N; ++i) {
                const float z = lg.z(raw[i], ck, i);
                const uint32_t key = KEY::key(raw[i], z);
                const bool in_bucket = r == 0 || (key >> (shift + 8)) == prefix;
                if (((mask >> i) & 1u) && z >= lo && in_bucket) {
                    const u64 w = WEIGHTED ? fixed_mass(z, zmax) : 1ull;
                    if (w) atomicAdd(&mine[(key >> shift) & 255u], w);
                }
            }
        }
        __syncthreads();
        if (tid < 256) {
            u64 t = 0;
            for (int cp = 0; cp < kHistCopies; ++cp) t += sh.hist[cp * kHistStride + tid];
            sh.bins[tid] = t;
        }
        __syncthreads();
        if (wave == 0) {
            // lane l holds the digits 255 - 4 l ... 252 - 4 l: lanes and registers in DESCENDING digit order
            u64 c4[4], tot = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c4[j] = sh.bins[255 - 4 * lane - j];
                tot += c4[j];
            }
            const u64 incl = wave_scan_u64(tot, lane);
            if (WEIGHTED && r == 0) {
                const u64 total = shfl_u64(incl, 63);
                u64 t = (u64)ceil((double)top_p * (double)total);
                t = t < 1 ? 1 : t;
                target = t > total ? total : t;   // only wave 0 needs it, and keeps it for the later rounds
            }
            u64 run = above + incl - tot;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (run < target && run + c4[j] >= target) {
                    sh.sel_digit = 255 - 4 * lane - j;
                    sh.sel_above = run;
                }
                run += c4[j];
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | sh.sel_digit;
        above = sh.sel_above;
        __syncthreads();   // sel_* are rewritten by the next round
    }
    return prefix;
}

}  // namespace

template <class TAG>
__global__ __launch_bounds__(kPickThreads) void pick_token_kernel(const PickParams p) {
    using ET = typename PickTag<TAG>::elem;
    using E = RowElem<ET>;
    constexpr bool CTL = PickTag<TAG>::ctl;
    __shared__ PickShared sh;
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RowView<ET> row(static_cast<const char *>(p.logits) + (int64_t)b * p.row_stride * E::EB, p.vocab);
    const int counter = p.counters ? p.counters[b] : 0;

    const uint32_t *bitmap = nullptr;
    [[maybe_unused]] LimOutputs out;   // limited rows only
    [[maybe_unused]] PhraseTail tail;  // phrased rows only
    if constexpr (CTL) {
        extern __shared__ uint32_t pick_bitmap[];   // (vocab + 31) / 32 + 1 words when theta != 1, else none (limited: LimLayout)
        if (p.finished && p.finished[b] != 0) {     // workgroup-uniform: the pad, no draw, the flag stays
            if (tid == 0) {
                p.tokens[(int64_t)b * p.tokens_stride] = p.pad;
                if (p.sequences && counter >= 0 && counter < p.seq_cols) p.sequences[(int64_t)b * p.seq_stride + counter] = p.pad;
                if (p.stats) {
                    float u = 0.f;
                    if (p.do_sample) {
                        const DropoutStream rs = dropout_stream(p.rng_state, (uint32_t)b);
                        uint32_t r0, r1;
                        philox2x32((uint32_t)counter, rs.salt, rs.key, r0, r1);
                        u = ((float)(r0 >> 8) + 0.5f) * 0x1p-24f;
                    }
                    float *st = p.stats + (int64_t)b * 4;
                    st[0] = 0.f; st[1] = 0.f; st[2] = 0.f; st[3] = u;
                }
            }
            return;
        }
        const int hist = counter < p.seq_cols ? counter : p.seq_cols;
        if constexpr (PickTag<TAG>::lim) {
            Logits<TAG>::build(p, b, hist, pick_bitmap);
            bitmap = pick_bitmap;
            out = LimOutputs(p, b, counter);
            if constexpr (PickTag<TAG>::phrases) tail = PhraseTail(p, row_params<TAG>(p, b), b, counter);
        } else if (p.theta != 1.f && p.sequences && hist > 0) {
            const int words = (p.vocab + 31) / 32 + 1;
            for (int i = tid; i < words; i += kPickThreads) pick_bitmap[i] = 0u;
            __syncthreads();
            const int64_t *seq = p.sequences + (int64_t)b * p.seq_stride;
            for (int j = tid; j < hist; j += kPickThreads) {
                const int64_t id = seq[j];
                if (id >= 0 && id < (int64_t)p.vocab) atomicOr(&pick_bitmap[id >> 5], 1u << (id & 31));
            }
            __syncthreads();
            bitmap = pick_bitmap;
        }
    }
    const Logits<TAG> lg(p, counter, bitmap);

    // ---- pass 1: argmax.  key = (ordered value << 32) | ~index: the maximum is the largest value at its lowest index
    u64 best = 0;
    uint32_t zbest = 0;   // controlled rows: the ordered maximum of z as well
    for (int s = 0; s < row.steps(); ++s) {
        const int c = row.chunk(wave, s, lane);
        if (c < 0) continue;
        uint32_t raw[8], mask;
        const int col0 = row.load(c, raw, mask);
        const auto ck = lg.chunk(row, c);
#pragma unroll
        for (int i = 0; i < E::N; ++i) {
            const u64 k = ((u64)greedy_key(lg.x(raw[i], ck, i)) << 32) | (uint32_t)~(uint32_t)(col0 + i);
            if (((mask >> i) & 1u) && k > best) best = k;
            if constexpr (CTL) {
                const uint32_t zk = greedy_key(lg.z(raw[i], ck, i));
                if (((mask >> i) & 1u) && zk > zbest) zbest = zk;
            }
        }
    }
    best = wave_max_u64(best);
    if (lane == 0) sh.wave64[wave] = best;
    __syncthreads();
    best = sh.wave64[0];
#pragma unroll
    for (int w = 1; w < kPickWaves; ++w) best = sh.wave64[w] > best ? sh.wave64[w] : best;
    __syncthreads();   // wave64 is reused by the scan
    if constexpr (CTL) {
        zbest = (uint32_t)wave_max_u64((u64)zbest);
        if (lane == 0) sh.wave64[wave] = zbest;
        __syncthreads();
        zbest = (uint32_t)sh.wave64[0];
#pragma unroll
        for (int w = 1; w < kPickWaves; ++w) zbest = (uint32_t)sh.wave64[w] > zbest ? (uint32_t)sh.wave64[w] : zbest;
        __syncthreads();
    }
    const uint32_t gkey = (uint32_t)(best >> 32);
    const int greedy = (int)~(uint32_t)best;
    const float xmax = greedy_unkey(gkey);   // garbage for a NaN, which is caught first

    int token = greedy;
    bool sampled = false;   // workgroup-uniform: the row is drawn from, not degenerate
    float st_lo = xmax, st_lse = xmax, st_count = 1.f, st_u = 0.f;
    if (p.do_sample) {
        const DropoutStream rs = dropout_stream(p.rng_state, (uint32_t)b);
        uint32_t r0, r1;
        philox2x32((uint32_t)counter, rs.salt, rs.key, r0, r1);
        const uint32_t n24 = r0 >> 8;
        st_u = ((float)n24 + 0.5f) * 0x1p-24f;
        // (a NaN row keeps the plain form: its zmax only reaches `stats`)
        const float zmax = CTL && gkey != 0xffffffffu ? greedy_unkey(zbest) : xmax * p.inv_t;
        st_lo = st_lse = zmax;
        const bool degenerate = gkey == 0xffffffffu || !(fabsf(zmax) < INFINITY);
        sampled = !degenerate;
        if (sampled) {
            float lo = -INFINITY;
            if (p.top_k > 0 && p.top_k < p.vocab) {
                const uint32_t k = radix_select<TAG, false>(row, sh, lg, zmax, lo, (u64)p.top_k, 1.f);
                lo = SelectKey<TAG>::threshold(k, p.inv_t);
            }
            if (p.top_p < 1.f) {
                const uint32_t k = radix_select<TAG, true>(row, sh, lg, zmax, lo, 0, p.top_p);
                lo = SelectKey<TAG>::threshold(k, p.inv_t);
            }
            // ---- the scan.  Lane sums, wave totals, the row's total (all integers: no order to fix)
            u64 acc = 0;
            int count = 0;
            float zmin = INFINITY;
            for (int s = 0; s < row.steps(); ++s) {
                const int c = row.chunk(wave, s, lane);
                if (c < 0) continue;
                uint32_t raw[8], mask;
                row.load(c, raw, mask);
                const auto ck = lg.chunk(row, c);
#pragma unroll
                for (int i = 0; i < E::N; ++i) {
                    const float z = lg.z(raw[i], ck, i);
                    if (((mask >> i) & 1u) && z >= lo) {
                        acc += fixed_mass(z, zmax);
                        ++count;
                        zmin = fminf(zmin, z);
                    }
                }
            }
            acc = wave_sum_u64(acc);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                count += __shfl_xor(count, o);
                zmin = fminf(zmin, __shfl_xor(zmin, o));
            }
            if (lane == 0) { sh.wave64[wave] = acc; sh.wavei[wave] = count; sh.wavef[wave] = zmin; }
            __syncthreads();
            u64 total = 0, before_wave = 0;
            count = 0;
            zmin = INFINITY;
#pragma unroll
            for (int w = 0; w < kPickWaves; ++w) {
                if (w == wave) before_wave = total;
                total += sh.wave64[w];
                count += sh.wavei[w];
                zmin = fminf(zmin, sh.wavef[w]);
            }
            // the draw: lowest t with C(t) > u S  <=>  C(t) > floor(u S) for the integers C; u S = (2 n + 1) S 2^-25
            u64 target = (u64)((double)(2u * n24 + 1u) * (double)total * 0x1p-25);
            if (target >= total) target = total - 1;   // total >= 2^40: the maximum itself is always kept
            st_lo = zmin;
            st_lse = zmax + fast_log2((float)total * (1.f / kFixedOne)) * kLn2;
            st_count = (float)count;
            const u64 mine = sh.wave64[wave];
            token = -1;
            if (before_wave <= target && target < before_wave + mine) {   // exactly one wave
                u64 run = before_wave;
                for (int s = 0; s < row.steps(); ++s) {
                    const int c = row.chunk(wave, s, lane);
                    uint32_t raw[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mask = 0;
                    int col0 = 0;
                    if (c >= 0) col0 = row.load(c, raw, mask);
                    const auto ck = lg.chunk(row, c);
                    u64 wgt[8], v = 0;
#pragma unroll
                    for (int i = 0; i < E::N; ++i) {
                        const float z = lg.z(raw[i], ck, i);
                        wgt[i] = (((mask >> i) & 1u) && z >= lo) ? fixed_mass(z, zmax) : 0ull;
                        v += wgt[i];
                    }
                    const u64 incl = wave_scan_u64(v, lane);
                    const u64 step_total = shfl_u64(incl, 63);
                    if (target < run + step_total) {   // wave-uniform
                        const u64 hit = __ballot(run + incl > target);
                        const int first = __ffsll((long long)hit) - 1;
                        if (lane == first) {
                            u64 cum = run + incl - v;
#pragma unroll
                            for (int i = 0; i < E::N; ++i) {
                                cum += wgt[i];
                                if (token < 0 && cum > target) token = col0 + i;
                            }
                        }
                        break;
                    }
                    run += step_total;
                }
            }
        }
    }
    if constexpr (PickTag<TAG>::phrases) {
        // the flag, `ends` and `reasons` wait for the stop phrases: thread 0 writes them behind the scan
        if (sampled ? token >= 0 : tid == 0) {
            *out.token = token;
            if (out.column) *out.column = token;
            sh.sel_digit = (uint32_t)token;
            sh.sel_above = ~0ull;
        }
        if (out.stats && tid == 0) {
            out.stats[0] = st_lo; out.stats[1] = st_lse; out.stats[2] = st_count; out.stats[3] = st_u;
        }
        __syncthreads();
        const int picked = (int)sh.sel_digit;
        if (tail.n > 0) tail.scan(out.column, picked, &sh.sel_above);   // workgroup-uniform
        __syncthreads();
        if (tid == 0 && tail.flag) {
            const bool eos = tail.eos >= 0 && picked == tail.eos;
            const u64 low = sh.sel_above;
            if (eos || low != ~0ull) {
                *tail.flag = 1;
                if (tail.ends) *tail.ends = tail.c + 1;
                if (tail.reasons) *tail.reasons = eos ? 0 : 1 + (int)low;
            }
        }
        return;
    } else if constexpr (PickTag<TAG>::lim) {
        if (sampled ? token >= 0 : tid == 0) {
            *out.token = token;
            if (out.column) *out.column = token;
            if (out.flag && token == p.eos) *out.flag = 1;
        }
        if (out.stats && tid == 0) {
            out.stats[0] = st_lo; out.stats[1] = st_lse; out.stats[2] = st_count; out.stats[3] = st_u;
        }
        return;
    }
    // the greedy answer is known to every thread (thread 0 writes it), a drawn token to the lane that found it
    if (sampled ? token >= 0 : tid == 0) {
        p.tokens[(int64_t)b * p.tokens_stride] = token;
        if (p.sequences && counter >= 0 && counter < p.seq_cols) p.sequences[(int64_t)b * p.seq_stride + counter] = token;
        if constexpr (CTL) {
            if (p.finished && p.eos >= 0 && token == p.eos) p.finished[b] = 1;
        }
    }
    if (p.stats && tid == 0) {
        float *st = p.stats + (int64_t)b * 4;
        st[0] = st_lo; st[1] = st_lse; st[2] = st_count; st[3] = st_u;
    }
}

// One workgroup per row of pick_token_kernel<TAG<ET>> with `lds` bytes of dynamic LDS (none for the plain form,
// TAG = Plain).  Each pick_token*.hip calls this once: the instantiations land in the caller's code object.
template <template <class> class TAG>
hipError_t launch_pick(const PickParams &p, size_t lds, int dtype, hipStream_t stream) {
    return with_row_dtype(dtype, [&](auto et) {
        auto kernel = pick_token_kernel<TAG<decltype(et)>>;
        if (lds > 48 * 1024) {   // ask for the large dynamic allocation by name
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kernel, dim3((unsigned)p.batch), dim3(kPickThreads), lds, stream, p);
        return hipGetLastError();
    });
}

}  // namespace bp
