// What the kernels that stream one vocabulary-sized row per workgroup share: xentropy.hip, score_rows.hip, pick_report.hip,
// row_extremes.hip, beam_pick.hip and the pick kernels of pick_core.h.  Nothing here is about picking a token.
//
//   RowElem<ET>     an element type (fp32, bf16, fp16): 16-byte loads as raw bits or as floats, stores, the order-preserving key
//   u64 helpers     shuffles, sum, maximum and prefix sum of 64-bit integers over a wave
//   keys            order_key / greedy_key: a float as an unsigned integer of the same order
//   statistics      the online softmax (m, s[, t]): the rescale of a thread's running sums, the two merges of partials, and
//                   the fixed-point mass whose sums do not depend on their order
//   the two walks   RowView (1024 threads, wave-contiguous) and RowSplit (256 threads, strided): see below
#pragma once
#include "bp_common.h"

namespace bp {

namespace {

typedef unsigned long long u64;

// ---- elements.  Raw forms: the bits of an element in the low end of a 32-bit word (`load`, `one`), its value (`to_f32`) and its
// order-preserving integer key (`key` / `unkey`: -0 < +0, NaNs at the ends by sign).  Float forms, for the kernels that
// only want values: `load_f32` / `one_f32`, and `store_f32` / `store_one_f32` (round to nearest even).
template <class ET> struct RowElem;
template <> struct RowElem<float> {
    static constexpr int N = 4, EB = 4, KEY_BITS = 32;
    static BP_DEV float to_f32(uint32_t raw) { return as_f32(raw); }
    static BP_DEV uint32_t one(const char *p) { return *reinterpret_cast<const uint32_t *>(p); }
    static BP_DEV void load(const char *p, uint32_t (&raw)[8]) {
        const u32x4 w = *reinterpret_cast<const u32x4 *>(p);
        const uint32_t a = w[0], b = w[1], c = w[2], d = w[3];
        raw[0] = a; raw[1] = b; raw[2] = c; raw[3] = d;
    }
    static BP_DEV uint32_t key(uint32_t raw) { return raw ^ ((raw & 0x80000000u) ? 0xffffffffu : 0x80000000u); }
    static BP_DEV uint32_t unkey(uint32_t k) { return k ^ ((k & 0x80000000u) ? 0x80000000u : 0xffffffffu); }

    static BP_DEV void load_f32(const char *p, float (&v)[8]) {
        const u32x4 w = *reinterpret_cast<const u32x4 *>(p);
        const uint32_t a = w[0], b = w[1], c = w[2], d = w[3];
        v[0] = as_f32(a); v[1] = as_f32(b); v[2] = as_f32(c); v[3] = as_f32(d);
    }
    static BP_DEV float one_f32(const char *p) { return *reinterpret_cast<const float *>(p); }
    static BP_DEV void store_f32(char *p, const float (&v)[8]) {
        *reinterpret_cast<u32x4 *>(p) = u32x4{as_u32(v[0]), as_u32(v[1]), as_u32(v[2]), as_u32(v[3])};
    }
    static BP_DEV void store_one_f32(char *p, float x) { *reinterpret_cast<float *>(p) = x; }
};
template <class H> struct RowElem16 {
    static constexpr int N = 8, EB = 2, KEY_BITS = 16;
    static BP_DEV float to_f32(uint32_t raw) { return Elem<H>::lo_f32(raw); }
    static BP_DEV uint32_t one(const char *p) { return *reinterpret_cast<const uint16_t *>(p); }
    static BP_DEV void load(const char *p, uint32_t (&raw)[8]) {
        const u32x4 w = *reinterpret_cast<const u32x4 *>(p);
        const uint32_t a = w[0], b = w[1], c = w[2], d = w[3];
        raw[0] = a & 0xffffu; raw[1] = a >> 16; raw[2] = b & 0xffffu; raw[3] = b >> 16;
        raw[4] = c & 0xffffu; raw[5] = c >> 16; raw[6] = d & 0xffffu; raw[7] = d >> 16;
    }
    static BP_DEV uint32_t key(uint32_t raw) { return raw ^ ((raw & 0x8000u) ? 0xffffu : 0x8000u); }
    static BP_DEV uint32_t unkey(uint32_t k) { return k ^ ((k & 0x8000u) ? 0x8000u : 0xffffu); }

    static BP_DEV void load_f32(const char *p, float (&v)[8]) {
        const u32x4 w = *reinterpret_cast<const u32x4 *>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t x = w[i];
            v[2 * i] = Elem<H>::lo_f32(x);
            v[2 * i + 1] = Elem<H>::hi_f32(x);
        }
    }
    static BP_DEV float one_f32(const char *p) { return Elem<H>::lo_f32(*reinterpret_cast<const uint16_t *>(p)); }
    static BP_DEV void store_f32(char *p, const float (&v)[8]) {
        const u32x4 w = u32x4{Elem<H>::pack2(v[0], v[1]), Elem<H>::pack2(v[2], v[3]),
                              Elem<H>::pack2(v[4], v[5]), Elem<H>::pack2(v[6], v[7])};
        *reinterpret_cast<u32x4 *>(p) = w;   // (non-temporal here: +5 % time in the cross-entropy backward -- the line was just read)
    }
    static BP_DEV void store_one_f32(char *p, float x) { *reinterpret_cast<uint16_t *>(p) = Elem<H>::from_float(x); }
};
template <> struct RowElem<BF16> : RowElem16<BF16> {};
template <> struct RowElem<F16> : RowElem16<F16> {};

// ---- 64-bit integers over a wave
BP_DEV u64 shfl_xor_u64(u64 v, int mask) {
    const uint32_t lo = __shfl_xor((uint32_t)v, mask), hi = __shfl_xor((uint32_t)(v >> 32), mask);
    return ((u64)hi << 32) | lo;
}
BP_DEV u64 shfl_up_u64(u64 v, int delta) {
    const uint32_t lo = __shfl_up((uint32_t)v, delta), hi = __shfl_up((uint32_t)(v >> 32), delta);
    return ((u64)hi << 32) | lo;
}
BP_DEV u64 shfl_u64(u64 v, int lane) {
    const uint32_t lo = __shfl((uint32_t)v, lane), hi = __shfl((uint32_t)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}
BP_DEV u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += shfl_xor_u64(v, o);
    return v;
}
BP_DEV u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const u64 w = shfl_xor_u64(v, o);
        v = w > v ? w : v;
    }
    return v;
}
// inclusive prefix sums over the lanes of a wave
BP_DEV u64 wave_scan_u64(u64 v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 w = shfl_up_u64(v, o);
        if (lane >= o) v += w;
    }
    return v;
}
BP_DEV uint32_t wave_scan_u32(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t w = __shfl_up(v, o);
        if (lane >= o) v += w;
    }
    return v;
}

// ---- keys.  The value part of an argmax key (value << 32 | ~column: the maximum is the largest value at its lowest column)
// order_key: -0 == +0, otherwise the order of the floats; a NaN is for the caller to key apart
BP_DEV uint32_t order_key(float x) {
    const uint32_t raw = as_u32(x + 0.f);   // -0 + 0 = +0
    return raw ^ ((raw & 0x80000000u) ? 0xffffffffu : 0x80000000u);
}
// the same with a NaN above everything (torch.argmax)
BP_DEV uint32_t greedy_key(float x) {
    if (x != x) return 0xffffffffu;
    return order_key(x);
}
BP_DEV float greedy_unkey(uint32_t k) { return as_f32(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xffffffffu)); }

// ---- online softmax statistics: m the maximum, s = sum e^(x - m), and for the entropy t = sum e^(x - m) x.
// The two merges of partial results are NOT one function with an optional third term: the cross-entropy multiplies inside the
// select (s * exp2(..), 0 for an empty partial) and adds the two products' roundings; the scoring kernels select the FACTOR
// and form s a + s2 b behind it, which contracts into a multiplication and an fma.  Different roundings, and the tests of
// each kernel pin its bits.
BP_DEV void merge_ms(float &m, float &s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    // exp2(-inf - -inf) would be NaN: an empty partial has s = 0 and is skipped by the select
    const float a = (m == -INFINITY) ? 0.f : s * fast_exp2((m - mn) * kLog2e);
    const float b = (m2 == -INFINITY) ? 0.f : s2 * fast_exp2((m2 - mn) * kLog2e);
    m = mn;
    s = a + b;
}
BP_DEV void merge_mst(float &m, float &s, float &t, float m2, float s2, float t2) {
    const float mn = fmaxf(m, m2);
    // exp2(-inf - -inf) would be NaN: an empty partial has s = t = 0 and is skipped by the select
    const float a = (m == -INFINITY) ? 0.f : fast_exp2((m - mn) * kLog2e);
    const float b = (m2 == -INFINITY) ? 0.f : fast_exp2((m2 - mn) * kLog2e);
    s = s * a + s2 * b;
    t = t * a + t2 * b;
    m = mn;
}

constexpr uint32_t kLowestBits = 0xff7fffffu;   // -FLT_MAX

// A thread's running (m, s, t) over the chunks it walks, rescaled only when the maximum moves.  Per chunk, with cm its
// maximum: if (cm > m) online_rescale(m, s, t, cm); then online_term() for each element against ms = online_shift(m),
// collecting the chunk's cs and ct; then s += cs, t += ct where the caller wants them.
BP_DEV void online_rescale(float &m, float &s, float &t, float cm) {   // m = -inf before: s = t = 0, exp2(-inf) = 0
    const float f = fast_exp2((m - cm) * kLog2e);
    s *= f;
    t *= f;
    m = cm;
}
BP_DEV float online_shift(float m) { return (m == -INFINITY) ? 0.f : m; }   // -inf - -inf would be a NaN
// one element: e = e^(x - ms) goes to cs, e x to ct
BP_DEV void online_term(float x, float ms, float &cs, float &ct) {
    const float e = fast_exp2((x - ms) * kLog2e);
    cs += e;
    // a -inf entry has e = 0 and must add 0, not 0 * -inf: its bits, the largest of the negative numbers as an unsigned
    // integer, are clamped to those of -FLT_MAX (one v_min_u32; every other number keeps its bits)
    ct = fmaf(e, as_f32(min(as_u32(x), kLowestBits)), ct);
}

// exp(z - m) in fixed point, 2^-40 a unit, as a 64-bit integer: sums of these do not depend on their order.  z <= m, m finite
constexpr float kFixedOne = 1099511627776.f;   // 2^40
BP_DEV u64 fixed_mass(float z, float m) { return (u64)(fast_exp2((z - m) * kLog2e) * kFixedOne); }

// ---- the two ways of walking a row.  Both read 16 bytes at a time on 16-byte boundaries of the address space and the
// elements in front of the first boundary and behind the last one by one; no kernel is to be moved from one to the other.
//
// RowView: 1024 threads, WAVE-CONTIGUOUS -- wave w owns the chunks [w cpw, (w + 1) cpw), lane l of step s the chunk 64 s + l
// of them.  For the kernels that need the vocabulary ORDER of what they find (the cumulative scan of the pick, the ties of
// row_extremes) or walk the row several times from L2 with 16 waves to hide the latency: pick_core.h, pick_report.hip,
// row_extremes.hip, beam_pick.hip.  Edge chunks come with a `mask`, so every pass has one loop body.
//
// RowSplit: 256 threads, STRIDED -- thread t takes the body chunks t, t + 256, ...; head and tail are walked element-wise.
// For the single-pass, HBM-bound kernels whose body loop must be free of masks and of a per-chunk edge test:
// xentropy.hip (forward and backward) and score_rows.hip.
constexpr int kPickThreads = 1024;
constexpr int kPickWaves = kPickThreads / 64;
// the radix-select histograms of the 1024-thread kernels: 32 copies (lane & 31) of 256 bins, a copy stride of 257 words
constexpr int kHistCopies = 32;
constexpr int kHistStride = 257;

// The row as seen by one lane: chunks of N elements on 16-byte boundaries of the address space (chunk 0 starts at or
// before the row), wave w owning the chunks [w cpw, (w + 1) cpw).  Chunks that reach outside the row are read element
// by element; `mask` has a bit per valid element.
template <class ET> struct RowView {
    using E = RowElem<ET>;
    const char *vbase;   // address of chunk 0
    int head, vocab, nch, cpw;
    BP_DEV RowView(const char *row, int vocab_) : vocab(vocab_) {
        head = (int)((reinterpret_cast<uintptr_t>(row) & 15u) / E::EB);
        vbase = row - head * E::EB;
        nch = (vocab + head + E::N - 1) / E::N;
        cpw = (nch + kPickWaves - 1) / kPickWaves;
    }
    BP_DEV int steps() const { return (cpw + 63) / 64; }
    // chunk of (wave, step, lane), -1 past the wave's run
    BP_DEV int chunk(int wave, int step, int lane) const {
        const int local = step * 64 + lane;
        const int c = wave * cpw + local;
        return (local < cpw && c < nch) ? c : -1;
    }
    // returns the column of element 0 of the chunk (may be negative for chunk 0)
    BP_DEV int load(int c, uint32_t (&raw)[8], uint32_t &mask) const {
        const int col0 = c * E::N - head;
        if (col0 >= 0 && col0 + E::N <= vocab) {
            E::load(vbase + (int64_t)c * 16, raw);
            mask = (1u << E::N) - 1u;
        } else {
            mask = 0;
#pragma unroll
            for (int i = 0; i < E::N; ++i) {
                const int col = col0 + i;
                const bool ok = col >= 0 && col < vocab;
                raw[i] = ok ? E::one(vbase + ((int64_t)c * E::N + i) * E::EB) : 0u;
                if (ok) mask |= 1u << i;
            }
        }
        return col0;
    }
};

// Head, 16-byte body and tail of a row of `cols` elements for the strided walk: columns [0, nhead) in front of the first
// boundary, nvec chunks of N from there, [tail0, cols) behind them.  vectors = false: no body (everything is head).
template <class ET> struct RowSplit {
    using E = RowElem<ET>;
    int nhead, nvec, tail0;
    BP_DEV RowSplit(const char *row, int cols, bool vectors = true) {
        const int head = (int)(((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) / E::EB);
        nhead = vectors ? min(head, cols) : cols;
        nvec = (cols - nhead) / E::N;
        tail0 = nhead + nvec * E::N;
    }
    BP_DEV int col0(int c) const { return nhead + c * E::N; }   // first column of body chunk c
    // head and tail as ONE run of loose elements: their number, and the column of the c-th
    BP_DEV int loose(int cols) const { return nhead + (cols - tail0); }
    BP_DEV int loose_col(int c) const { return c < nhead ? c : tail0 + (c - nhead); }
};

}  // namespace

}  // namespace bp
