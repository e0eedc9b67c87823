// Sense kernels for WIDE senses, 128 < d_k <= 640 (gfx950).
//
// The reference's few-sense ablations -- training/configs/experiment/owt/backpack-mini-flash-vecs-4.yaml (k = 4, d_k = 160)
// and ...-vecs-1.yaml (k = 1, d_k = 640) -- lie beyond the width the LDS-DMA kernels (and the reference's own attention
// kernels, csrc/flash_attn/fmha_api.cpp:245) take: a query's fragments no longer fit the register file next to the
// accumulators.  These three kernels cover them natively; same tile algebra as the rest of this directory (bp_common.h:
// S^T = K Q^T on v_mfma_f32_32x32x16, one query per lane, P^T straight into the second GEMM), with two changes:
//   * a query's fragments for one sense stay in REGISTERS for the whole key sweep in both width classes -- 48 registers up
//     to d_k = 192, 160 up to d_k = 640, where the workgroup's one wave per SIMD owns the whole 512-entry file and hipcc
//     parks what exceeds the 256 architectural registers in accumulation registers (no scratch) -- while the K rows of a
//     32-key block sit in LDS (up to 1296 bytes each);
//   * d_k is a run-time loop bound inside its class: one instantiation per dtype, alignment class and width class.
// With few senses this path is small next to the trunk (k = 1: 3 % of the Mini k = 64 mix flops), so the schedule is the
// simple one of flash_fwd.hip / sense_mix.hip (tiles staged through registers into a double-buffered LDS image, one
// __syncthreads per key block), not a ring.
//   sense_lse_wide_kernel    log-sum-exp of every (sense, query) row          (reference backpack.py:116-122, first half)
//   sense_alpha_wide_kernel  alpha (B,k,S,S) materialised, zeros above the diagonal     (backpack.py:116-122)
//   sense_mix_wide_kernel    out = sum_l alpha_l C_l, alpha never stored               (backpack.py:313)
#include "bp_common.h"
#include "bp_kernels.h"
#include "staged_tile.h"

namespace bp {

// KDT: compile-time bound of the 16-column steps of the sense width.  Two classes are instantiated:
//   KDT = 12  (d_k <= 192, e.g. vecs-4's 160): 48 fragment registers, 12.8 KB K tiles, two (mix: registers) to six (LSE,
//             alpha: LDS) workgroups per CU;
//   KDT = 40  (d_k <= 640, vecs-1): 160 fragment registers (the first version re-fetched them per key block from the L2:
//             33 ms per mix launch at Mini k = 1, B = 1024, profiles/r06_d_bench_mini_k1_native.json), 41.5 KB K tiles,
//             one workgroup per CU.
template <int KDT>
struct WideCfgT {
    static constexpr int BM = 128;                 // queries per workgroup (4 waves x 32)
    static constexpr int BK = 32;                  // keys per block
    static constexpr int NT = 256;
    static constexpr int KD_MAX = KDT;
    static constexpr int KTILE_MAX = BK * k_pitch(KD_MAX);
    static constexpr int K_ITERS_MAX = tile_iters(BK, KD_MAX * 2, NT);
    static constexpr int NB = 4;                   // 32-column blocks of the output per workgroup (mix)
    static constexpr int CROW = NB * 64;
    static constexpr int CTILE = BK * CROW;        // 8 192 bytes
    static constexpr int CCH = NB * 4;
    static constexpr int C_ITERS = tile_iters(BK, CCH, NT);   // 2
};
constexpr int kWideSmallKd = 12, kWideLargeKd = 40;

// WideKLoader, wide_load_q and the alpha kernel's store4 serve sense_lse_wide_kernel and sense_alpha_wide_kernel only;
// sense_mix_wide_kernel uses the same steps from staged_tile.h.  On the shared functions the two kernels missed their
// same-speed bound against the parent at S = 1000, d_k = 160 (0.0416 against 0.0412 ms, 0.0555 against 0.0546 + 0.0005;
// profiles/README.md "staged tiles"), so their text went back and their code is the parent's.
// K rows [kb*32, kb*32+32) of one sense -> registers -> LDS image (row pitch krow = 32*KD + 16 bytes: conflict-free b128)
template <bool VEC, int KDT>
struct WideKLoader {
    using WideCfg = WideCfgT<KDT>;
    u32x4 reg[WideCfg::K_ITERS_MAX];
    BP_DEV void fetch(const uint16_t *kg, int64_t k_rs, int kb, int S, int dk, int kd, int tid) {
        const int kch = kd * 2;
#pragma unroll
        for (int i = 0; i < WideCfg::K_ITERS_MAX; ++i) {
            const int c = tid + i * WideCfg::NT;
            const int row = c / kch, ch = c - row * kch;
            const int key = kb * WideCfg::BK + row;
            u32x4 v = {0u, 0u, 0u, 0u};   // keys past the sequence and columns past d_k are ZERO
            if (c < WideCfg::BK * kch && key < S && ch * 8 < dk) {
                const uint16_t *r = kg + (int64_t)key * k_rs;
                v = VEC ? ld_global_16B(r + ch * 8) : ld_global_8x2B(r, ch * 8, dk);
            }
            reg[i] = v;
        }
    }
    BP_DEV void stash(char *kbuf, int kd, int tid) const {
        const int kch = kd * 2, krow = kd * 32 + 16;
#pragma unroll
        for (int i = 0; i < WideCfg::K_ITERS_MAX; ++i) {
            const int c = tid + i * WideCfg::NT;
            const int row = c / kch, ch = c - row * kch;
            if (c < WideCfg::BK * kch) lds_write_16B(kbuf, row * krow + ch * 16, reg[i]);
        }
    }
};

// The query fragments of my row for one sense (B operand of S^T = K Q^T): column 16 s + 8 hh .. +7 of step s.
template <bool VEC, int KDT>
BP_DEV void wide_load_q(u32x4 (&qf)[KDT], const uint16_t *qrow, bool q_valid, int dk, int hh) {
#pragma unroll
    for (int s = 0; s < KDT; ++s) {
        const int col = 16 * s + 8 * hh;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (q_valid && col < dk) v = VEC ? ld_global_16B(qrow + col) : ld_global_8x2B(qrow, col, dk);
        qf[s] = v;
    }
}

struct WideParams {          // the three kernels' common part (all strides in 16-bit elements)
    const uint16_t *q, *k;   // q_l[t] = q + b*qk_bs + t*qk_rs + l*qk_ss
    int64_t qk_bs, qk_rs, qk_ss;
    float *lse;              // (b, nsenses, lse_stride) fp32, natural log
    int64_t lse_stride;
    int b, s, nsenses, dk;
    float scale_log2e;
};

// ---- LSE ------------------------------------------------------------------------------------------------------------
template <class ET, bool VEC, int KDT>
__global__ __launch_bounds__(256) void sense_lse_wide_kernel(const WideParams p) {
    using WideCfg = WideCfgT<KDT>;
    __shared__ __attribute__((aligned(16))) char smem[2 * WideCfg::KTILE_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hh = lane >> 5;
    const int n_qtiles = (p.s + WideCfg::BM - 1) / WideCfg::BM;
    int grp, slot;
    if (!xcd_map(blockIdx.x, p.b * p.nsenses, n_qtiles, grp, slot)) return;
    const int qt = n_qtiles - 1 - slot;
    const int batch = grp / p.nsenses, l = grp - batch * p.nsenses;
    const int S = p.s, dk = p.dk, kd = (dk + 15) / 16;
    const int ktile = WideCfg::BK * (kd * 32 + 16);
    const uint16_t *qg = p.q + batch * p.qk_bs + (int64_t)l * p.qk_ss;
    const uint16_t *kg = p.k + batch * p.qk_bs + (int64_t)l * p.qk_ss;
    const int k_end = min(S, qt * WideCfg::BM + WideCfg::BM);
    const int nkb = (k_end + WideCfg::BK - 1) / WideCfg::BK;
    const int q0 = qt * WideCfg::BM + wave * 32, my_q = q0 + l31;
    const bool wave_has_rows = q0 < S;
    const int my_last_kb = q0 / WideCfg::BK;
    const float c2 = p.scale_log2e;
    const uint16_t *qrow = qg + (int64_t)min(my_q, S - 1) * p.qk_rs;

    WideKLoader<VEC, KDT> ld;
    u32x4 qf[KDT];
    wide_load_q<VEC, KDT>(qf, qrow, my_q < S, dk, hh);
    float m_run = -INFINITY, l_run = 0.f;
    ld.fetch(kg, p.qk_rs, 0, S, dk, kd, tid);
    ld.stash(smem, kd, tid);
    __syncthreads();
    for (int kb = 0; kb < nkb; ++kb) {
        const int cur = kb & 1;
        if (kb + 1 < nkb) ld.fetch(kg, p.qk_rs, kb + 1, S, dk, kd, tid);
        if (wave_has_rows && kb <= my_last_kb) {
            f32x16 st = st_half_wide<ET>(smem + cur * ktile, qf, kd, l31, hh);
            const int lim = min(S - 1, my_q) - kb * WideCfg::BK - 4 * hh;   // last visible key of my row, as st_key(0, r, 0) of my half-wave
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (st_key(0, r, 0) > lim) st[r] = -INFINITY;
            float mx = st[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[r]);
            mx = xhalf_max(mx);
            const float m_new = fmaxf(m_run, mx);
            const float mc = (m_new == -INFINITY) ? 0.f : m_new * c2;
            const float alpha = fast_exp2(m_run * c2 - mc);
            m_run = m_new;
            float rs = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) rs += fast_exp2(fmaf(st[r], c2, -mc));
            l_run = l_run * alpha + rs;
        }
        if (kb + 1 < nkb) ld.stash(smem + (cur ^ 1) * ktile, kd, tid);
        __syncthreads();
    }
    if (!wave_has_rows || my_q >= S) return;
    const float l_tot = xhalf_sum(l_run);
    if (hh == 0)
        p.lse[((int64_t)batch * p.nsenses + l) * p.lse_stride + my_q] =
            l_tot > 0.f ? (m_run * c2 + fast_log2(l_tot)) * kLn2 : -INFINITY;
}

// ---- alpha materialised ------------------------------------------------------------------------------------------------
struct WideAlphaParams {
    WideParams w;
    uint16_t *alpha;          // (b, nsenses, s, s) 16-bit, contiguous
    int vec_store;            // 8-byte stores of 4 keys are aligned (s % 4 == 0, base aligned)
};

template <class ET, bool VEC, int KDT>
__global__ __launch_bounds__(256) void sense_alpha_wide_kernel(const WideAlphaParams pa) {
    using E = Elem<ET>;
    using WideCfg = WideCfgT<KDT>;
    const WideParams &p = pa.w;
    __shared__ __attribute__((aligned(16))) char smem[2 * WideCfg::KTILE_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hh = lane >> 5;
    const int n_qtiles = (p.s + WideCfg::BM - 1) / WideCfg::BM;
    int grp, slot;
    if (!xcd_map(blockIdx.x, p.b * p.nsenses, n_qtiles, grp, slot)) return;
    const int qt = n_qtiles - 1 - slot;
    const int batch = grp / p.nsenses, l = grp - batch * p.nsenses;
    const int S = p.s, dk = p.dk, kd = (dk + 15) / 16;
    const int ktile = WideCfg::BK * (kd * 32 + 16);
    const uint16_t *qg = p.q + batch * p.qk_bs + (int64_t)l * p.qk_ss;
    const uint16_t *kg = p.k + batch * p.qk_bs + (int64_t)l * p.qk_ss;
    const int k_end = min(S, qt * WideCfg::BM + WideCfg::BM);
    const int nkb = (k_end + WideCfg::BK - 1) / WideCfg::BK;
    const int q0 = qt * WideCfg::BM + wave * 32, my_q = q0 + l31;
    const bool wave_has_rows = q0 < S;
    const int my_last_kb = q0 / WideCfg::BK;
    const float c2 = p.scale_log2e;
    const uint16_t *qrow = qg + (int64_t)min(my_q, S - 1) * p.qk_rs;
    const float lse2 = (wave_has_rows && my_q < S)
                           ? p.lse[((int64_t)batch * p.nsenses + l) * p.lse_stride + my_q] * kLog2e : 0.f;
    uint16_t *arow = pa.alpha + (((int64_t)batch * p.nsenses + l) * S + min(my_q, S - 1)) * S;

    auto store4 = [&](int key0, float x0, float x1, float x2, float x3) {   // 4 consecutive keys of my row
        if (pa.vec_store) {
            if (key0 < S) {   // (s % 4 == 0: a group is inside or outside as a whole)
                const u32x2 w = {E::pack2(x0, x1), E::pack2(x2, x3)};
                *reinterpret_cast<u32x2 *>(arow + key0) = w;
            }
        } else {
            if (key0 + 0 < S) arow[key0 + 0] = E::from_float(x0);
            if (key0 + 1 < S) arow[key0 + 1] = E::from_float(x1);
            if (key0 + 2 < S) arow[key0 + 2] = E::from_float(x2);
            if (key0 + 3 < S) arow[key0 + 3] = E::from_float(x3);
        }
    };

    WideKLoader<VEC, KDT> ld;
    u32x4 qf[KDT];
    wide_load_q<VEC, KDT>(qf, qrow, my_q < S, dk, hh);
    ld.fetch(kg, p.qk_rs, 0, S, dk, kd, tid);
    ld.stash(smem, kd, tid);
    __syncthreads();
    for (int kb = 0; kb < nkb; ++kb) {
        const int cur = kb & 1;
        if (kb + 1 < nkb) ld.fetch(kg, p.qk_rs, kb + 1, S, dk, kd, tid);
        if (wave_has_rows && kb <= my_last_kb) {
            f32x16 st = st_half_wide<ET>(smem + cur * ktile, qf, kd, l31, hh);
            const int lim = my_q - kb * WideCfg::BK - 4 * hh;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float e = fast_exp2(fmaf(st[r], c2, -lse2));
                if (st_key(0, r, 0) > lim) e = 0.f;      // above the diagonal: exact zeros
                st[r] = e;
            }
            if (my_q < S) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    store4(kb * WideCfg::BK + 8 * g + 4 * hh, st[4 * g], st[4 * g + 1], st[4 * g + 2], st[4 * g + 3]);
            }
        }
        if (kb + 1 < nkb) ld.stash(smem + (cur ^ 1) * ktile, kd, tid);
        __syncthreads();
    }
    // the key blocks entirely above my wave's rows: zeros, written explicitly (the caller's buffer is uninitialised)
    if (wave_has_rows && my_q < S) {
        const int nkb_all = (S + WideCfg::BK - 1) / WideCfg::BK;
        for (int kb = my_last_kb + 1; kb < nkb_all; ++kb)
#pragma unroll
            for (int g = 0; g < 4; ++g) store4(kb * WideCfg::BK + 8 * g + 4 * hh, 0.f, 0.f, 0.f, 0.f);
    }
}

// ---- fused mix -----------------------------------------------------------------------------------------------------------
template <class ET, bool VEC_QK, bool VEC_C, int KDT>
__global__ __launch_bounds__(256) void sense_mix_wide_kernel(const MixParams p) {
    using W = WideCfgT<KDT>;
    __shared__ __attribute__((aligned(16))) char smem[2 * (W::KTILE_MAX + W::CTILE)];
    const LaneCoord L = lane_coord();
    const int tid = L.tid, l31 = L.l31, hh = L.hh;
    const int S = p.s, dk = p.dk, kd = (dk + 15) / 16;
    const int ktile = W::BK * k_pitch(kd), stage = ktile + W::CTILE;
    const int n_qtiles = (S + W::BM - 1) / W::BM;
    const int n_chunks = (p.dout + W::NB * 32 - 1) / (W::NB * 32);
    int grp, slot;
    if (!xcd_map(blockIdx.x, p.b * n_chunks, n_qtiles, grp, slot)) return;
    const int qt = n_qtiles - 1 - slot;
    const int batch = grp / n_chunks, chunk = grp - batch * n_chunks;
    const int col_base = chunk * W::NB * 32;
    const uint16_t *qg = reinterpret_cast<const uint16_t *>(p.q) + batch * p.qk_bs;
    const uint16_t *kg = reinterpret_cast<const uint16_t *>(p.k) + batch * p.qk_bs;
    const uint16_t *cg = reinterpret_cast<const uint16_t *>(p.c) + batch * p.c_bs;
    const int k_end = min(S, qt * W::BM + W::BM);
    const int nkb = (k_end + W::BK - 1) / W::BK;
    const int nsteps = p.nsenses * nkb;
    const QueryRows R = query_rows(L, qt * W::BM, S);
    const int q0 = R.q0, my_q = R.my_q;
    const bool wave_has_rows = R.wave_has_rows;
    const int my_last_kb = q0 / W::BK;
    const float c2 = p.scale_log2e;
    const int nb_live = min(W::NB, (p.dout - col_base + 31) / 32);

    u32x4 qf[KDT];
    u32x4 kreg[W::K_ITERS_MAX];
    u32x4 creg[W::C_ITERS];
    auto fetch = [&](int step) {
        const int l = step / nkb, kb = step - l * nkb;
        k_fetch<VEC_QK, W::BK, W::NT>(kreg, kg + (int64_t)l * p.qk_ss, p.qk_rs, kb * W::BK, S, dk, kd, tid);
        c_fetch<VEC_C, W::NB, W::BK, W::NT>(creg, cg + (int64_t)l * p.c_ss, p.c_rs, kb * W::BK, S, col_base, p.dout, tid);
    };
    auto stash = [&](int buf) {
        char *kb_ = smem + buf * stage;
        k_stash<W::BK, W::NT>(kreg, kb_, kd, tid);
        c_stash<W::NB, W::BK, W::NT>(creg, kb_ + ktile, tid);
    };

    f32x16 acc[W::NB];
#pragma unroll
    for (int n = 0; n < W::NB; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    const TrLane tr = tr_lane(L);
    float lse2 = 0.f;

    fetch(0);
    stash(0);
    __syncthreads();
    for (int step = 0; step < nsteps; ++step) {
        const int cur = step & 1;
        const int l = step / nkb, kb = step - l * nkb;
        if (step + 1 < nsteps) fetch(step + 1);
        if (kb == 0 && wave_has_rows) {   // new sense: my row's log-sum-exp (and its fragments, when they live in registers)
            lse2 = (my_q < S) ? p.lse[((int64_t)batch * p.nsenses + l) * p.lse_stride + my_q] * kLog2e : 0.f;
            load_q_frags<VEC_QK>(qf, qg + (int64_t)l * p.qk_ss, p.qk_rs, my_q, S, dk, hh);
        }
        if (wave_has_rows && kb <= my_last_kb) {
            const char *kbuf = smem + cur * stage;
            const char *cbuf = kbuf + ktile;
            f32x16 st = st_half_wide<ET>(kbuf, qf, kd, l31, hh);
            const int lim = my_q - kb * W::BK - 4 * hh;
            const float *kw = p.kw != nullptr ? p.kw + batch * p.kw_bs + (int64_t)l * p.kw_ss : nullptr;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rel = st_key(0, r, 0);
                float e = fast_exp2(fmaf(st[r], c2, -lse2));
                if (rel > lim || my_q >= S) e = 0.f;
                if (kw != nullptr) e *= kw[min(st_key(kb * W::BK, r, hh), S - 1)];   // intervention hook
                st[r] = e;
            }
            accumulate_pv<ET>(acc, st, cbuf, 0, tr, nb_live);
        }
        if (step + 1 < nsteps) stash(cur ^ 1);
        __syncthreads();
    }

    if (!wave_has_rows || my_q >= S) return;
    uint16_t *og = reinterpret_cast<uint16_t *>(p.o) + batch * p.o_bs + (int64_t)my_q * p.o_rs;
    store_acc_row<ET, VEC_C>(og, acc, col_base, p.dout, hh);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
// the LSE / alpha kernels' operands out of the mix operands; `lse` is written (LSE) or read (alpha)
static WideParams wide_params(const MixParams &p, float *lse) {
    return WideParams{static_cast<const uint16_t *>(p.q), static_cast<const uint16_t *>(p.k), p.qk_bs, p.qk_rs, p.qk_ss,
                      lse, p.lse_stride, p.b, p.s, p.nsenses, p.dk, p.scale_log2e};
}

// one instantiation per (dtype, alignment class, width class): f(element type, VEC, KDT)
template <class F> static hipError_t with_wide(int dtype, bool vec, int dk, F &&f) {
    return with_dtype(dtype, [&](auto et) {
        return with_flag(vec, [&](auto v) {
            if (dk <= 16 * kWideSmallKd) return f(et, v, std::integral_constant<int, kWideSmallKd>{});
            return f(et, v, std::integral_constant<int, kWideLargeKd>{});
        });
    });
}

hipError_t launch_sense_lse_wide(const MixParams &p, float *lse, int dtype, bool vec, hipStream_t stream) {
    const WideParams w = wide_params(p, lse);
    const dim3 grid(xcd_grid(p.b * p.nsenses, (p.s + 127) / 128)), block(256);
    return with_wide(dtype, vec, p.dk, [&](auto et, auto v, auto kdt) {
        hipLaunchKernelGGL((sense_lse_wide_kernel<decltype(et), v, kdt>), grid, block, 0, stream, w);
        return hipGetLastError();
    });
}

hipError_t launch_sense_alpha_wide(const MixParams &p, void *alpha, int dtype, bool vec, hipStream_t stream) {
    WideAlphaParams pa;
    pa.w = wide_params(p, const_cast<float *>(p.lse));
    pa.alpha = static_cast<uint16_t *>(alpha);
    pa.vec_store = (p.s % 4 == 0) && ((reinterpret_cast<uintptr_t>(alpha) & 7) == 0);
    const dim3 grid(xcd_grid(p.b * p.nsenses, (p.s + 127) / 128)), block(256);
    return with_wide(dtype, vec, p.dk, [&](auto et, auto v, auto kdt) {
        hipLaunchKernelGGL((sense_alpha_wide_kernel<decltype(et), v, kdt>), grid, block, 0, stream, pa);
        return hipGetLastError();
    });
}

hipError_t launch_sense_mix_wide(const MixParams &p, int dtype, bool vec_qk, bool vec_c, hipStream_t stream) {
    return with_wide(dtype, vec_qk, p.dk, [&](auto et, auto vq, auto kdt) {
        using W = WideCfgT<kdt>;
        const int n_qtiles = (p.s + W::BM - 1) / W::BM;
        const int n_chunks = (p.dout + W::NB * 32 - 1) / (W::NB * 32);
        const dim3 grid(xcd_grid(p.b * n_chunks, n_qtiles)), block(W::NT);
        return with_flag(vec_c, [&](auto vc) {
            hipLaunchKernelGGL((sense_mix_wide_kernel<decltype(et), vq, vc, kdt>), grid, block, 0, stream, p);
            return hipGetLastError();
        });
    });
}

}  // namespace bp
