// Backward of the fused Backpack sense combination (second half) for gfx950.
//
// Forward (sense_mix_dma.hip):  out[t,:] = sum_l sum_{s<=t} P_l[t,s] C[s,l,:],  P_l[t,s] = exp(scale q_l[t].k_l[s] - lse_l[t])
// The reference leaves this to autograd through `torch.sum(contextualization @ content, dim=1)` and the softmax
// (training/src/models/backpack.py:116-122,313), which keeps three (B,k,S,S) fp32 tensors alive.  Here nothing of
// that size exists; P is recomputed from the saved log-sum-exp, as the attention backward does.
//
//   dC[s,l,:]  = sum_{t>=s} P_l[t,s] dout[t,:]                                     -> sense_mix_dc_kernel (this file)
//   dP_l[t,s]  = dout[t,:] . C[s,l,:]          (a 768-deep contraction: a plain GEMM, done by the BLAS library in
//                                               slabs of 128 queries into a (B, S*k, 128) buffer, see bp_hip/__init__.py)
//   D_l[t]     = sum_s P_l[t,s] dP_l[t,s]
//   dS_l[t,s]  = P_l[t,s] (dP_l[t,s] - D_l[t])
//   dq_l[t]    = scale sum_s dS_l[t,s] k_l[s]                                      -> sense_dq_kernel
//   dk_l[s]    = scale sum_t dS_l[t,s] q_l[t]                                      -> sense_dk_kernel
//
// sense_mix_dc_kernel is the forward kernel with the roles of queries and keys exchanged: a workgroup owns 256 KEYS
// x 256 output columns (8 waves x 32 keys, K_l fragments and the accumulators dC^T in registers), streams 64-query
// tiles of Q_l, dout and lse_l through the same 3-slot LDS-DMA ring, and flushes / clears its accumulators once per
// sense.  S = Q K^T comes out with lane = key and the queries along the registers, which is the B-operand layout of
// dC^T = dout^T P.  Same persistent job queues (heaviest key tile = tile 0 first), same pinned MFMA / softmax
// interleave in the steps that need no masking.
#include <atomic>

#include "bp_common.h"
#include "bp_dma.h"
#include "bp_kernels.h"
#include "mix_ring.h"

namespace bp {

// the ring of mix_ring.h: A = Q rows, B = dout rows, aux = lse of the tile's 64 queries
template <int KD> using MixDcCfg = MixRingCfg<KD, true>;

template <class ET, int KD, bool FULL>
__global__ __launch_bounds__(512) void sense_mix_dc_kernel(const MixBwdParams p) {
    using C = MixDcCfg<KD>;
    using E = Elem<ET>;
    __shared__ __attribute__((aligned(16))) char smem[C::SMEM];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const int S = p.s;
    const float c2 = p.scale_log2e;
    const uint32_t lds0 = lds_base_addr(smem);

    const MixTileReader<C> rd(lane);
    uint32_t exhausted = 0;   // job queues with no jobs left (mix_take_job)

    for (int word; (word = mix_take_job<C>(smem, p.queues, exhausted, p.b, p.n_chunks, p.n_ktiles)) >= 0;) {
        const MixJob job = mix_decode_job<C>(word, p.n_chunks);
        const int batch = job.batch, col_base = job.col_base;
        const int kt = job.rank;   // key tile 0 = the most query tiles = the heaviest first

        const uint16_t *qg = reinterpret_cast<const uint16_t *>(p.q) + batch * p.qk_bs;
        const uint16_t *kg = reinterpret_cast<const uint16_t *>(p.k) + batch * p.qk_bs;
        const uint16_t *dg = reinterpret_cast<const uint16_t *>(p.dout) + batch * p.do_bs;

        const int key0 = kt * C::BM + wave * 32;
        const int my_key = key0 + l31;
        const int my_key_clamped = min(my_key, S - 1);
        const bool wave_has_keys = key0 < S;
        const int my_key_sub = key0 >> 5;
        const int nb_live = FULL ? C::NB : min(C::NB, (p.dout_cols - col_base + 31) / 32);

        // query tiles (64 queries) of this job: [qb_begin, nqb); masks needed before qb_clean and in a partial last tile
        const int nqb = (S + C::BK - 1) / C::BK;
        const int qb_begin = (kt * C::BM) / C::BK;
        const int qb_full_end = S / C::BK;
        const int qb_clean = min(qb_begin + C::BM / C::BK, nqb);

        // the DMA side of the job (mix_ring.h): query tiles [qb_begin, nqb) of every sense; dout does not depend on the sense
        MixStream<C> ring;
        ring.begin_job(lds0, wave, lane, S, p.nsenses, qb_begin, S, qg, p.qk_rs, p.qk_ss, p.dk, dg, p.do_rs, 0);
        uint32_t d_voff[C::B_DMA];
        ring.template b_offsets<FULL>(d_voff, p.do_rs, col_base, p.dout_cols);
        auto issue = [&](int slot, uint32_t pieces) {
            ring.issue(
                slot, pieces,
                [&](int j, int back, uint32_t lds_dst) { dma16_s(ring.bt2, d_voff[j] - (uint32_t)(back * p.do_rs) * 2u, lds_dst); },
                [&](int l) { return p.lse + ((int64_t)batch * p.nsenses + l) * p.lse_stride; });   // lse[b, l, :]
        };
        constexpr uint32_t kAllPieces = C::ALL_PIECES;

        f32x16 acc[C::NB];
        u32x4 kf[KD];
#pragma unroll
        for (int s = 0; s < KD; ++s) kf[s] = u32x4{0u, 0u, 0u, 0u};
        auto take_k = [&](int l) {
            const uint16_t *row = kg + (int64_t)my_key_clamped * p.qk_rs + (int64_t)l * p.qk_ss;
#pragma unroll
            for (int s = 0; s < KD; ++s) {
                const int col = 16 * s + 8 * hh;
                u32x4 v = {0u, 0u, 0u, 0u};
                if (col < p.dk) v = ld_global_16B(row + col);
                kf[s] = v;
            }
        };

        // lse (in log2 units) of the queries my registers hold: four runs of four consecutive queries
        auto row_lse = [&](int stage, int kk, float (&l2)[16]) {
            const int base = stage + C::AUX_OFF + wave * 256 + (kk * 32 + 4 * hh) * 4;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const u32x4 w4 = lds_read_16B(smem, base + g * 32);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t wi = w4[i];   // by-value copy (bp_common.h, as_f32)
                    l2[4 * g + i] = as_f32(wi) * kLog2e;
                }
            }
        };
        // dC^T += dout^T P over the 16-query steps pk[] from query row `row0` of the tile at `stage` (one operand stream)
        auto pv_stream = [&](int stage, int row0, const auto &pk, auto &&mid) {
            mix_pv_stream<E, C, FULL>(smem, rd, acc, nb_live, stage, row0, pk, mid);
        };

        // ---- steady-state step (every query of the tile exists and sees every key of the workgroup), cut as in
        // sense_mix_dma.hip into a vector-heavy half X (S of both query halves as one operand stream, softmax of half 0,
        // the first 8 MFMAs of half 0 with the exponentials of half 1 between them, pack) and a matrix-only half Y (the
        // other 24 MFMAs); the two waves of a SIMD (w, w + 4) run them in anti-phase, X at raised priority.
        u32x4 pfc[3];   // P of half 0 queries 16..31, of half 1 queries 0..15 and 16..31
        auto clean_x = [&](int stage, int slot2, bool dma) {
            __builtin_amdgcn_s_setprio(3);
            u32x4 pf0[2];
            f32x16 st1;
            {
                f32x16 st0;
                mix_scores_both<E, C>(smem, rd, stage, kf, st0, st1);   // S of both query halves as one operand stream
                float lq[16];
                row_lse(stage, 0, lq);
#pragma unroll
                for (int r = 0; r < 16; ++r) st0[r] = fast_exp2(fmaf(st0[r], c2, -lq[r]));
                mix_pack<E>(st0, pf0);
            }
            float lq1[16];
            row_lse(stage, 1, lq1);
            if (dma) issue(slot2, 0x03u);
            // 8 MFMAs of half 0, queries 0..15, with the exponentials of half 1 between them (one lse per register: its query's;
            // every column block, the ones past dout_cols are never stored)
            mix_x_block<E, C, true>(smem, rd, acc, C::NB, stage, pf0[0], st1, c2, [&](int r) { return lq1[r]; });
            if (dma) issue(slot2, kAllPieces & ~0x03u);
            pfc[0] = pf0[1];
            u32x4 pf1[2];
            mix_pack<E>(st1, pf1);
            pfc[1] = pf1[0];
            pfc[2] = pf1[1];
            asm volatile("" : "+v"(pfc[0]), "+v"(pfc[1]), "+v"(pfc[2]));   // the packs belong to X, not behind the barrier
            __builtin_amdgcn_s_setprio(0);
        };
        auto clean_y = [&](int stage, int slot2, bool dma) {
            if (dma) issue(slot2, 0x03u);
            pv_stream(stage, 16, pfc, [&](int i) {
                if (i == 11 && dma) issue(slot2, kAllPieces & ~0x03u);
            });
        };

        // ---- a step in the diagonal region or on the partial last tile: per-half liveness, masking
        auto edge_step = [&](int stage, int qb, int slot2) {
            issue(slot2, 0x01u);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int qsub = qb * 2 + kk;
                const bool live = wave_has_keys && qsub >= my_key_sub && qsub * 32 < S;
                u32x4 pf[2];
                if (live) {
                    f32x16 st = mix_scores<E, C>(smem, rd, stage, kk, kf);
                    float lq[16];
                    row_lse(stage, kk, lq);
#pragma unroll
                    for (int r = 0; r < 16; ++r) st[r] = fast_exp2(fmaf(st[r], c2, -lq[r]));
                    mix_pack<E>(st, pf);
                    // query of register r: qsub*32 + (r&3) + 8*(r>>2) + 4*hh.  It must exist (< S) and must not lie
                    // before my key: AND masks on the packed words (AND also kills an inf from an invisible pair).
                    const int q_lim = S - 1 - qsub * 32 - 4 * hh;                   // largest valid rel index (w/o 4hh)
                    const int k_rel = qsub == my_key_sub ? l31 - 4 * hh : -64;      // smallest visible rel index
                    if (qsub == my_key_sub || qsub * 32 + 31 >= S) {
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const int r0 = ks * 8 + 2 * i;
                                const int rel0 = (r0 & 3) + 8 * (r0 >> 2);   // rel of r0 + 1 is rel0 + 1
                                const uint32_t keep = ((rel0 >= k_rel && rel0 <= q_lim) ? 0x0000ffffu : 0u) |
                                                      ((rel0 + 1 >= k_rel && rel0 + 1 <= q_lim) ? 0xffff0000u : 0u);
                                pf[ks][i] &= keep;
                            }
                    }
                    pv_stream(stage, kk * 32, pf, [](int) {});
                }
                issue(slot2, kk == 0 ? 0x0eu : (kAllPieces & ~0x0fu));
            }
        };

        // ---- pipeline: two tiles in flight (mix_ring.h) ------------------------------------------------------------
        ring.prime([&](int slot) { issue(slot, kAllPieces); });
        uint16_t *dcg = reinterpret_cast<uint16_t *>(p.dc) + batch * p.c_bs + (int64_t)my_key * p.c_rs;
        for (int l = 0; l < p.nsenses; ++l) {
            if (wave_has_keys) take_k(l);
#pragma unroll
            for (int n = 0; n < C::NB; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
            for (int qb = qb_begin; qb < qb_clean; ++qb) {
                ring.step_begin();
                edge_step(ring.stage(), qb, ring.refill_slot());
                ring.step_end();
            }
            // clean steps, two barriers each; waves 4-7 one barrier late (see sense_mix_dma.hip for the ring argument)
            if (qb_clean < qb_full_end) {
                const bool late = wave >= C::NWAVE / 2;
                if (late) ring.step_begin();
                for (int qb = qb_clean; qb < qb_full_end; ++qb) {
                    ring.step_begin();
                    clean_x(ring.stage(), ring.refill_slot(), late);
                    ring.step_begin();
                    clean_y(ring.stage(), ring.refill_slot(), !late);
                    ring.step_end();
                }
                if (!late) __builtin_amdgcn_s_barrier();
            }
            for (int qb = max(qb_clean, qb_full_end); qb < nqb; ++qb) {
                ring.step_begin();
                edge_step(ring.stage(), qb, ring.refill_slot());
                ring.step_end();
            }
            // dC[my key, sense l, chunk columns]
            if (wave_has_keys && my_key < S) mix_store_row<E, C>(dcg + (int64_t)l * p.c_ss, acc, col_base, p.dout_cols, hh);
        }
        wait_vmcnt<0>();
    }

}

// =====================================================================================================================
// dq and dk from the precomputed dP^T slab.
//
// dpt: (B, N, TS) 16-bit, row index s*k + l (key s, sense l), TS = 128 queries of the slab [t0, t0 + TS): the output of
// the BLAS GEMM  C_flat[:, :N, :] @ dout[:, t0:t0+TS, :]^T  with N = (number of keys the slab can see) * k.
// Both kernels recompute P from q, k and the saved lse; one workgroup = one (batch, sense), 4 waves.
//   * sense_dq_kernel: wave = 32 queries of the slab, sweeps 64-key tiles (K_l rows + their dP^T rows through LDS;
//     dP^T is read with ds_read_b64_tr_b16 so that it lands in the register order of S^T = K Q^T).  D is not known
//     until the sweep ends, so the sweep accumulates  A1 = sum_s P dP k_s,  A2 = sum_s P k_s  and  D = sum_s P dP,
//     and the epilogue forms dq = scale (A1 - D A2).  D goes to memory for the dk kernel.
//   * sense_dk_kernel: wave = 32 keys (K_l fragments in registers), sweeps the slab's queries; lane = key, so its row
//     of dP^T is read directly; dS = P (dP - D) feeds dK^T += Q^T dS.  The result is ADDED to an fp32 accumulator:
//     slabs run one after the other on one stream and each (batch, sense, key) is owned by exactly one wave of one
//     launch, so the sum is deterministic.
// =====================================================================================================================
template <int KD>
struct SenseGradCfg {
    static constexpr int NT = 256, NWAVE = 4, TS = 128, BK = 64;
    static constexpr int KROW = KD <= 4 ? 128 : 256;   // K / Q row image pitch (b128 reads)
    static constexpr int KSLOTS = KROW / 16;
    static constexpr int NVK = KD <= 2 ? 1 : KD <= 4 ? 2 : 4;   // 64-byte chunks per row of the transposed-read image
    static constexpr int TROW = NVK * 64;
};

// ---- dq ----------------------------------------------------------------------------------------------------
template <class ET, int KD>
__global__ __launch_bounds__(256) void sense_dq_kernel(const SenseGradParams p) {
    using C = SenseGradCfg<KD>;
    using E = Elem<ET>;
    constexpr int NVK = C::NVK;
    // stage = K row image | K transposed-read image | dP^T tile (64 keys x 128 queries, 256-B rows)
    constexpr int RTILE = C::BK * C::KROW, TTILE = C::BK * C::TROW, PTILE = C::BK * 256;
    constexpr int STAGE = RTILE + TTILE + PTILE;
    constexpr int R_DMA = RTILE / 1024 / C::NWAVE, T_DMA = TTILE / 1024 / C::NWAVE, P_DMA = PTILE / 1024 / C::NWAVE;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
    const uint32_t lds0 = lds_base_addr(smem);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const int batch = blockIdx.x / p.nsenses;
    const int l = blockIdx.x - batch * p.nsenses;
    const int S = p.s;

    const uint16_t *qg = reinterpret_cast<const uint16_t *>(p.q) + batch * p.qk_bs + (int64_t)l * p.qk_ss;
    const uint16_t *kg = reinterpret_cast<const uint16_t *>(p.k) + batch * p.qk_bs + (int64_t)l * p.qk_ss;
    const uint16_t *pg = reinterpret_cast<const uint16_t *>(p.dpt) + batch * p.dpt_bs;   // row (s*k + l), 128 queries

    const int q0 = p.t0 + wave * 32;
    const int my_q = q0 + l31;
    const bool wave_has_rows = q0 < S;
    const float c2 = p.scale * kLog2e;
    const int k_end = min(S, p.t0 + C::TS);
    const int nkb = (k_end + C::BK - 1) / C::BK;

    if (p.dk * 2 != C::KROW || p.dk * 2 != C::TROW) {   // pad slots of the images must read as 0
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (int off = tid * 16; off < 2 * STAGE; off += C::NT * 16) lds_write_16B(smem, off, z);
        __syncthreads();
    }

    u32x4 qf[KD];
    float lse2 = 0.f;
    {
        const int q = min(my_q, S - 1);
#pragma unroll
        for (int s = 0; s < KD; ++s) {
            const int col = 16 * s + 8 * hh;
            u32x4 a = {0u, 0u, 0u, 0u};
            if (col < p.dk) a = ld_global_16B(qg + (int64_t)q * p.qk_rs + col);
            qf[s] = a;
        }
        lse2 = p.lse[((int64_t)batch * p.nsenses + l) * p.lse_stride + q] * kLog2e;
#pragma unroll
        for (int s = 0; s < KD; ++s) settle(qf[s]);
        settle(lse2);
    }

    // DMA descriptors: K row image, K transposed-read image, dP^T rows (RowImage / TrImage::src and tr_lane of lds_image.h,
    // spelled here in dq and dk: through the header both kernels' code differed)
    int rr[R_DMA], rc[R_DMA], tr[T_DMA], tc[T_DMA], pr[P_DMA], pc[P_DMA];
#pragma unroll
    for (int j = 0; j < R_DMA; ++j) {
        rr[j] = (wave * R_DMA + j) * (1024 / C::KROW) + lane / C::KSLOTS;
        rc[j] = ((lane % C::KSLOTS) ^ k_swz<C::KROW>(rr[j])) * 8;
    }
#pragma unroll
    for (int j = 0; j < T_DMA; ++j) {
        const int c = (wave * T_DMA + j) * 64 + lane;
        tr[j] = c / (NVK * 4);
        const int stored = c - tr[j] * (NVK * 4);
        int c64 = stored >> 2;
        if (NVK == 2) c64 ^= (tr[j] >> 1) & 1;
        if (NVK == 4) c64 ^= tr[j] & 3;
        tc[j] = ((c64 << 2) | (stored & 3)) * 8;
    }
#pragma unroll
    for (int j = 0; j < P_DMA; ++j) {
        const int c = (wave * P_DMA + j) * 64 + lane;   // 16 chunks of 16 B per 256-B row
        pr[j] = c >> 4;
        const int stored = c & 15;
        const int c64 = (stored >> 2) ^ (pr[j] & 3);
        pc[j] = ((c64 << 2) | (stored & 3)) * 8;
    }
    auto issue = [&](int kb) {
        const uint32_t st = __builtin_amdgcn_readfirstlane(lds0 + (kb & 1) * STAGE);
#pragma unroll
        for (int j = 0; j < R_DMA; ++j) {
            const int64_t row = min(kb * C::BK + rr[j], S - 1);
            if (rc[j] < p.dk) dma16_d(kg + row * p.qk_rs + rc[j], st + (wave * R_DMA + j) * 1024);
        }
#pragma unroll
        for (int j = 0; j < T_DMA; ++j) {
            const int64_t row = min(kb * C::BK + tr[j], S - 1);
            if (tc[j] < p.dk) dma16_d(kg + row * p.qk_rs + tc[j], st + RTILE + (wave * T_DMA + j) * 1024);
        }
#pragma unroll
        for (int j = 0; j < P_DMA; ++j) {
            const int64_t key = min(kb * C::BK + pr[j], k_end - 1);
            dma16_d(pg + (key * p.nsenses + l) * (int64_t)C::TS + pc[j], st + RTILE + TTILE + (wave * P_DMA + j) * 1024);
        }
    };

    // accumulators: A1 = sum_s (P dP) k_s and A2 = sum_s P k_s as (d_k x my queries), D = sum_s P dP
    f32x16 a1[NVK], a2[NVK];
#pragma unroll
    for (int n = 0; n < NVK; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) { a1[n][r] = 0.f; a2[n][r] = 0.f; }
    float dsum = 0.f;

    int r_read_off[KD];
#pragma unroll
    for (int s = 0; s < KD; ++s) r_read_off[s] = RowImage<C::KROW>::read_off(l31, hh, s);
    const int t_row_lane = 4 * hh + ((lane & 15) >> 2);
    const int t_ch_lane = ((lane >> 4) & 1) * 2 + ((lane & 3) >> 1);
    int t_read_off[NVK];
#pragma unroll
    for (int n = 0; n < NVK; ++n) t_read_off[n] = v_lds_off<NVK>(t_row_lane, n * 4 + t_ch_lane) + (lane & 1) * 8;
    // dP^T tile: 256-B rows = 4 chunks of 64 B (one per wave's 32 queries), chunk index swizzled with row & 3
    const int p_read_off = v_lds_off<4>(t_row_lane, wave * 4 + t_ch_lane) + (lane & 1) * 8;

    // Row reference r[t] ~ D[t], estimated from the first 32 keys as sum P dP / sum P (key 0 is visible to every query,
    // so the denominator is positive): the softmax backward is invariant under dP -> dP - r[t], and a component of
    // dout . C that is common to all keys of a row -- the bias of the sense network's last layer is one -- would
    // otherwise survive into the 16-bit products P dP and cancel only in A1 - D A2
    // (tests: ..._with_a_common_offset_in_dout_c).  With g = P (dP - r):
    //     D = sum g + r sum P,      dq = scale (sum g k - (sum g + r (sum P - 1)) sum P k).
    float rref = 0.f, psum = 0.f;
    // one 32-key sub-block; REF: only sum P dP and sum P over it (into dsum / psum), no products
    auto sub_block = [&](const char *k_r, const char *k_t, const char *dp_t, int kb, int kk, auto REF) {
        constexpr bool kRef = decltype(REF)::value;
        const int kbase = kb * C::BK + kk * 32;
        f32x16 st_;
#pragma unroll
        for (int r = 0; r < 16; ++r) st_[r] = 0.f;
#pragma unroll
        for (int s = 0; s < KD; ++s) {
            const u32x4 a = lds_read_16B(k_r, r_read_off[s] + kk * 32 * C::KROW);
            st_ = E::mfma(a, qf[s], st_);
        }
        u32x4 pf[2], gf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            // dP^T of keys {0..3, 8..11} + 4 hh + 16 ks for my query: same order as the S^T registers
            const int rows = (kk * 32 + ks * 16) * 256;
            const u32x2 lo = lds_read_tr16_8B(dp_t, p_read_off + rows);
            const u32x2 hi = lds_read_tr16_8B(dp_t, p_read_off + rows + 8 * 256);
            const uint32_t dw[4] = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = ks * 8 + 2 * i;
                const int key = kbase + (r & 3) + 8 * (r >> 2) + 4 * hh;
                float p0 = fast_exp2(fmaf(st_[r], c2, -lse2));
                float p1 = fast_exp2(fmaf(st_[r + 1], c2, -lse2));
                if (key > my_q || key >= S) p0 = 0.f;
                if (key + 1 > my_q || key + 1 >= S) p1 = 0.f;
                const uint32_t d = dw[i];   // by-value copy (bp_common.h)
                const float g0 = p0 * (E::lo_f32(d) - rref), g1 = p1 * (E::hi_f32(d) - rref);
                dsum += g0 + g1;
                psum += p0 + p1;
                pf[ks][i] = E::pack2(p0, p1);
                gf[ks][i] = E::pack2(g0, g1);
            }
        }
        if (kRef) return;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int rows = (kk * 32 + ks * 16) * C::TROW;
#pragma unroll
            for (int n = 0; n < NVK; ++n) {
                const u32x2 lo = lds_read_tr16_8B(k_t, t_read_off[n] + rows);
                const u32x2 hi = lds_read_tr16_8B(k_t, t_read_off[n] + rows + 8 * C::TROW);
                const u32x4 a = {lo[0], lo[1], hi[0], hi[1]};
                a1[n] = E::mfma(a, gf[ks], a1[n]);
                a2[n] = E::mfma(a, pf[ks], a2[n]);
            }
        }
    };
    if (nkb > 0) issue(0);
    for (int kb = 0; kb < nkb; ++kb) {
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (kb + 1 < nkb) issue(kb + 1);
        if (!wave_has_rows || kb * C::BK > q0 + 31) continue;
        const char *st = smem + (kb & 1) * STAGE;
        const char *k_r = st, *k_t = st + RTILE, *dp_t = st + RTILE + TTILE;
        if (kb == 0) {
            sub_block(k_r, k_t, dp_t, 0, 0, std::true_type{});
            const float num = xhalf_sum(dsum), den = xhalf_sum(psum);
            rref = den > 0.f ? num / den : 0.f;
            // the slab holds 16-bit values: a reference of the same precision keeps dP - r exact for dP near r
            rref = E::lo_f32(E::pack2(rref, 0.f));
            dsum = 0.f;
            psum = 0.f;
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int kbase = kb * C::BK + kk * 32;
            if (kbase >= S || kbase > q0 + 31) continue;
            sub_block(k_r, k_t, dp_t, kb, kk, std::false_type{});
        }
    }

    if (!wave_has_rows) return;
    const float g_tot = xhalf_sum(dsum), p_tot = xhalf_sum(psum);
    const float d_tot = fmaf(rref, p_tot - 1.f, g_tot);    // D - r: what multiplies sum P k
    if (my_q < S) {
        if (hh == 0) p.dsum[((int64_t)batch * p.nsenses + l) * p.lse_stride + my_q] = fmaf(rref, p_tot, g_tot);   // D itself
        uint16_t *dqg = reinterpret_cast<uint16_t *>(p.dq) + batch * p.dq_bs + (int64_t)my_q * p.dq_rs + (int64_t)l * p.dq_ss;
#pragma unroll
        for (int n = 0; n < NVK; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d0 = n * 32 + 8 * g + 4 * hh;
                if (d0 < p.dk) {
                    float v[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = p.scale * (a1[n][4 * g + i] - d_tot * a2[n][4 * g + i]);
                    u32x2 w = {E::pack2(v[0], v[1]), E::pack2(v[2], v[3])};
                    *reinterpret_cast<u32x2 *>(dqg + d0) = w;
                }
            }
    }
}

// ---- dk ----------------------------------------------------------------------------------------------------
template <class ET, int KD>
__global__ __launch_bounds__(256) void sense_dk_kernel(const SenseGradParams p) {
    using C = SenseGradCfg<KD>;
    using E = Elem<ET>;
    constexpr int NVK = C::NVK;
    // the slab's 128 queries of this (batch, sense): Q row image | Q transposed-read image | lse, D
    constexpr int RTILE = C::TS * C::KROW, TTILE = C::TS * C::TROW, STATS = 2 * C::TS * 4;
    constexpr int R_DMA = RTILE / 1024 / C::NWAVE, T_DMA = TTILE / 1024 / C::NWAVE;
    __shared__ __attribute__((aligned(16))) char smem[RTILE + TTILE + STATS];
    const uint32_t lds0 = lds_base_addr(smem);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const int per_bl = (min(p.s, p.t0 + C::TS) + 127) / 128;           // 128-key tiles this slab can see
    const int bl = blockIdx.x / per_bl, ktile = blockIdx.x - bl * per_bl;
    const int batch = bl / p.nsenses;
    const int l = bl - batch * p.nsenses;
    const int S = p.s;

    const uint16_t *qg = reinterpret_cast<const uint16_t *>(p.q) + batch * p.qk_bs + (int64_t)l * p.qk_ss;
    const uint16_t *kg = reinterpret_cast<const uint16_t *>(p.k) + batch * p.qk_bs + (int64_t)l * p.qk_ss;
    const uint16_t *pg = reinterpret_cast<const uint16_t *>(p.dpt) + batch * p.dpt_bs;
    const float *lse_g = p.lse + ((int64_t)batch * p.nsenses + l) * p.lse_stride;
    const float *dsum_g = p.dsum + ((int64_t)batch * p.nsenses + l) * p.lse_stride;

    const int key0 = ktile * 128 + wave * 32;
    const int my_key = key0 + l31;
    const int k_end = min(S, p.t0 + C::TS);
    const bool wave_has_keys = key0 < k_end;
    const float c2 = p.scale * kLog2e;
    const int nq = min(C::TS, S - p.t0);   // queries that exist in the slab

    {   // pad slots of the images must read as 0 (also rows past the sequence)
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (int off = tid * 16; off < RTILE + TTILE + STATS; off += C::NT * 16) lds_write_16B(smem, off, z);
        __syncthreads();
    }
    // ---- the slab's Q rows (two images) and per-query statistics: one DMA round ---------------------------------
#pragma unroll
    for (int j = 0; j < R_DMA; ++j) {
        const int row = (wave * R_DMA + j) * (1024 / C::KROW) + lane / C::KSLOTS;
        const int col = ((lane % C::KSLOTS) ^ k_swz<C::KROW>(row)) * 8;
        const int64_t q = min(p.t0 + row, S - 1);
        if (col < p.dk) dma16_d(qg + q * p.qk_rs + col, lds0 + (wave * R_DMA + j) * 1024);
    }
#pragma unroll
    for (int j = 0; j < T_DMA; ++j) {
        const int c = (wave * T_DMA + j) * 64 + lane;
        const int row = c / (NVK * 4), stored = c - row * (NVK * 4);
        int c64 = stored >> 2;
        if (NVK == 2) c64 ^= (row >> 1) & 1;
        if (NVK == 4) c64 ^= row & 3;
        const int col = ((c64 << 2) | (stored & 3)) * 8;
        const int64_t q = min(p.t0 + row, S - 1);
        if (col < p.dk) dma16_d(qg + q * p.qk_rs + col, lds0 + RTILE + (wave * T_DMA + j) * 1024);
    }
    if (wave < 2) {   // wave 0: lse of the 128 queries (two 64-float pieces), wave 1: D
        const float *src = wave == 0 ? lse_g : dsum_g;
        dma4(src + min(p.t0 + lane, S - 1), lds0 + RTILE + TTILE + wave * 512);
        dma4(src + min(p.t0 + 64 + lane, S - 1), lds0 + RTILE + TTILE + wave * 512 + 256);
    }

    u32x4 kf[KD];
    {
        const int key = min(my_key, S - 1);
#pragma unroll
        for (int s = 0; s < KD; ++s) {
            const int col = 16 * s + 8 * hh;
            u32x4 a = {0u, 0u, 0u, 0u};
            if (col < p.dk) a = ld_global_16B(kg + (int64_t)key * p.qk_rs + col);
            kf[s] = a;
        }
    }
    // my row of dP^T: 128 queries = 256 bytes, in the register order of S (runs of 4 queries)
    u32x2 dprow[4][4];   // [32-query block][g]
    {
        const uint16_t *row = pg + ((int64_t)min(my_key, k_end - 1) * p.nsenses + l) * (int64_t)C::TS;
#pragma unroll
        for (int qb = 0; qb < 4; ++qb)
#pragma unroll
            for (int g = 0; g < 4; ++g) dprow[qb][g] = *reinterpret_cast<const u32x2 *>(row + qb * 32 + 8 * g + 4 * hh);
    }
    wait_vmcnt<0>();
    __syncthreads();
    if (!wave_has_keys) return;

    int r_read_off[KD];
#pragma unroll
    for (int s = 0; s < KD; ++s) r_read_off[s] = RowImage<C::KROW>::read_off(l31, hh, s);
    const int t_row_lane = 4 * hh + ((lane & 15) >> 2);
    const int t_ch_lane = ((lane >> 4) & 1) * 2 + ((lane & 3) >> 1);
    int t_read_off[NVK];
#pragma unroll
    for (int n = 0; n < NVK; ++n) t_read_off[n] = v_lds_off<NVK>(t_row_lane, n * 4 + t_ch_lane) + (lane & 1) * 8;
    const char *q_r = smem, *q_t = smem + RTILE, *stats = smem + RTILE + TTILE;

    f32x16 dk[NVK];
#pragma unroll
    for (int n = 0; n < NVK; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[n][r] = 0.f;

#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
        const int qbase = p.t0 + qb * 32;
        if (qb * 32 >= nq || qbase + 31 < key0) continue;   // no such queries, or all of them before my first key
        f32x16 s_;
#pragma unroll
        for (int r = 0; r < 16; ++r) s_[r] = 0.f;
#pragma unroll
        for (int s = 0; s < KD; ++s) {
            const u32x4 a = lds_read_16B(q_r, r_read_off[s] + qb * 32 * C::KROW);
            s_ = E::mfma(a, kf[s], s_);
        }
        u32x4 dsf[2];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const u32x4 l4 = lds_read_16B(stats, (qb * 32 + 8 * g + 4 * hh) * 4);
            const u32x4 d4 = lds_read_16B(stats, 512 + (qb * 32 + 8 * g + 4 * hh) * 4);
            const u32x2 dp2 = dprow[qb][g];
            const uint32_t dpw[2] = {dp2[0], dp2[1]};
            float de[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 4 * g + i;
                const int q = qbase + 8 * g + 4 * hh + i;
                const uint32_t lw = l4[i], dw = d4[i], pw = dpw[i >> 1];   // by-value copies (bp_common.h)
                const float pv = fast_exp2(fmaf(s_[r], c2, -as_f32(lw) * kLog2e));
                const float dp = (i & 1) ? E::hi_f32(pw) : E::lo_f32(pw);
                const bool dead = q >= S || my_key >= S || my_key > q;
                de[i] = dead ? 0.f : pv * (dp - as_f32(dw));
            }
            dsf[g >> 1][(g & 1) * 2 + 0] = E::pack2(de[0], de[1]);
            dsf[g >> 1][(g & 1) * 2 + 1] = E::pack2(de[2], de[3]);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int rows = (qb * 32 + ks * 16) * C::TROW;
#pragma unroll
            for (int n = 0; n < NVK; ++n) {
                dk[n] = E::mfma(tr_operand(q_t, t_read_off[n] + rows, C::TROW), dsf[ks], dk[n]);
            }
        }
    }

    if (my_key >= S) return;
    float *acc = p.dk_acc + batch * p.dka_bs + (int64_t)my_key * p.dka_rs + (int64_t)l * p.dka_ss;
#pragma unroll
    for (int n = 0; n < NVK; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d0 = n * 32 + 8 * g + 4 * hh;
            if (d0 < p.dk) {
                float *dst = acc + d0;
                const f32x4 old = *reinterpret_cast<const f32x4 *>(dst);
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = old[i] + p.scale * dk[n][4 * g + i];
                *reinterpret_cast<f32x4 *>(dst) = v;
            }
        }
}

// ---- launchers -------------------------------------------------------------------------------------------------
hipError_t launch_sense_mix_dc(const MixBwdParams &params, int dtype, hipStream_t stream) {
    return launch_mix_persistent(params, params.n_ktiles, params.dout_cols, dtype, stream,
                                 [&](auto et, auto kd, auto full, dim3 g, dim3 t, const MixBwdParams &p) {
        hipLaunchKernelGGL((sense_mix_dc_kernel<decltype(et), kd, full>), g, t, 0, stream, p);
    });
}

hipError_t launch_sense_dq_dk(const SenseGradParams &p, int dtype, hipStream_t stream) {
    const int per_bl = ((p.s < p.t0 + 128 ? p.s : p.t0 + 128) + 127) / 128;
    return with_dtype(dtype, [&](auto et) {
        return with_kd(p.dk, [&](auto kd) {
            using ET = decltype(et);
            hipLaunchKernelGGL((sense_dq_kernel<ET, kd>), dim3(p.b * p.nsenses), dim3(256), 0, stream, p);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL((sense_dk_kernel<ET, kd>), dim3(p.b * p.nsenses * per_bl), dim3(256), 0, stream, p);
            return hipGetLastError();
        });
    });
}

}  // namespace bp
