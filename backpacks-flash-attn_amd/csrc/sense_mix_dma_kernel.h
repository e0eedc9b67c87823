// Fused Backpack sense combination, LDS-DMA ring version (the fast path for 16-byte-aligned shapes).
//
//     out[b,t,:] = sum_l sum_{s<=t} exp(scale * q_l[t].k_l[s] - lse[b,l,t]) * C[b,s,l,:]
//
// Same contraction and tile algebra as sense_mix.hip (see there and bp_common.h).  One workgroup = 8 waves
// = 256 queries x 256 output columns of one sample; sense outer, 64-key tile inner; a pipeline step = one
// (sense, key tile): S^T (KD MFMAs per 32 keys) -> P^T = exp2(S^T c - lse) -> O^T += C^T P^T (16 MFMAs per
// 32 keys), probabilities final on first touch thanks to the LSE pre-pass.
//   * tiles are 64 keys (40 KB: 32 KB of C + 8 KB of K) in a 3-slot LDS ring (120 KB, one workgroup per CU),
//     filled by `global_load_lds_dwordx4` (no VGPR round trip, no ds_write pass), two tiles always in flight,
//     COUNTED waits + ONE raw s_barrier per tile (bp_dma.h); the XOR swizzles that make ds_read_b128 (K) and
//     ds_read_b64_tr_b16 (C) conflict-free are applied to the per-lane SOURCE address.  Every lane of every
//     DMA piece moves VALID data (pad slots receive a duplicate of column 0): K pad columns meet zero Q columns,
//     C pad columns feed output columns that are never stored, so nothing is predicated and nothing is zeroed.
//   * the two waves of a SIMD (w and w + 4) leave a tile barrier together, so in a one-phase step both sit in their
//     softmax (VALU, matrix pipe idle) and then both in their MFMAs (VALU idle): the per-phase clock account of round 3
//     (scripts/probes/mix_timeline) found the sum of the phases' lower bounds equal to the measured step, 4085 clocks
//     against 2432 of matrix-pipe time.  A clean step is therefore two halves under two barriers -- X: S^T, softmax of
//     key half 0, 8 MFMAs with the exponentials of half 1 between them; Y: the other 24 MFMAs -- and waves 4-7 run the
//     clean loop one barrier late, so X of one wave always meets Y of its partner.  Every MFMA operand that comes from LDS
//     is requested two MFMAs ahead (mfma_stream, bp_common.h).  Steps that touch the diagonal (some waves dead or
//     masking) keep the simple per-half form.
//   * PERSISTENT launch: one workgroup per CU pulls (group, query tile) jobs from 8 per-XCD queues, heaviest
//     query tiles first, stealing from the other queues when its own is empty.  The hardware dispatcher places
//     workgroups in order and round-robin: with one workgroup per CU and jobs of 4,3,2,1 units that gave rounds of
//     4+3+2 = 9 units per CU against 7.5 ideal (dispatch_order probe); a static snake assignment lost
//     to run-time variance (r01).  A group's tiles still prefer one XCD, i.e. one L2 holds its C tiles.
//     Queue state: a 64-byte record of device memory, the caller's (`queue_ws`) or one of a small ring owned by the
//     library, zeroed by a one-wave kernel in front of every launch, see arm_mix_queues.
// Rows past the sequence are fetched from a clamped (valid) row: their probabilities are exactly 0 by the
// causal mask and 0 * finite = 0.
//
// The template lives in this header because two code objects instantiate it: sense_mix_dma.hip (fixed length: plain,
// weighted, gathering) and sense_mix_varlen.hip (packed batches: Varlen<ET> below, plain and gathering).
#pragma once
#include "bp_common.h"
#include "bp_dma.h"
#include "bp_kernels.h"
#include "mix_ring.h"

namespace bp {

// Packed (variable-length) form, bp_sense_mix_varlen / bp_sense_mix_gather_varlen: sense_mix_dma_kernel<Varlen<ET>, ...>
// reads every job's sequence from MixParams::cu (the slot of the key weights, which the packed form does not have).  The
// flag rides on the element tag (as Weighted<ET> in decode_core.h, Controlled<ET> in pick_core.h), so the fixed-length
// instantiations keep their names, their argument block and their text.  Forms that were tried and changed that text:
// the body as a device function behind two __global__ functions (by reference and by value: other scalar spills), a
// parameter type that depends on the tag (other mangled names), a new field at the end of MixParams (the arguments
// that the wide LSE kernels take behind it move).
//   * jobs are still (sample, column chunk) x n_qtiles with n_qtiles = ceil(max_seqlen / 256), heaviest rank first;
//   * a job's S = cu[b + 1] - cu[b]; q, k, content and out start at row cu[b] (row strides; the batch strides are not
//     read), row_index at cu[b], lse at b * nsenses * lse_stride;
//   * a job whose tile starts at or beyond S takes the next ticket at once (short and zero-length samples);
//   * behind that point the job is the fixed-length job at seqlen = S: the same key tiles in the same order, so a sample's
//     rows carry the bits of the fixed-length launch on that sample alone.  Rows behind the sample's end belong to the
//     NEXT sample of the packed tensor: nothing is stored at my_q >= S, and every clamped read (my_q_clamped, the partial
//     tile of MixStream, the index table of the gathering form) stays inside rows [cu[b], cu[b + 1]).
template <class ET> struct Varlen {};
template <class ET> struct MixTag {
    using elem = ET;
    static constexpr bool varlen = false;
    BP_DEV static int cu(const MixParams &, int) { return 0; }
};
template <class T> struct MixTag<Varlen<T>> {
    using elem = T;
    static constexpr bool varlen = true;
    BP_DEV static int cu(const MixParams &p, int i) { return p.cu[i]; }
};

// Development builds only (-DBP_MIX_PROFILE, scripts/probes/mix_timeline): every wave adds up the s_memtime ticks its
// clean steps spend in each phase; never in the shipped library.  The counters (g_mix_prof) belong to the fixed-length code
// object: sense_mix_dma.hip defines them in front of this header, sense_mix_varlen.hip switches the profile off.
#ifdef BP_MIX_PROFILE
#define MIX_TICK(var) const unsigned long long var = __builtin_readcyclecounter()
#define MIX_ADD(k, expr) prof[k] += (expr)
#else
#define MIX_TICK(var) do { } while (0)
#define MIX_ADD(k, expr) do { } while (0)
#endif

// The ring (mix_ring.h: A = K rows, B = content rows, aux = key weights when WEIGHTED) and, behind it, the forward's own areas
template <int KD, bool WEIGHTED = false>
struct MixDmaCfg : MixRingCfg<KD, WEIGHTED> {
    using R = MixRingCfg<KD, WEIGHTED>;
    // Next sense's query operands, staged through LDS by DMA (see request_q): per wave KD fragments of 64 lanes x 16 B and
    // 64 x 4 B of log-sum-exp.  Only where the ring leaves room (128-byte K rows) and the flat two-phase loop runs.
    static constexpr bool ASYNC_Q = !WEIGHTED && KD <= 3;   // (d_k = 64 spills with the staging reads; wider ones have no LDS left)
    static constexpr int QSTAGE_OFF = R::SMEM;
    static constexpr int QSTAGE_WAVE = KD * 1024 + 256;
    static constexpr int QSTAGE_BYTES = ASYNC_Q ? R::NWAVE * QSTAGE_WAVE : 0;
    // GATHER (bp_sense_mix_gather): the content rows are rows of a TABLE (one per token id), picked by an index per key.
    // The job's row indices live behind the staging area as u16: 8 KB = 4096 keys (= kMixGatherMaxKeys, bp_kernels.h), tables
    // of up to 65 536 rows (= kMixGatherMaxRows: any GPT-2 vocabulary); the byte offset row * row bytes is formed per piece.
    // (A u16 / u32 switch per launch costs the d_k = 48 instantiation five spilled registers: larger tables are gathered by
    // the caller, bp_hip.sense_mix_gather_supported.)
    static constexpr int GATHER_OFF = R::SMEM + QSTAGE_BYTES;
    static constexpr int GATHER_BYTES = 8192;
    static constexpr int LDS_BYTES = R::SMEM + QSTAGE_BYTES;
    static_assert(LDS_BYTES + GATHER_BYTES <= 160 * 1024, "LDS budget");
};

// TAG: BF16 / F16, or Varlen<BF16> / Varlen<F16> for the packed form
template <class TAG, int KD, bool FULL, bool WEIGHTED, bool GATHER = false>
__global__ __launch_bounds__(512) void sense_mix_dma_kernel(const MixParams p) {
    using C = MixDmaCfg<KD, WEIGHTED>;
    using T = MixTag<TAG>;
    using E = Elem<typename T::elem>;
    constexpr bool VARLEN = T::varlen;
    static_assert(!(VARLEN && WEIGHTED), "no weighted packed form");
    __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES + (GATHER ? C::GATHER_BYTES : 0)];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const int S_launch = p.s;   // the sequence length of every job; VARLEN: max_seqlen, each job reads its own below
    const float c2 = p.scale_log2e;
    const uint32_t lds0 = lds_base_addr(smem);

    const MixTileReader<C> rd(lane);
    uint32_t exhausted = 0;   // job queues with no jobs left (mix_take_job)

#ifdef BP_MIX_PROFILE
    unsigned long long prof[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    for (int word; (word = mix_take_job<C>(smem, p.queues, exhausted, p.b, p.n_chunks, p.n_qtiles)) >= 0;) {
        const MixJob job = mix_decode_job<C>(word, p.n_chunks);
        const int batch = job.batch, col_base = job.col_base;
        const int qt = p.n_qtiles - 1 - job.rank;   // heaviest query tiles (the last ones) first
        // VARLEN: the sample's rows are [first_row, first_row + S) of the packed operands; a tile at or beyond S has no rows (a short
        // or an empty sample: n_qtiles counts the tiles of max_seqlen) and the workgroup takes the next ticket
        const int64_t first_row = VARLEN ? T::cu(p, batch) : 0;
        const int S = VARLEN ? T::cu(p, batch + 1) - (int)first_row : S_launch;
        if (VARLEN && qt * C::BM >= S) continue;
        MIX_TICK(job_t0);

        const uint16_t *qg = reinterpret_cast<const uint16_t *>(p.q) + (VARLEN ? first_row * p.qk_rs : batch * p.qk_bs);
        const uint16_t *kg = reinterpret_cast<const uint16_t *>(p.k) + (VARLEN ? first_row * p.qk_rs : batch * p.qk_bs);
        const uint16_t *cg = reinterpret_cast<const uint16_t *>(p.c) + (GATHER ? 0 : VARLEN ? first_row * p.c_rs : batch * p.c_bs);

        const int k_end = min(S, qt * C::BM + C::BM);
        const int nkb = (k_end + C::BK - 1) / C::BK;
        // key tiles below this index are full and entirely visible to every row of the workgroup
        const int nkb_clean = WEIGHTED ? 0 : min((qt * C::BM) / C::BK, S / C::BK);

        const int q0 = qt * C::BM + wave * 32;
        const int my_q = q0 + l31;
        const int my_q_clamped = min(my_q, S - 1);
        const bool wave_has_rows = q0 < S;
        const int my_diag_sub = q0 >> 5;   // index of the 32-key sub-block that holds my diagonal
        const int nb_live = FULL ? C::NB : min(C::NB, (p.dout - col_base + 31) / 32);

        // the DMA side of the job (mix_ring.h): key tiles [0, nkb) of every sense
        MixStream<C> ring;
        ring.begin_job(lds0, wave, lane, S, p.nsenses, 0, k_end, kg, p.qk_rs, p.qk_ss, p.dk, cg, p.c_rs, p.c_ss);
        uint32_t c_voff[C::B_DMA];
        ring.template b_offsets<FULL>(c_voff, GATHER ? 0 : p.c_rs, col_base, p.dout);   // (GATHER: the row part comes from the table)
        if (GATHER) {
            // table row of every key of the job, clamped past the sequence end (those keys are masked) and to the table
            // (an index outside it reads its last row, never memory outside it); every wave is done with the previous
            // job's table (the __syncthreads in front of the job word)
            const int32_t *idx = p.row_index + (VARLEN ? first_row : (int64_t)batch * p.idx_bs);
            for (int i = tid; i < nkb * C::BK; i += C::NT) {
                const uint32_t row = min((uint32_t)idx[min(i, S - 1)], p.last_table_row);
                *reinterpret_cast<uint16_t *>(smem + C::GATHER_OFF + i * 2) = (uint16_t)row;
            }
            __syncthreads();
        }

        // GATHER: B piece j of tile ring.t2 = two table rows, their indices read from the job's LDS table; the base is the
        // SENSE's (table + l2 * c_ss), and table rows are re-read by other jobs, so the loads stay cacheable
        const uint32_t gather_row_bytes = (uint32_t)p.c_rs * 2u;
        auto gather_piece = [&](int j, uint32_t lds_dst) {
            const int key = ring.t2 * C::BK + ring.b_piece_row(j);
            const uint32_t row = *reinterpret_cast<const uint16_t *>(smem + C::GATHER_OFF + key * 2);
            dma16_s(ring.bs2, row * gather_row_bytes + c_voff[j], lds_dst);
        };
        auto issue = [&](int slot, uint32_t pieces) {
            ring.issue(
                slot, pieces,
                [&](int j, int back, uint32_t lds_dst) {
                    if (GATHER) gather_piece(j, lds_dst);
                    // the content stream is read once per job: non-temporal (-1.6 % at B=64, r02_p)
                    else dma16_s_nt(ring.bt2, c_voff[j] - (uint32_t)(back * p.c_rs) * 2u, lds_dst);
                },
                [&](int l) { return p.kw + batch * p.kw_bs + (int64_t)l * p.kw_ss; });   // key weights w[b, l, :]
        };
        constexpr uint32_t kAllPieces = C::ALL_PIECES;

        f32x16 acc[C::NB];
#pragma unroll
        for (int n = 0; n < C::NB; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;

        u32x4 qf[KD];
#pragma unroll
        for (int s = 0; s < KD; ++s) qf[s] = u32x4{0u, 0u, 0u, 0u};
        float lse2 = 0.f;
        // per-sense operands of this wave: my query's fragments (B operand of S^T = K Q^T) and its LSE
        auto take_q = [&](int l) {
            const uint16_t *row = qg + (int64_t)my_q_clamped * p.qk_rs + (int64_t)l * p.qk_ss;
#pragma unroll
            for (int s = 0; s < KD; ++s) {
                const int col = 16 * s + 8 * hh;
                u32x4 v = {0u, 0u, 0u, 0u};
                if (col < p.dk) v = ld_global_16B(row + col);
                qf[s] = v;
            }
            lse2 = p.lse[((int64_t)batch * p.nsenses + l) * p.lse_stride + my_q_clamped] * kLog2e;
        };

        // The same for the NEXT sense, requested in the middle of a sense's last ring step (between its X and Y parts) and
        // adopted behind it -- THROUGH LDS: every lane's fragments and its log-sum-exp are DMA'd into the wave's own staging
        // area and read back after the ring's counted wait.  The DMAs are older than the pieces of tile + 2, which that step
        // issues in its Y part, so `vmcnt(DMA_PER_STAGE)` covers them and no compiler-placed vmcnt(0) stalls the wave
        // once per sense (a quarter of the steps of a light query tile).
        // Rounds 3-4 used asynchronous loads into REGISTERS here.  That is only sound while the compiler never copies the
        // destination registers before the data has landed, which it is free to do: with the request on two paths (live
        // / dead wave) hipcc loaded into temporaries and placed the phi copies `v_mov home, temporary` at the join, in
        // front of the wait -- garbage query fragments, NaN outputs (round-5 listing).  LDS has no such hazard, and the
        // staged operands cost no registers while they travel.
        const int qstage = C::QSTAGE_OFF + wave * C::QSTAGE_WAVE;
        auto request_q = [&](int l) {
            const uint16_t *row = qg + (int64_t)my_q_clamped * p.qk_rs + (int64_t)l * p.qk_ss;
#pragma unroll
            for (int s = 0; s < KD; ++s)
                dma16(row + min(16 * s + 8 * hh, p.dk - 8), __builtin_amdgcn_readfirstlane(lds0 + qstage + s * 1024));
            dma4(p.lse + ((int64_t)batch * p.nsenses + l) * p.lse_stride + my_q_clamped, lds0 + qstage + KD * 1024);
        };
        auto adopt_q = [&]() {
            wait_vmcnt<C::DMA_PER_STAGE>();   // everything older than the last step's DMA pieces has landed
#pragma unroll
            for (int s = 0; s < KD; ++s) {
                qf[s] = lds_read_16B(smem, qstage + s * 1024 + lane * 16);
                if (16 * s + 8 * hh >= p.dk) qf[s] = u32x4{0u, 0u, 0u, 0u};
            }
            lse2 = *reinterpret_cast<const float *>(smem + qstage + KD * 1024 + lane * 4) * kLog2e;
        };

        auto exponentiate = [&](f32x16 &st) {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[r] = fast_exp2(fmaf(st[r], c2, -lse2));
        };
        // O^T += C^T P^T over the 16-key steps pk[] from key row `row0` of the tile at `stage` (one operand stream)
        auto pv_stream = [&](int stage, int row0, const auto &pk, auto &&mid) {
            mix_pv_stream<E, C, FULL>(smem, rd, acc, nb_live, stage, row0, pk, mid);
        };

        // Causal mask of one 32-key half on its packed P^T words.  `rel` = the half's sub-block index minus the index of
        // the sub-block that holds this wave's diagonal (wave-uniform): < 0 entirely visible, == 0 the diagonal sub-block
        // (its first key is q0: clear the 16-bit entries whose key lies above my query), > 0 entirely invisible.  AND
        // masks, so an inf from an invisible, larger score dies too.
        auto mask_half = [&](u32x4 (&pf)[2], int rel) {
            if (rel > 0) {
                pf[0] = pf[1] = u32x4{0u, 0u, 0u, 0u};
            } else if (rel == 0) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r0 = ks * 8 + 2 * i;
                        const int rel0 = (r0 & 3) + 8 * (r0 >> 2) + 4 * hh;   // rel of r0 + 1 is rel0 + 1
                        const uint32_t keep = (rel0 <= l31 ? 0x0000ffffu : 0u) | (rel0 + 1 <= l31 ? 0xffff0000u : 0u);
                        pf[ks][i] &= keep;
                    }
            }
        };

        // The step is cut into a vector-heavy half X (S^T of both key halves, softmax of half 0, the first 8 MFMAs of
        // half 0 with the exponentials of half 1 between them, pack) and a matrix-only half Y (the other 24 MFMAs),
        // and the two waves of a SIMD (w and w + 4) run them in ANTI-PHASE: waves 4-7 enter the job's loop one barrier
        // late, so X of one wave always meets Y of the other (see the loop below).  X hands Y three packed operands.
        // Since round 5 EVERY step has this form, the ones that touch the diagonal too (`edge`: the masks above on the
        // packed words; a wave whose rows lie entirely above the tile -- `live` false -- only issues its DMA share and
        // keeps the barrier count).  Before, diagonal steps ran a one-phase per-half form in which both waves of a SIMD sat
        // in their softmax and then both in their MFMAs: 4340 clocks per step against 3260 for a clean one, with 40 % of a
        // job's steps on the diagonal at S = 1024 (profiles/r05_*), and the anti-phase had to be re-established per sense.
        u32x4 pfc[3];   // P^T of half 0 keys 16..31, of half 1 keys 0..15 and 16..31
        auto step_x = [&](int stage, int kb, int slot2, bool dma, bool live, bool edge) {
            if (!live) {
                if (dma) issue(slot2, kAllPieces);
                return;
            }
            // X is one dependent chain (S^T -> softmax -> first MFMAs), Y a stream of independent MFMAs: without a
            // priority the older waves 0-3 win every arbitration, and X of waves 4-7 starves behind their Y (2230
            // clocks against 1360 the other way round, r03_ab timeline)
            __builtin_amdgcn_s_setprio(3);
            f32x16 st0, st1;
            mix_scores_both<E, C>(smem, rd, stage, qf, st0, st1);   // S^T of both key halves as one operand stream
            u32x4 pf0[2];
            exponentiate(st0);
            mix_pack<E>(st0, pf0);
            if (edge) mask_half(pf0, 2 * kb - my_diag_sub);
            if (dma) issue(slot2, 0x03u);
            // 8 MFMAs of half 0, keys 0..15, with the exponentials of half 1 between them (one lse per lane: my query's)
            mix_x_block<E, C, FULL>(smem, rd, acc, nb_live, stage, pf0[0], st1, c2, [&](int) { return lse2; });
            if (dma) issue(slot2, kAllPieces & ~0x03u);
            pfc[0] = pf0[1];
            u32x4 pf1[2];
            mix_pack<E>(st1, pf1);
            if (edge) mask_half(pf1, 2 * kb + 1 - my_diag_sub);
            pfc[1] = pf1[0];
            pfc[2] = pf1[1];
            asm volatile("" : "+v"(pfc[0]), "+v"(pfc[1]), "+v"(pfc[2]));   // the packs belong to X, not behind the barrier
            __builtin_amdgcn_s_setprio(0);
        };
        auto step_y = [&](int stage, int slot2, bool dma, bool live) {
            if (!live) {
                if (dma) issue(slot2, kAllPieces);
                return;
            }
            if (dma) issue(slot2, 0x03u);
            pv_stream(stage, 16, pfc, [&](int i) {
                if (i == 11 && dma) issue(slot2, kAllPieces & ~0x03u);
            });
        };

        // ---- key-weighted launches (the intervention hook): every step in the simple one-phase per-half form
        auto weighted_step = [&](int stage, int l, int kb, int slot2) {
            issue(slot2, 0x01u);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int sub = kb * 2 + kk;
                const bool live = wave_has_rows && sub <= my_diag_sub;
                u32x4 pf[2];
                if (live) {
                    f32x16 st = mix_scores<E, C>(smem, rd, stage, kk, qf);
                    exponentiate(st);
                    if (WEIGHTED) {
                        // alpha[b, l, :, key] *= w[b, l, key]  (register r holds key (r & 3) + 8 (r >> 2) + 4 hh of the
                        // sub-block: four runs of four consecutive keys)
                        const int wbase = stage + C::AUX_OFF + wave * 256 + (kk * 32 + 4 * hh) * 4;
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const u32x4 w4 = lds_read_16B(smem, wbase + g * 32);
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const uint32_t wi = w4[i];   // by-value copy (bp_common.h, as_f32)
                                st[4 * g + i] *= as_f32(wi);
                            }
                        }
                    }
                    mix_pack<E>(st, pf);
                    mask_half(pf, sub - my_diag_sub);
                    pv_stream(stage, kk * 32, pf, [](int) {});
                }
                issue(slot2, kk == 0 ? 0x0eu : (kAllPieces & ~0x0fu));
            }
        };

        // ---- pipeline: two tiles in flight ---------------------------------------------------------------
        // The clean and the edge steps of a sense run in two consecutive loops, each with ONE body: the accumulators
        // then never meet at an if/else join (hipcc answers such a join of 128 registers with copies and spills).
        ring.prime([&](int slot) { issue(slot, kAllPieces); });
        if (wave_has_rows) take_q(0);
        if (WEIGHTED) {
            for (int l = 0; l < p.nsenses; ++l) {
                if (l > 0 && wave_has_rows) take_q(l);
                for (int kb = 0; kb < nkb; ++kb) {
                    ring.step_begin();
                    weighted_step(ring.stage(), l, kb, ring.refill_slot());
                    ring.step_end();
                }
            }
        } else {
            // Per sense: the clean tiles (entirely below the workgroup's queries) in the two-phase form, then the tiles
            // that touch the diagonal in ONE phase per step.
            //   clean: waves 0-3 run  [bar X bar Y]  per tile and one closing barrier; waves 4-7 one opening barrier and
            //   then the same [bar X bar Y]: between any two barriers one wave of a SIMD is in X (VALU + 14 MFMAs) and
            //   the other in Y (24 MFMAs) of the same or the previous tile.  Ring: tile t + 2 goes to the slot of tile
            //   t - 1, last read by Y of waves 4-7 in front of the barrier that ends X(t) of waves 0-3 -- so every wave
            //   issues it right behind that barrier (start of Y for waves 0-3, of X for waves 4-7); every wave waits for
            //   its share of the next tile before each barrier (a no-op on every other one).
            //   diagonal: X and Y of a step back to back under one barrier (`step_x` / `step_y` with the causal masks on
            //   the packed words; a wave whose rows lie above the tile only issues its DMA share).  From the third of a
            //   full query tile's four diagonal steps on every SIMD holds at most ONE live wave, and what bounds the step
            //   is that wave's own dependent chain: S^T of both halves as one stream, the first MFMAs between the second
            //   half's exponentials and one 24-MFMA stream instead of round 4's per-half form (scores, softmax, 16 MFMAs,
            //   twice: ~3190 clocks per diagonal step whoever was live, profiles/r05_c_timeline_*).  Carrying the
            //   anti-phase THROUGH the diagonal steps (two barriers there too) was built first and measured slower:
            //   a lone wave then serialises X, barrier, Y (3216 clocks per diagonal step; r05_c).
            const bool late = wave >= C::NWAVE / 2;
            for (int l = 0; l < p.nsenses; ++l) {
                const int next_sense = (C::ASYNC_Q && wave_has_rows && l + 1 < p.nsenses) ? l + 1 : -1;
                if (!C::ASYNC_Q && l > 0 && wave_has_rows) take_q(l);   // (no LDS left for the staging: plain loads)
                if (nkb_clean > 0) {
                    if (late) ring.step_begin();
                    for (int kb = 0; kb < nkb_clean; ++kb) {
                        const int slot2 = ring.refill_slot();
                        MIX_TICK(t0);
                        ring.step_begin();
                        MIX_TICK(t1);
                        step_x(ring.stage(), kb, slot2, late, true, false);   // (waves without rows run on clamped operands: nothing is stored)
#ifdef BP_MIX_PROFILE
                        asm volatile("" : "+v"(acc[7]), "+v"(pfc[0]), "+v"(pfc[1]), "+v"(pfc[2]));
#endif
                        MIX_TICK(t2);
                        ring.step_begin();
                        MIX_TICK(t3);
                        step_y(ring.stage(), slot2, !late, true);
#ifdef BP_MIX_PROFILE
                        asm volatile("" : "+v"(acc[7]));
#endif
                        MIX_TICK(t4);
                        MIX_ADD(0, t1 - t0); MIX_ADD(1, t2 - t1); MIX_ADD(2, t3 - t2); MIX_ADD(3, t4 - t3); MIX_ADD(6, 1);
                        ring.step_end();
                    }
                    if (!late) __builtin_amdgcn_s_barrier();
                }
                for (int kb = nkb_clean; kb < nkb; ++kb) {   // (never empty: the diagonal tile is one of these)
                    const bool live = wave_has_rows && 2 * kb <= my_diag_sub;
                    const int slot2 = ring.refill_slot();
                    MIX_TICK(e0);
                    ring.step_begin();
                    MIX_TICK(e1);
                    step_x(ring.stage(), kb, slot2, false, live, true);
                    if (kb == nkb - 1 && next_sense >= 0) request_q(next_sense);   // in front of the step's DMA pieces (in Y)
                    step_y(ring.stage(), slot2, true, live);
#ifdef BP_MIX_PROFILE
                    asm volatile("" : "+v"(acc[7]));
#endif
                    MIX_TICK(e2);
                    // profile slots: clean steps 0 wait X, 1 X, 2 wait Y, 3 Y; diagonal steps 4 whole step, 5 X + Y of LIVE waves;
                    // 6 = #clean steps + (#diagonal steps << 32) + (#live diagonal steps << 48); 7 job ticks
                    MIX_ADD(4, e2 - e0);
                    MIX_ADD(5, live ? e2 - e1 : 0);
                    MIX_ADD(6, (1ull << 32) + (live ? (1ull << 48) : 0ull));
#ifdef BP_MIX_PROFILE
                    {   // 8 / 9: X + Y and count of the live steps in which the SIMD's other wave (wave ^ 4) is dead; 10 / 11: ... is live
                        const int pq0 = qt * C::BM + (wave ^ 4) * 32;
                        const bool partner_live = pq0 < S && 2 * kb <= (pq0 >> 5);
                        if (live) { prof[partner_live ? 10 : 8] += e2 - e1; prof[partner_live ? 11 : 9] += 1; }
                    }
#endif
                    ring.step_end();
                }
                if (next_sense >= 0) adopt_q();
            }
        }
        wait_vmcnt<0>();   // the two re-fetched tiles: nothing may still be landing when the next job refills the ring

        if (wave_has_rows && my_q < S) {
            uint16_t *og = reinterpret_cast<uint16_t *>(p.o) + (VARLEN ? first_row * p.o_rs : batch * p.o_bs) + (int64_t)my_q * p.o_rs;
            mix_store_row<E, C>(og, acc, col_base, p.dout, hh);
        }
        MIX_TICK(job_t1);
        MIX_ADD(7, job_t1 - job_t0);
    }
#ifdef BP_MIX_PROFILE
    if (lane == 0 && blockIdx.x < 256)
        for (int k = 0; k < 12; ++k) g_mix_prof[blockIdx.x][wave][k] = prof[k];
#endif
}

}  // namespace bp
