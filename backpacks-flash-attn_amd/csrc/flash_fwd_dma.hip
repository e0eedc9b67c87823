// Fused attention forward for gfx950, LDS-DMA ring version: the fast path for 16-byte friendly
// shapes (head_dim % 8 == 0, aligned rows) -- every shape the reference kernel accepts
// (csrc/flash_attn/fmha_api.cpp:245).  Same math and tile algebra as flash_fwd.hip (bp_common.h):
//   * K/V tiles (64 keys) go straight from global memory to a 2-slot LDS ring with
//     global_load_lds_dwordx4: no VGPR staging, no ds_write pass, counted completion + ONE raw
//     s_barrier per tile (bp_dma.h); K rows: power-of-two pitch + XOR slot swizzle, V rows: 64-B chunk
//     swizzle, both applied on the DMA source address; every MFMA operand read is `lane base + immediate`.
//   * TWO tile bodies.  The kernel is bound by the VALU stream of the softmax, not by MFMA or memory
//     (DESIGN.md section 4), so the steady-state body carries the minimum: with the running reference
//     maximum m of a row fixed, p = exp2(s*c - m*c) and the row sum need no row maximum at all -- one fma,
//     one exp, one add and half a pack per score.  It is legal as long as no p overflows, and since
//     p >= 0 the tile's row sum bounds every p from above: ONE wave-wide compare of the 32 partial sums
//     against 2^14 (fp16) / 2^30 (bf16) validates the tile after the fact.  If it fails (a score jumped far
//     above everything the row has seen), nothing has been accumulated yet; the EXACT body recomputes the
//     tile from LDS with the textbook online-softmax step (true maximum, rescale of O and l) -- for the rows
//     whose own sums failed; the other rows of the wave keep their reference point through the repeat, so a
//     row's bits never depend on its wave-mates (online_max_step).  The exact body also serves every tile that
//     needs masking (sequence end, causal diagonal) and the first tile of a row, which sets m.  The reference keeps the exact form for every tile
//     (csrc/flash_attn/src/fmha/softmax.h:238-251, fmha_fprop_kernel_1xN.h:429-444); results agree to
//     rounding because softmax is invariant to the reference point.
//   * without dropout, P is rounded to 16 bit right behind the exponential and the row sum runs over the rounded
//     pairs (v_dot2c_f32_{bf16,f16} against {1, 1}): one VALU instruction per two scores, and the normaliser
//     is the sum of exactly the values that multiply V.
//   * in-kernel dropout (training; reference fmha_fprop_kernel_1xN.h:494-506): counter-based bits per
//     (batch*head, query, key), see bp_philox.h; dropped probabilities are zeroed AFTER the row sum, the
//     output is scaled by 1 / (1 - p) once in the epilogue.
#include "bp_common.h"
#include "bp_dma.h"
#include "bp_kernels.h"
#include "bp_philox.h"

namespace bp {

// waves per SIMD the register allocator must leave room for (512 VGPRs per SIMD lane): the trunk shapes
// (head_dim <= 64; <= 96 without dropout since the odd K pitch of round 4) run at least three workgroups per CU
constexpr int flash_min_waves(int nv, bool drop) { return nv <= 2 || (nv == 3 && !drop) ? 3 : 1; }

// Development builds only (-DBP_FWD_PROFILE, scripts/probes/flash_fwd_phases): every wave adds up s_memtime deltas per
// phase of a pass; never in the shipped library.
#ifdef BP_FWD_PROFILE
// [workgroup][wave][0 wait+barrier, 1 DMA issue, 2 S^T, 3 softmax, 4 PV, 5 exact tiles (whole), 6 #fast tiles, 7 pass clocks,
//  8 prologue (pass start -> first ring step), 9 epilogue, 10 #passes]
__device__ unsigned long long g_fwd_prof[8192][4][12];
#define FWD_TICK(var) const unsigned long long var = __builtin_readcyclecounter()
#define FWD_ADD(k, expr) prof[k] += (expr)
#else
#define FWD_TICK(var) do { } while (0)
#define FWD_ADD(k, expr) do { } while (0)
#endif

// four waves: 256-query workgroups of eight waves were 2-4 % slower at S = 1024 (profiles/r04_d_ab_flash_8wave_workgroups.jsonl)
template <int KD, int NV, bool HAS_V>
struct FlashDmaCfg {
    static constexpr int NWAVE = 4;
    static constexpr int BM = 32 * NWAVE, BN = 64, NT = 64 * NWAVE, NSTAGE = 2;
    // K row pitch in LDS.  Head dims 64 and 128 fill a power-of-two pitch (128 / 256 bytes) and XOR-swizzle the
    // 16-byte slots (RowImage, lds_image.h); every other width (d_h = 80: Mini; the senses' d_k = 48 / 24 / 16) takes an ODD number of slots,
    // 2 KD + 1 (a narrow K tile is also fewer DMA pieces: d_k = 16 moves 3 KB per tile instead of 8): the
    // quad-bank of (row, slot) is (row * KSLOTS + slot) mod 16, distinct for the 16 rows of every ds_read_b128 lane group
    // without any swizzle, and the tile shrinks from 16 KB to 11 / 13 / 15 KB -- at d_h = 80 that is 47 KB per workgroup
    // instead of 57 KB, i.e. three workgroups per CU instead of two (profiles/r04_j_ab_flash_odd_k_pitch_d80_d96_d112.jsonl).
    static constexpr bool ODD = KD != 4 && KD != 8;
    static constexpr int KSLOTS = ODD ? 2 * KD + 1 : KD <= 4 ? 8 : 16;
    static constexpr int KROW = KSLOTS * 16;
    static constexpr int VROW = NV * 64;
    static constexpr int VCH = NV * 4;
    static constexpr int KTILE = BN * KROW;
    static constexpr int VTILE = HAS_V ? BN * VROW : 0;
    static constexpr int STAGE = KTILE + VTILE;
    static constexpr int K_PIECES = KTILE / 1024;                 // 1-KiB DMA pieces per tile (8, 11, 13, 15 or 16)
    static constexpr int K_DMA = (K_PIECES + NWAVE - 1) / NWAVE;  // per wave per tile (the last wave may own fewer)
    static constexpr int V_DMA = HAS_V ? VTILE / 1024 / NWAVE : 0;  // 1..4
};

template <class ET> struct ProbLimit;   // largest tile row sum the fast body accepts (see header)
template <> struct ProbLimit<BF16> { static constexpr float value = 1073741824.f; };   // 2^30
template <> struct ProbLimit<F16> { static constexpr float value = 16384.f; };         // 2^14

// One 128-query tile `qt` of (sample, head) `bh`: the whole online-softmax sweep over its key tiles.
// FULLD: head_dim fills the K row pitch exactly (64 or 128): no predicated DMA pieces, no pad columns.
template <class ET, int KD, int NV, bool HAS_V, bool FULLD, bool DROP>
BP_DEV void flash_fwd_tile(const FlashParams p, char *smem, const uint32_t lds0, const int bh, const int qt) {
    using C = FlashDmaCfg<KD, NV, HAS_V>;
    using KI = RowImage<C::KROW>;   // K image: swizzled for the two power-of-two pitches, plain for the odd ones
    using E = Elem<ET>;
    constexpr float kLimit = ProbLimit<ET>::value;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int hh = lane >> 5;

    const int batch = bh / p.h;
    const int head = bh - batch * p.h;

    int seq_q, seq_k;
    int64_t q_off, k_off, v_off, o_off;
    if (p.cu_q != nullptr) {
        const int a = p.cu_q[batch], b = p.cu_q[batch + 1];
        const int c = p.cu_k[batch], d = p.cu_k[batch + 1];
        seq_q = b - a; seq_k = d - c;
        q_off = a * p.q_rs; o_off = a * p.o_rs; k_off = c * p.k_rs; v_off = c * p.v_rs;
    } else {
        seq_q = p.max_sq; seq_k = p.max_sk;
        q_off = batch * p.q_bs; o_off = batch * p.o_bs; k_off = batch * p.k_bs; v_off = batch * p.v_bs;
    }
    if (qt * C::BM >= seq_q) return;
#ifdef BP_FWD_PROFILE
    unsigned long long prof[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    FWD_TICK(pass_t0);

    const uint16_t *qg = reinterpret_cast<const uint16_t *>(p.q) + q_off + (int64_t)head * p.q_hs;
    const uint16_t *kg = reinterpret_cast<const uint16_t *>(p.k) + k_off + (int64_t)head * p.k_hs;
    const uint16_t *vg = HAS_V ? reinterpret_cast<const uint16_t *>(p.v) + v_off + (int64_t)head * p.v_hs : nullptr;

    int k_end = seq_k;
    if (p.causal) k_end = min(seq_k, qt * C::BM + C::BM);
    const int nkb = (k_end + C::BN - 1) / C::BN;

    const int q0 = qt * C::BM + wave * 32;
    const int my_q = q0 + l31;
    const bool wave_has_rows = q0 < seq_q;
    const float c2 = p.scale_log2e;

    // Which key tiles this wave computes, and which of them the fast body may take: a tile is "clean" when
    // every key exists and every (query, key) pair of my 32 rows is visible.
    const int my_nkb = !wave_has_rows ? 0 : p.causal ? min(nkb, (q0 + 31) / C::BN + 1) : nkb;
    const int my_clean_end = p.causal ? min(seq_k / C::BN, (q0 + 1) / C::BN) : seq_k / C::BN;

    // K pad slots (head_dim not a multiple of 16, or pitch wider than the row) are never written by
    // the DMA and meet zero Q columns in the MFMA: they must hold finite values -> zero them once.
    if (!FULLD) {
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (int off = tid * 16; off < C::NSTAGE * C::STAGE; off += C::NT * 16) lds_write_16B(smem, off, z);
        __syncthreads();
    }

    DropoutStream rng = {0u, 0u};
    if (DROP) rng = dropout_stream(p.rng_state, (uint32_t)bh);

    // ---- Q fragments (B operand of S^T = K Q^T) ----------------------------------------------------
    u32x4 qf[KD];
    {
        const uint16_t *row = qg + (int64_t)min(my_q, seq_q - 1) * p.q_rs;
#pragma unroll
        for (int s = 0; s < KD; ++s) {
            const int col = 16 * s + 8 * hh;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (FULLD || col < p.d) v = ld_global_16B(row + col);
            qf[s] = v;
        }
#pragma unroll
        for (int s = 0; s < KD; ++s) settle(qf[s]);
    }

    // ---- per-lane DMA source descriptors: tile row / column of the 16-B chunk this lane moves ----------
    int k_row[C::K_DMA], k_col[C::K_DMA];
    uint32_t k_voff[C::K_DMA];
#pragma unroll
    for (int j = 0; j < C::K_DMA; ++j) {
        // lane's 16 bytes of piece (wave * K_DMA + j): linear 16-byte slot of the tile image (lds_image.h)
        const TileSrc s = KI::src((wave * C::K_DMA + j) * 64 + lane);
        k_row[j] = s.row;
        k_col[j] = s.col;
        k_voff[j] = (uint32_t)(s.row * p.k_rs + s.col) * 2u;
    }
    int v_row[HAS_V ? C::V_DMA : 1], v_col[HAS_V ? C::V_DMA : 1];
    uint32_t v_voff[HAS_V ? C::V_DMA : 1];
    if (HAS_V) {
#pragma unroll
        for (int j = 0; j < C::V_DMA; ++j) {
            // (TrImage<NV>::src spelled here, as are tr_lane and the read pairs below: through the header the V kernels' code differed)
            const int c = (wave * C::V_DMA + j) * 64 + lane;   // linear 16-B chunk of the tile
            const int row = c / C::VCH, stored = c - row * C::VCH;
            int c64 = stored >> 2;
            if (NV == 2) c64 ^= (row >> 1) & 1;
            if (NV == 4) c64 ^= row & 3;
            v_row[j] = row;
            v_col[j] = ((c64 << 2) | (stored & 3)) * 8;
            v_voff[j] = (uint32_t)(row * p.v_rs + v_col[j]) * 2u;
        }
    }
    // Scalar tile base + constant per-lane byte offset -> no VALU at all.  The only partial tile a sweep can meet is
    // the sequence's last one; its rows are clamped to the final valid key (those keys are masked later): the clamped
    // offsets are recomputed from the lane's row in that one (cold) step instead of living in registers all along.
    const int kb_partial = (seq_k % C::BN) != 0 ? seq_k / C::BN : -1;
    const int last_row = seq_k - 1 - (seq_k / C::BN) * C::BN;
    const int64_t k_tile_stride = (int64_t)C::BN * p.k_rs, v_tile_stride = (int64_t)C::BN * p.v_rs;
    const uint16_t *kt = kg, *vt = vg;   // tile kb of the NEXT issue (tiles are issued in order 0, 1, 2, ...)
    auto issue = [&](int kb) {
        // (readfirstlane: inside the per-lane predicate of the !FULLD case hipcc may hold the uniform address in a VGPR)
        const uint32_t stage = __builtin_amdgcn_readfirstlane(lds0 + (kb & 1) * C::STAGE);
        if (__builtin_expect(kb == kb_partial, 0)) {
#pragma unroll
            for (int j = 0; j < C::K_DMA; ++j) {
                const int row = ((wave * C::K_DMA + j) * 64 + lane) / C::KSLOTS;
                const uint32_t back = (uint32_t)(max(row - last_row, 0) * p.k_rs) * 2u;
                if (wave * C::K_DMA + j < C::K_PIECES && (FULLD || k_col[j] < p.d))
                    dma16_s(kt, k_voff[j] - back, __builtin_amdgcn_readfirstlane(stage + (wave * C::K_DMA + j) * 1024));
            }
            if (HAS_V) {
#pragma unroll
                for (int j = 0; j < C::V_DMA; ++j) {
                    const int row = ((wave * C::V_DMA + j) * 64 + lane) / C::VCH;
                    const uint32_t back = (uint32_t)(max(row - last_row, 0) * p.v_rs) * 2u;
                    if (FULLD || v_col[j] < p.d)
                        dma16_s(vt, v_voff[j] - back,
                                __builtin_amdgcn_readfirstlane(stage + C::KTILE + (wave * C::V_DMA + j) * 1024));
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < C::K_DMA; ++j)
                if (wave * C::K_DMA + j < C::K_PIECES && (FULLD || k_col[j] < p.d))
                    dma16_s(kt, k_voff[j], __builtin_amdgcn_readfirstlane(stage + (wave * C::K_DMA + j) * 1024));
            if (HAS_V) {
#pragma unroll
                for (int j = 0; j < C::V_DMA; ++j)
                    if (FULLD || v_col[j] < p.d)
                        dma16_s(vt, v_voff[j],
                                __builtin_amdgcn_readfirstlane(stage + C::KTILE + (wave * C::V_DMA + j) * 1024));
            }
        }
        if (HAS_V) vt += v_tile_stride;
        kt += k_tile_stride;
    };

    f32x16 acc[HAS_V ? NV : 1];
#pragma unroll
    for (int n = 0; n < (HAS_V ? NV : 1); ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    float m_run = -INFINITY;   // reference maximum of my row (raw score units)
    float mc = 0.f;            // m_run * c2, 0 while the row has seen no key
    float l_run = 0.f;         // my half-wave's share of sum p

    int k_read_off[KD];
#pragma unroll
    for (int s = 0; s < KD; ++s)
        k_read_off[s] = KI::read_off(l31, hh, s);
    int v_read_off[HAS_V ? NV : 1];
    if (HAS_V) {
        const int v_row_lane = 4 * hh + ((lane & 15) >> 2);
        const int v_ch_lane = ((lane >> 4) & 1) * 2 + ((lane & 3) >> 1);
#pragma unroll
        for (int n = 0; n < NV; ++n) v_read_off[n] = v_lds_off<NV>(v_row_lane, n * 4 + v_ch_lane) + (lane & 1) * 8;
    }

    // p (in place) = exp2(s*c2 - mc), returns my share of the row sum
    auto exponentiate = [&](f32x16 (&st)[2]) {
        float rs0 = 0.f, rs1 = 0.f;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float x0 = fast_exp2(fmaf(st[kk][r], c2, -mc));
                const float x1 = fast_exp2(fmaf(st[kk][r + 1], c2, -mc));
                st[kk][r] = x0;
                st[kk][r + 1] = x1;
                rs0 += x0;
                rs1 += x1;
            }
        return rs0 + rs1;
    };
    // Without dropout P is rounded to 16 bit right behind the exponential and the row sum is taken over the ROUNDED
    // pairs, one v_dot2c_f32_{bf16,f16} per two scores instead of two adds: the sum then normalises exactly the
    // values that multiply V, and the VALU stream this kernel is bound by is 16 instructions per tile shorter.
    constexpr bool PACKED_SUM = HAS_V && !DROP;
    u32x4 pf[2][2];   // [32-key half][16-key step]
    auto exponentiate_packed = [&](f32x16 (&st)[2]) {
        float rs0 = 0.f, rs1 = 0.f;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = ks * 8 + 2 * i;
                    const float x0 = fast_exp2(fmaf(st[kk][r], c2, -mc));
                    const float x1 = fast_exp2(fmaf(st[kk][r + 1], c2, -mc));
                    const uint32_t w = E::pack2(x0, x1);
                    pf[kk][ks][i] = w;
                    if (i & 1) rs1 = E::add_pair(w, rs1);
                    else rs0 = E::add_pair(w, rs0);
                }
        return rs0 + rs1;
    };
    auto accumulate_packed = [&](const char *vbuf, bool skip_hi) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            if (kk == 1 && skip_hi) continue;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int rows = (kk * 32 + ks * 16) * C::VROW;
#pragma unroll
                for (int n = 0; n < NV; ++n) {
                    const u32x2 lo = lds_read_tr16_8B(vbuf, v_read_off[n] + rows);
                    const u32x2 hi = lds_read_tr16_8B(vbuf, v_read_off[n] + rows + 8 * C::VROW);
                    const u32x4 a = {lo[0], lo[1], hi[0], hi[1]};
                    acc[n] = E::mfma(a, pf[kk][ks], acc[n]);
                }
            }
        }
    };
    // dropout (after the row sum), then O^T += V^T P^T
    auto accumulate = [&](int kb, const char *vbuf, f32x16 (&st)[2], bool skip_hi) {
        if (!HAS_V) return;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            if (kk == 1 && skip_hi) continue;
            if (DROP) {
                const uint32_t keep = dropout_keep_rowlane(rng, p.drop_thr, (uint32_t)my_q,
                                                           (uint32_t)(kb * C::BN + kk * 32), hh);
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (!((keep >> r) & 1u)) st[kk][r] = 0.f;
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                u32x4 pf;
#pragma unroll
                for (int i = 0; i < 4; ++i) pf[i] = E::pack2(st[kk][ks * 8 + 2 * i], st[kk][ks * 8 + 2 * i + 1]);
                const int rows = (kk * 32 + ks * 16) * C::VROW;
#pragma unroll
                for (int n = 0; n < NV; ++n) {
                    const u32x2 lo = lds_read_tr16_8B(vbuf, v_read_off[n] + rows);
                    const u32x2 hi = lds_read_tr16_8B(vbuf, v_read_off[n] + rows + 8 * C::VROW);
                    const u32x4 a = {lo[0], lo[1], hi[0], hi[1]};
                    acc[n] = E::mfma(a, pf, acc[n]);
                }
            }
        }
    };

    // Textbook online-softmax bookkeeping of one tile, on raw scores (in place): mask what my row may not see,
    // take the true tile maximum, move the row's reference maximum and rescale O and l accordingly.
    // `moves` (per lane): this row takes the tile's maximum into its reference point.  True for every row of a tile that
    // is exact by POSITION (first tile, masked tile); in a RETRY only for the rows whose own sums failed the validation --
    // the others keep their reference (alpha = 1 exactly, the same exponent offsets), i.e. they come out with the bits the
    // steady-state body would have given them: whether a wave repeats a tile depends on all 32 rows, the result of a row
    // only on that row (tests/test_gpu_properties.py: what precedes a cut never depends on what follows it).
    auto online_max_step = [&](int kb, f32x16 (&st)[2], bool moves) {
        // register r of half kk holds key base + kk*32 + (r&3) + 8*(r>>2) + 4*hh: dead iff that exceeds the last
        // visible key of my row -> ONE per-lane limit against compile-time constants
        int last = seq_k - 1;
        if (p.causal) last = min(last, my_q);
        int lim = last - kb * C::BN - 4 * hh;
        // (opaque on purpose: otherwise hipcc speculates the 32 compares out of this rarely taken branch into every tile)
        asm volatile("" : "+v"(lim));
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kk * 32 + (r & 3) + 8 * (r >> 2) > lim) st[kk][r] = -INFINITY;
        // row max: four independent chains, then the other half-wave
        float mxa = st[0][0], mxb = st[0][8], mxc = st[1][0], mxd = st[1][8];
#pragma unroll
        for (int r = 1; r < 8; ++r) {
            mxa = fmaxf(mxa, st[0][r]);
            mxb = fmaxf(mxb, st[0][8 + r]);
            mxc = fmaxf(mxc, st[1][r]);
            mxd = fmaxf(mxd, st[1][8 + r]);
        }
        const float mt = xhalf_max(fmaxf(fmaxf(mxa, mxb), fmaxf(mxc, mxd)));
        const float m_new = moves ? fmaxf(mt, m_run) : m_run;
        // alpha = 1 exactly for a row whose maximum did not move; exp2(-inf - x) = 0 for a fresh row, whose (zero) O
        // and l are "rescaled" harmlessly
        const float mc_new = !moves ? mc : (m_new == -INFINITY) ? 0.f : m_new * c2;
        // (a row that keeps its reference: 1 by construction, not by the exponent's arithmetic -- contracted into an fma,
        // m_run * c2 - mc_new is the rounding error of the product, not 0; for the same reason a row that moves but whose
        // maximum this tile does not raise -- a key that ties with an earlier tile's best included -- takes 1 as well:
        // 2^(half an ulp of m c2) is 1 + 2e-5 at m c2 ~ 500, and O = (a V1 + V2) / (a + 1) then leaves 1e-5 |V| where
        // V1 = -V2; tests/test_gpu_prefill_needles.py, test_pair_flash_fwd_rows_are_the_means_of_their_needles)
        const float alpha = (moves && m_new != m_run) ? fast_exp2(m_run * c2 - mc_new) : 1.f;
        l_run *= alpha;
        if (HAS_V) {
#pragma unroll
            for (int n = 0; n < NV; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[n][r] *= alpha;
        }
        m_run = m_new;
        mc = mc_new;
    };

    // One key tile.  `exact`: the tile needs masking (sequence end, causal diagonal) or is the first of the row ->
    // the textbook step above runs before the exponentials.  Otherwise the steady-state form: the reference
    // maximum stays, and if its overflow test fails afterwards (rare; nothing accumulated yet) the SAME code runs
    // once more on scores recomputed from LDS, the textbook way.
    auto tile = [&](int kb, const char *kbuf, const char *vbuf, bool exact) {
        f32x16 st[2];
        float rs;
        bool moves = true;
        const bool fast_entry = !exact;
        FWD_TICK(t0);
#ifdef BP_FWD_PROFILE
        unsigned long long t_s = t0, t_e = t0;
#endif
        for (;;) {
            {   // S^T of both 32-key halves as one operand stream, alternating accumulators; operand i + 2 requested
                // before MFMA i (profiles/r03_ao_flash_fwd_diet_stream_ab.jsonl)
                f32x16 zero;
#pragma unroll
                for (int r = 0; r < 16; ++r) zero[r] = 0.f;
                mfma_stream<2 * KD>(
                    [&](int i) { return lds_read_16B(kbuf, k_read_off[i >> 1] + (i & 1) * 32 * C::KROW); },
                    [&](int i, const u32x4 &a) { st[i & 1] = E::mfma(a, qf[i >> 1], i < 2 ? zero : st[i & 1]); });
            }
#ifdef BP_FWD_PROFILE
            asm volatile("" : "+v"(st[0]), "+v"(st[1]));
            t_s = __builtin_readcyclecounter();
#endif
            if (__builtin_expect(exact, 0)) online_max_step(kb, st, moves);
            rs = PACKED_SUM ? exponentiate_packed(st) : exponentiate(st);
            if (__builtin_expect(exact || __all(rs <= kLimit), 1)) break;   // inf and NaN fail the test too
            // a row's keys are summed by two lanes (l and l ^ 32): the row moves if either share failed
            moves = xhalf_max(rs <= kLimit ? 0.f : 1.f) != 0.f;
            exact = true;
        }
#ifdef BP_FWD_PROFILE
        if (PACKED_SUM) asm volatile("" : "+v"(pf[0][0]), "+v"(pf[0][1]), "+v"(pf[1][0]), "+v"(pf[1][1]), "+v"(rs));
        t_e = __builtin_readcyclecounter();
#endif
        l_run += rs;
        // second 32-key half entirely above my rows (diagonal tile): all its p are 0
        const bool skip_hi = p.causal && (kb * C::BN + 32 > q0 + 31);
        if (PACKED_SUM) accumulate_packed(vbuf, skip_hi);
        else accumulate(kb, vbuf, st, skip_hi);
#ifdef BP_FWD_PROFILE
        asm volatile("" : "+v"(acc[0]), "+v"(acc[NV - 1]));
        const unsigned long long t_p = __builtin_readcyclecounter();
        if (fast_entry && !exact) {
            prof[2] += t_s - t0; prof[3] += t_e - t_s; prof[4] += t_p - t_e; prof[6] += 1;
        } else {
            prof[5] += t_p - t0;
        }
#endif
    };


    if (nkb > 0) issue(0);
    // (the first tile's DMA issued BEFORE the wait for the Q fragments, so that the two round trips of a pass's prologue
    // overlap, was measured on its own in round 6: +-1 %, profiles/r06_e_ab_flash_issue_first.jsonl -- not kept)
    // One ring step; SLOT is the ring slot as a compile-time constant (the loop is unrolled by the ring depth), so
    // the LDS addresses of all operand reads fold into instruction offsets.
    auto ring_step = [&](int kb, auto SLOT) {
        constexpr int kSlot = decltype(SLOT)::value;
        FWD_TICK(r0);
#ifdef BP_FWD_PROFILE
        if (kb == 0) prof[8] += r0 - pass_t0;
#endif
        wait_vmcnt<0>();                    // my share of tile kb has landed ...
        __builtin_amdgcn_s_barrier();       // ... so has everybody's; all waves are done reading the other slot
        FWD_TICK(r1);
        FWD_ADD(0, r1 - r0);
        if (kb + 1 < nkb) issue(kb + 1);
        FWD_TICK(r2);
        FWD_ADD(1, r2 - r1);
        if (kb < my_nkb) {
            const char *kbuf = smem + kSlot * C::STAGE;
            const char *vbuf = kbuf + C::KTILE;
            tile(kb, kbuf, vbuf, kb == 0 || kb >= my_clean_end);
        }
    };
    for (int kb = 0; kb < nkb; kb += 2) {
        ring_step(kb, std::integral_constant<int, 0>{});
        if (kb + 1 < nkb) ring_step(kb + 1, std::integral_constant<int, 1>{});
    }

    FWD_TICK(ep0);
#ifdef BP_FWD_PROFILE
    auto flush = [&](unsigned long long t_end) {
        prof[9] += t_end - ep0; prof[7] += t_end - pass_t0; prof[10] += 1;
        if (lane == 0 && blockIdx.x < 8192)
            for (int k = 0; k < 12; ++k) atomicAdd(&g_fwd_prof[blockIdx.x][wave][k], prof[k]);
    };
    if (!wave_has_rows) { flush(__builtin_readcyclecounter()); return; }
#else
    if (!wave_has_rows) return;
#endif
    const float l_tot = xhalf_sum(l_run);
    float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    if (DROP) inv *= p.drop_scale;
    if (my_q < seq_q) {
        if (hh == 0 && p.lse != nullptr) {
            const float lse = l_tot > 0.f ? (mc + fast_log2(l_tot)) * kLn2 : -INFINITY;
            p.lse[((int64_t)batch * p.h + head) * p.lse_stride + my_q] = lse;
        }
        if (HAS_V) {
            uint16_t *og = reinterpret_cast<uint16_t *>(p.o) + o_off + (int64_t)my_q * p.o_rs + (int64_t)head * p.o_hs;
            // 16-byte column groups: a lane holds columns 8g + 4hh .. +3 of its row for every g; one v_permlane32_swap per
            // dword pairs groups (g, g + 1) across the half-waves -- the lower half-wave then owns columns 8g .. 8g+7, the
            // upper one 8(g+1) .. 8(g+1)+7 -- and the epilogue issues half the store instructions for the same bytes
            // (the store tail of a row-per-lane epilogue is bound by store ISSUE, not bandwidth: cdna_hip_programming T21;
            // profiles/r06_c_ab_flash_wide_store.jsonl)
#pragma unroll
            for (int n = 0; n < NV; ++n)
#pragma unroll
                for (int g = 0; g < 4; g += 2) {
                    const uint32_t a0 = E::pack2(acc[n][4 * g + 0] * inv, acc[n][4 * g + 1] * inv);
                    const uint32_t a1 = E::pack2(acc[n][4 * g + 2] * inv, acc[n][4 * g + 3] * inv);
                    const uint32_t b0 = E::pack2(acc[n][4 * g + 4] * inv, acc[n][4 * g + 5] * inv);
                    const uint32_t b1 = E::pack2(acc[n][4 * g + 6] * inv, acc[n][4 * g + 7] * inv);
                    auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
                    auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
                    const uint32_t x0 = r0[0], y0 = r0[1], x1 = r1[0], y1 = r1[1];
                    const int d0 = n * 32 + 8 * g + 8 * hh;
                    if (d0 < p.d) {
                        const u32x4 w = {x0, x1, y0, y1};
                        *reinterpret_cast<u32x4 *>(og + d0) = w;
                    }
                }
        }
    }
#ifdef BP_FWD_PROFILE
    flush(__builtin_readcyclecounter());
#endif
}

// Work order.  The dispatcher hands workgroups to the CUs of an XCD strictly round-robin and IN ORDER: block
// i+1 is not placed before block i, and block i waits for a free slot on ITS CU even when other CUs idle
// (scripts/probes/dispatch_order.hip).  With causal tiles of 1..n key blocks in block order, a CU keeps getting
// the same tile length and the short ones wait for the long ones: 64 time units instead of 36 for S = 1024 in a
// model of that dispatcher, and 8.3 vs 5.9 ms in the probe.  So a causal workgroup takes TWO query tiles of its
// (sample, head), the heaviest remaining and the lightest (t and n-1-t): every workgroup then carries the same
// n+1 key blocks, nothing waits, and both tiles still belong to one group, i.e. one XCD's L2 holds their K/V.
template <class ET, int KD, int NV, bool HAS_V, bool FULLD, bool DROP>
__global__ __launch_bounds__((FlashDmaCfg<KD, NV, HAS_V>::NT), flash_min_waves(NV, DROP))
void flash_fwd_dma_kernel(const FlashParams p) {
    using C = FlashDmaCfg<KD, NV, HAS_V>;
    __shared__ __attribute__((aligned(16))) char smem[C::NSTAGE * C::STAGE];
    const uint32_t lds0 = lds_base_addr(smem);
    const int n_qtiles = (p.max_sq + C::BM - 1) / C::BM;   // (the host's p.n_qtiles counts 128-query tiles)
    const bool pair = p.pair && n_qtiles > 1;
    const int per_group = pair ? (n_qtiles + 1) / 2 : n_qtiles;
    int bh, slot;
    if (!xcd_map(blockIdx.x, p.b * p.h, per_group, bh, slot)) return;
    // (round 4, r04_g: the workgroups resident on one CU are XCD-local blocks c, c + 32, c + 64, ... and therefore all carry the
    // SAME pair of query tiles; rotating the pair index by the residency round and / or running the light tile first in
    // every other round, so that co-resident workgroups are never in the same phase, changed nothing: +-0.5 %)
    const int heavy = n_qtiles - 1 - slot;
    const int npass = (pair && slot != heavy) ? 2 : 1;
    for (int pass = 0; pass < npass; ++pass) {
        if (pass) __syncthreads();   // every wave is done with the ring before the next tile's DMA refills it
        flash_fwd_tile<ET, KD, NV, HAS_V, FULLD, DROP>(p, smem, lds0, bh, pass ? slot : heavy);
    }
}

template <class ET, int KD, int NV, bool HAS_V, bool FULLD, bool DROP>
static hipError_t launch_one(const FlashParams &p, hipStream_t stream) {
    using C = FlashDmaCfg<KD, NV, HAS_V>;
    const int n_qtiles = (p.max_sq + C::BM - 1) / C::BM;
    const int grid = xcd_grid(p.b * p.h, (p.pair && n_qtiles > 1) ? (n_qtiles + 1) / 2 : n_qtiles);
    hipLaunchKernelGGL((flash_fwd_dma_kernel<ET, KD, NV, HAS_V, FULLD, DROP>), dim3(grid), dim3(C::NT), 0, stream, p);
    return hipGetLastError();
}

template <class ET, int KD, bool HAS_V, bool DROP>
static hipError_t launch_kd(const FlashParams &p, hipStream_t stream) {
    constexpr int NV = trunk_nv(KD);
    using C = FlashDmaCfg<KD, NV, HAS_V>;
    if constexpr (KD == 4 || KD == 8) {
        if (p.d * 2 == C::KROW) return launch_one<ET, KD, NV, HAS_V, true, DROP>(p, stream);
    }
    return launch_one<ET, KD, NV, HAS_V, false, DROP>(p, stream);
}

// Requires head_dim % 8 == 0, 16-byte aligned bases, strides multiples of 8, seq_k >= 1 per sequence
// handled inside (nkb == 0 issues nothing).  Dropout only with a V operand.
hipError_t launch_flash_fwd_dma(const FlashParams &p, int dtype, hipStream_t stream) {
    return with_dtype(dtype, [&](auto et) {
        return with_kd(p.d, [&](auto kd) {
            using ET = decltype(et);
            if (p.v == nullptr) return launch_kd<ET, kd, false, false>(p, stream);
            return with_flag(p.drop_thr != 0u, [&](auto drop) { return launch_kd<ET, kd, true, drop>(p, stream); });
        });
    });
}

#ifdef BP_FWD_PROFILE
extern "C" int bp_dev_fwd_prof(unsigned long long *host, int clear) {
    if (clear) {
        void *ptr = nullptr;
        if (hipGetSymbolAddress(&ptr, HIP_SYMBOL(g_fwd_prof)) != hipSuccess) return -1;
        return hipMemset(ptr, 0, sizeof(g_fwd_prof)) == hipSuccess ? 0 : -1;
    }
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_fwd_prof), sizeof(g_fwd_prof)) == hipSuccess ? 0 : -1;
}
#endif

}  // namespace bp
