// The register-staged tile schedule of the forward kernels that do not run on an LDS-DMA ring:
// flash_fwd.hip, attn_probs.hip, sense_mix.hip, sense_wide.hip.  This header owns the schedule's LDS formats and
// register maps; the kernels keep their tile sizes, their loop (fetch next / compute / stash next / barrier) and
// their masking.  attn_probs_kernel, sense_mix_kernel and sense_mix_wide_kernel use all of it; flash_fwd_kernel and
// the wide LSE / alpha kernels use the coordinates, S^T and the key map and keep loaders of their own (the reason
// stands with them).
//   * K rows: global -> registers (k_fetch, issued a tile ahead) -> LDS (k_stash), row pitch k_pitch(kd) bytes;
//   * one query row per lane, its fragments in registers (load_q_frags);
//   * S^T = K Q^T of 32 keys x the wave's 32 queries on v_mfma_f32_32x32x16 (st_half / st_half_wide); register r of
//     the result is key st_key(first key, r, hh);
//   * V / content rows: c_fetch / c_stash into the v_lds_off<NB> image, and O^T += C^T P^T with the operand read
//     through ds_read_b64_tr_b16 (accumulate_pv); P^T goes from the S^T registers into that MFMA as it stands;
//   * rows leave through store_acc_row (O) and store4 (probabilities).
// Every function is inlined and keeps the statement order of the kernel text it came from: the kernels are built
// without fast-math, so the results are the same bits.
//
// The online-softmax step of flash_fwd_kernel and sense_lse_wide_kernel is NOT shared.  The two differ in operations,
// not only in extent: flash_fwd reduces the maximum over 32 registers and exchanges it with ds_bpermute (xhalf),
// scaling max-or-zero by c2; the wide LSE reduces over 16, exchanges with v_permlane32_swap (xhalf_max) and selects
// between zero and the scaled maximum.  One function would have to reorder one of them.
#pragma once
#include <type_traits>

#include "bp_common.h"

namespace bp {

// ---- coordinates --------------------------------------------------------------------------------------------------------
struct LaneCoord {
    int tid, lane, wave, l31, hh;
};
BP_DEV LaneCoord lane_coord() {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    return LaneCoord{tid, lane, __builtin_amdgcn_readfirstlane(tid >> 6), lane & 31, lane >> 5};
}

// the 32 query rows of a wave inside a workgroup's query tile that starts at row `tile_q0`
struct QueryRows {
    int q0, my_q;          // first row of the wave, row of this lane
    bool wave_has_rows;    // wave-uniform
};
BP_DEV QueryRows query_rows(const LaneCoord &L, int tile_q0, int nq) {
    const int q0 = tile_q0 + L.wave * 32;
    return QueryRows{q0, q0 + L.l31, q0 < nq};
}

// Register r of a 32x32 MFMA result (bp_common.h, D layout) whose first row is `base` holds row st_key(base, r, hh): a
// key in S^T, an output column in O^T.  Registers 4g .. 4g+3 are four consecutive rows.
// The sum runs left to right from the wave-uniform base on purpose: summed as base + (register part + 4 hh), the
// compiler keeps one lane-dependent value per register live across the key loop (+30 VGPRs in attn_probs_kernel).
constexpr int st_key(int base, int r, int hh) { return base + (r & 3) + 8 * (r >> 2) + 4 * hh; }

// where the lane points its transposed reads (lds_image.h)
BP_DEV TrLane tr_lane(const LaneCoord &L) { return tr_lane(L.lane, L.hh); }

// ---- K tile -------------------------------------------------------------------------------------------------------------
// LDS image of a K tile: row pitch 32 bytes per 16-column step plus 16 (conflict-free ds_read_b128)
constexpr int k_pitch(int kd) { return kd * 32 + 16; }
// 16-byte chunks per thread of a tile of `rows` rows
constexpr int tile_iters(int rows, int chunks_per_row, int nt) { return (rows * chunks_per_row + nt - 1) / nt; }

// `rows` keys from key0 of the rows at kg -> the caller's registers.  Keys at or past nkeys and columns at or past d are
// ZERO in the image: the S^T MFMAs run over whole 16-column steps and whole 32-key halves.
// kd = 16-column steps per row: a std::integral_constant in the narrow kernels (every division folds), an int <= the
// bound that sized ITERS in the wide ones.
template <bool VEC, int ROWS, int NT, int ITERS, class KDv>
BP_DEV void k_fetch(u32x4 (&reg)[ITERS], const uint16_t *kg, int64_t row_stride, int key0, int nkeys, int d, KDv kd,
                    int tid) {
    const int kch = kd * 2;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
        const int c = tid + i * NT;
        const int row = c / kch, ch = c - row * kch;
        const int key = key0 + row;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (c < ROWS * kch && key < nkeys && ch * 8 < d) {
            const uint16_t *r = kg + (int64_t)key * row_stride;
            v = VEC ? ld_global_16B(r + ch * 8) : ld_global_8x2B(r, ch * 8, d);
        }
        reg[i] = v;
    }
}
template <int ROWS, int NT, int ITERS, class KDv>
BP_DEV void k_stash(const u32x4 (&reg)[ITERS], char *kbuf, KDv kd, int tid) {
    const int kch = kd * 2, krow = k_pitch(kd);
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
        const int c = tid + i * NT;
        const int row = c / kch, ch = c - row * kch;
        if (c < ROWS * kch) lds_write_16B(kbuf, row * krow + ch * 16, reg[i]);
    }
}

// ---- Q fragments --------------------------------------------------------------------------------------------------------
// The fragments of query row `row` of the rows at qg (B operand of S^T = K Q^T): columns 16 s + 8 hh .. +7 in step s;
// zero past d and for a row at or past nrows.
template <bool VEC, int KD>
BP_DEV void load_q_frags(u32x4 (&qf)[KD], const uint16_t *qg, int64_t row_stride, int row, int nrows, int d, int hh) {
#pragma unroll
    for (int s = 0; s < KD; ++s) {
        const int col = 16 * s + 8 * hh;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (row < nrows && col < d) {
            const uint16_t *qrow = qg + (int64_t)row * row_stride;
            v = VEC ? ld_global_16B(qrow + col) : ld_global_8x2B(qrow, col, d);
        }
        qf[s] = v;
    }
}

// ---- S^T of one 32-key half ---------------------------------------------------------------------------------------------
// where a lane reads its A fragments of S^T in a K tile (key row l31, half-wave's 16 bytes; + 32 per step)
BP_DEV int k_lane_off(int kd, int l31, int hh) { return l31 * k_pitch(kd) + hh * 16; }

// st[r] = q[my_q] . k[st_key(32 * half, r, hh)] of the tile at kbuf: one accumulation chain over the KD steps.
// k_lane = k_lane_off(KD, l31, hh), computed once per kernel.
template <class ET, int KD>
BP_DEV f32x16 st_half(const char *kbuf, const u32x4 (&qf)[KD], int k_lane, int half) {
    f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int s = 0; s < KD; ++s) {
        const u32x4 a = lds_read_16B(kbuf, k_lane + half * 32 * k_pitch(KD) + s * 32);
        st = Elem<ET>::mfma(a, qf[s], st);
    }
    return st;
}

// The same for a run-time step count kd <= KDT (tiles of 32 keys: one half).  Two accumulation chains (even / odd steps)
// so that consecutive MFMAs do not wait for each other; the fragments of the steps >= kd hold zeros and are skipped.
template <class ET, int KDT>
BP_DEV f32x16 st_half_wide(const char *kbuf, const u32x4 (&qf)[KDT], int kd, int l31, int hh) {
    using E = Elem<ET>;
    f32x16 st0, st1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { st0[r] = 0.f; st1[r] = 0.f; }
    const int k_lane = k_lane_off(kd, l31, hh);
#pragma unroll
    for (int s = 0; s < KDT; ++s)
        if (s < kd) {
            const u32x4 a = lds_read_16B(kbuf, k_lane + s * 32);
            if (s & 1) st1 = E::mfma(a, qf[s], st1);
            else st0 = E::mfma(a, qf[s], st0);
        }
    settle_acc(st1);   // the run-time bound `s < kd` puts a branch behind every MFMA: wait for the matrix pipe here (bp_common.h)
    pin_acc(st0);
#pragma unroll
    for (int r = 0; r < 16; ++r) st0[r] += st1[r];
    return st0;
}

// ---- V / content tile ---------------------------------------------------------------------------------------------------
// ROWS keys from key0, columns col_base .. col_base + 32 NB of the rows at cg -> registers -> the v_lds_off<NB> image.
// Keys at or past nkeys and columns at or past ncols MUST be zero: their probabilities are zero, and 0 * NaN = NaN in PV.
template <bool VEC, int NB, int ROWS, int NT, int ITERS>
BP_DEV void c_fetch(u32x4 (&reg)[ITERS], const uint16_t *cg, int64_t row_stride, int key0, int nkeys, int col_base,
                    int ncols, int tid) {
    constexpr int CCH = NB * 4;   // 16-byte chunks per row
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
        const int c = tid + i * NT;
        const int row = c / CCH, ch = c - row * CCH;
        const int key = key0 + row;
        const int col = col_base + ch * 8;
        u32x4 v = {0u, 0u, 0u, 0u};
        if ((ROWS * CCH % NT == 0 || c < ROWS * CCH) && key < nkeys && col < ncols) {
            const uint16_t *r = cg + (int64_t)key * row_stride;
            v = VEC ? ld_global_16B(r + col) : ld_global_8x2B(r, col, ncols);
        }
        reg[i] = v;
    }
}
template <int NB, int ROWS, int NT, int ITERS>
BP_DEV void c_stash(const u32x4 (&reg)[ITERS], char *cbuf, int tid) {
    constexpr int CCH = NB * 4;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
        const int c = tid + i * NT;
        const int row = c / CCH, ch = c - row * CCH;
        if (ROWS * CCH % NT == 0 || c < ROWS * CCH) lds_write_16B(cbuf, v_lds_off<NB>(row, ch), reg[i]);
    }
}

// O^T += C^T P^T for the 32 keys from row `row_base` of the tile at cbuf and the column blocks n < nb_live (wave-uniform).
// p holds the 16 probabilities of my query as S^T left them; registers 8 ks .. 8 ks + 7 are the B operand of key step ks.
template <class ET, int NB>
BP_DEV void accumulate_pv(f32x16 (&acc)[NB], const f32x16 &p, const char *cbuf, int row_base, const TrLane &t,
                          int nb_live) {
    using E = Elem<ET>;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        u32x4 pf;
#pragma unroll
        for (int i = 0; i < 4; ++i) pf[i] = E::pack2(p[ks * 8 + 2 * i], p[ks * 8 + 2 * i + 1]);
        const int row0 = row_base + ks * 16 + t.row;
#pragma unroll
        for (int n = 0; n < NB; ++n)
            if (n < nb_live) {
                const int ch = n * 4 + t.ch;
                acc[n] = E::mfma(tr_operand_at(cbuf, v_lds_off<NB>(row0, ch) + t.sub, v_lds_off<NB>(row0 + 8, ch) + t.sub), pf, acc[n]);
            }
    }
}

// ---- row epilogues ------------------------------------------------------------------------------------------------------
// My row of the O^T accumulators, times `scale`, to columns col0 .. of orow; columns at or past ncols are not written.
// VEC: four columns per 8-byte store (orow + col0 8-byte aligned, ncols a multiple of 4).  The default scale is exact
// and the compiler drops the multiplication.
template <class ET, bool VEC, int NB>
BP_DEV void store_acc_row(uint16_t *orow, const f32x16 (&acc)[NB], int col0, int ncols, int hh, float scale = 1.f) {
    using E = Elem<ET>;
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = st_key(col0 + n * 32, 4 * g, hh);
            const float x0 = acc[n][4 * g + 0] * scale, x1 = acc[n][4 * g + 1] * scale;
            const float x2 = acc[n][4 * g + 2] * scale, x3 = acc[n][4 * g + 3] * scale;
            if (VEC) {
                if (col < ncols) {
                    u32x2 w = {E::pack2(x0, x1), E::pack2(x2, x3)};
                    *reinterpret_cast<u32x2 *>(orow + col) = w;
                }
            } else {
                if (col + 0 < ncols) orow[col + 0] = E::from_float(x0);
                if (col + 1 < ncols) orow[col + 1] = E::from_float(x1);
                if (col + 2 < ncols) orow[col + 2] = E::from_float(x2);
                if (col + 3 < ncols) orow[col + 3] = E::from_float(x3);
            }
        }
}

// Four consecutive keys of a probability row: one 8-byte store when `vec` (prow + key0 8-byte aligned for every key0
// that is a multiple of 4) and the group lies inside the row, else element by element.
template <class ET>
BP_DEV void store4(uint16_t *prow, int key0, int nkeys, bool vec, float x0, float x1, float x2, float x3) {
    using E = Elem<ET>;
    if (vec && key0 + 3 < nkeys) {
        u32x2 w = {E::pack2(x0, x1), E::pack2(x2, x3)};
        *reinterpret_cast<u32x2 *>(prow + key0) = w;
    } else {
        if (key0 + 0 < nkeys) prow[key0 + 0] = E::from_float(x0);
        if (key0 + 1 < nkeys) prow[key0 + 1] = E::from_float(x1);
        if (key0 + 2 < nkeys) prow[key0 + 2] = E::from_float(x2);
        if (key0 + 3 < nkeys) prow[key0 + 3] = E::from_float(x3);
    }
}

}  // namespace bp
