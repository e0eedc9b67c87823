// bp_sense_mix_gather_mx8: the fused sense combination with the content rows read from the MXFP8 sense table
// (include/bp_hip.h, "MXFP8 sense table"), so that prefill and the eval forward need no 16-bit table:
//
//     out[b,t,:] = sum_l sum_{s<=t} exp(scale * q_l[t].k_l[s] - lse[b,l,t]) * e4m3(q8[row(b,s), l, :]) * 2^(scale8[row(b,s), l, :/32] - 127)
//
// The LDS-DMA ring of sense_mix_dma.hip cannot convert on the way, so this is the register-staged schedule of
// sense_mix.hip (staged_tile.h): one workgroup = 8 waves = 256 queries x 256 output columns of one sample, senses
// outermost, 32-key steps inside, S^T = K Q^T, P^T = exp2(S^T c - lse) with the causal zeroing on the diagonal block,
// O^T += C^T P^T with C^T read by ds_read_b64_tr_b16; K and C tiles double-buffered in LDS and fetched one step ahead.
// The scale does not fit the scaled MFMA forms (it belongs to (row, 32 COLUMNS) and so varies along the contraction
// index, the keys), hence the bytes are widened to the 16-bit type and the 16-bit MFMA runs as in the other mix kernels.
//
// What differs from sense_mix.hip is the content side of a step:
//   * a 32-key x 256-column tile is 8 KB of E4M3: thread (key = tid / 16, half = tid % 16) issues ONE 16-byte load (16
//     columns, half a scale block) and one byte load of its block's scale.  The two lanes of a block ask for the same
//     byte and the 16 lanes of a key for 8 consecutive bytes, so a wave's scale load touches the four 8-byte runs of
//     its four keys: one request per run in the cache, no exchange between lanes, no LDS;
//   * the row comes from row_index[b, key], clamped unsigned to table_rows - 1.  It depends on the key step alone; the
//     index of step + 2 is loaded while step + 1 is fetched, so no fetch waits for an index load it issued itself;
//   * row offsets are 64-bit: no limit on the table's size;
//   * at stash time the 16 bytes become two 16-byte chunks of 16-bit values (mx8_widen16: the dequantiser's own
//     instruction sequence, hence its bits) written into the v_lds_off<8> image the MFMA reader expects.  Lanes 0..7
//     of a key write their even chunk first, lanes 8..15 their odd one: the 16 lanes then cover 16 different 16-byte
//     bank groups in either write instead of 8 groups twice.
// Keys at or past the sequence end and columns at or past d_out are zero bytes under scale 127 (= +0.0): a masked key
// contributes exactly 0 and never a NaN.  No atomics, fp32 accumulation, one fixed order: two calls give the same bits.
#include "bp_common.h"
#include "bp_kernels.h"
#include "mx8_block.h"
#include "staged_tile.h"

namespace bp {

template <int KD>
struct MixMx8Cfg {
    static constexpr int BM = 256;             // queries per workgroup
    static constexpr int BK = 32;              // keys per step
    static constexpr int NB = 8;               // 32-column blocks per workgroup
    static constexpr int BNC = NB * 32;        // output columns per workgroup
    static constexpr int NT = 512;
    static constexpr int KTILE = BK * k_pitch(KD);
    static constexpr int CTILE = BK * NB * 64; // the 16-bit image: XOR-swizzled 64-byte chunks
    static constexpr int STAGE = KTILE + CTILE;
    static constexpr int K_ITERS = tile_iters(BK, KD * 2, NT);   // 1
    static_assert(BK * (BNC / 16) == NT, "one 16-byte E4M3 load per thread and step");
};

template <class ET, int KD>
__global__ __launch_bounds__(512) void sense_mix_gather_mx8_kernel(const MixMx8Params pp) {
    using C = MixMx8Cfg<KD>;
    using E = Elem<ET>;
    __shared__ __attribute__((aligned(16))) char smem[2 * C::STAGE];
    const MixParams &p = pp.m;

    const LaneCoord L = lane_coord();
    const int l31 = L.l31, hh = L.hh;

    int grp, slot;
    if (!xcd_map(blockIdx.x, p.b * p.n_chunks, p.n_qtiles, grp, slot)) return;
    const int qt = p.n_qtiles - 1 - slot;
    const int batch = grp / p.n_chunks;
    const int chunk = grp - batch * p.n_chunks;
    const int col_base = chunk * C::BNC;
    const int S = p.s;

    const uint16_t *qg = reinterpret_cast<const uint16_t *>(p.q) + batch * p.qk_bs;
    const uint16_t *kg = reinterpret_cast<const uint16_t *>(p.k) + batch * p.qk_bs;
    const uint8_t *q8 = reinterpret_cast<const uint8_t *>(p.c);
    const int32_t *idx_row = p.row_index + batch * p.idx_bs;

    const int k_end = min(S, qt * C::BM + C::BM);
    const int nkb = (k_end + C::BK - 1) / C::BK;
    const int nsteps = p.nsenses * nkb;

    const QueryRows R = query_rows(L, qt * C::BM, S);
    const int q0 = R.q0, my_q = R.my_q;
    const bool wave_has_rows = R.wave_has_rows;
    const int my_last_kb = q0 / C::BK;   // diagonal block of this wave (q0 is a multiple of 32)
    const float c2 = p.scale_log2e;
    const int nb_live = min(C::NB, (p.dout - col_base + 31) / 32);   // column blocks of this chunk (wave-uniform)

    // content side: my key of a step, my 16 columns
    const int c_row = L.tid >> 4, c_half = L.tid & 15;
    const int c_col = col_base + c_half * 16;
    const bool col_live = c_col < p.dout;        // d_out % 32 == 0: my 16 columns are inside the row or outside it
    const int first = c_half >> 3;               // which of my two chunks goes to LDS first
    // (sense, key block) of a step -> those of the next one: counted, not divided
    auto advance = [&](int &l, int &kb) {
        if (++kb == nkb) { kb = 0; ++l; }
    };
    // table row of my key of block kb of sense l; 0 where nothing will be fetched
    auto load_row = [&](int l, int kb) -> uint32_t {
        const int key = kb * C::BK + c_row;
        if (l >= p.nsenses || key >= S || !col_live) return 0u;
        return min((uint32_t)idx_row[key], p.last_table_row);
    };

    constexpr std::integral_constant<int, KD> kd;
    u32x4 kreg[C::K_ITERS];
    u32x4 creg;
    int cexp = 0;                                // my block's scale byte - 127
    auto fetch = [&](int l, int kb, uint32_t trow) {
        k_fetch<true, C::BK, C::NT>(kreg, kg + (int64_t)l * p.qk_ss, p.qk_rs, kb * C::BK, S, p.dk, kd, L.tid);
        creg = u32x4{0u, 0u, 0u, 0u};
        cexp = 0;
        if (kb * C::BK + c_row < S && col_live) {
            creg = *reinterpret_cast<const u32x4 *>(q8 + (int64_t)trow * p.c_rs + (int64_t)l * p.c_ss + c_col);
            cexp = (int)pp.scale8[(int64_t)trow * pp.s_rs + (int64_t)l * pp.s_ss + (c_col >> 5)] - 127;
        }
    };
    auto stash = [&](int buf) {
        char *kb_ = smem + buf * C::STAGE;
        k_stash<C::BK, C::NT>(kreg, kb_, kd, L.tid);
        u32x4 w[2];
        mx8_widen16<E>(creg, cexp, w[0], w[1]);
        char *cb = kb_ + C::KTILE;
        lds_write_16B(cb, v_lds_off<C::NB>(c_row, 2 * c_half + first), first ? w[1] : w[0]);
        lds_write_16B(cb, v_lds_off<C::NB>(c_row, 2 * c_half + (first ^ 1)), first ? w[0] : w[1]);
    };

    f32x16 acc[C::NB];
#pragma unroll
    for (int n = 0; n < C::NB; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;

    const int k_lane = k_lane_off(KD, l31, hh);
    const TrLane tr = tr_lane(L);

    u32x4 qf[KD];
    float lse2 = 0.f;

    int l = 0, kb = 0;          // this step
    int l1 = 0, kb1 = 0;        // the next one: fetched now
    int l2 = 0, kb2 = 0;        // the one behind it: its row index is loaded now
    fetch(0, 0, load_row(0, 0));
    advance(l1, kb1);
    advance(l2, kb2);
    advance(l2, kb2);
    uint32_t row_next = load_row(l1, kb1);
    stash(0);
    __syncthreads();
    for (int step = 0; step < nsteps; ++step, advance(l, kb), advance(l1, kb1), advance(l2, kb2)) {
        const int cur = step & 1;
        if (step + 1 < nsteps) {
            fetch(l1, kb1, row_next);
            row_next = load_row(l2, kb2);
        }
        if (kb == 0 && wave_has_rows) {
            // new sense: my query's fragments and its log-sum-exp
            load_q_frags<true>(qf, qg + (int64_t)l * p.qk_ss, p.qk_rs, my_q, S, p.dk, hh);
            const float lse = (my_q < S) ? p.lse[((int64_t)batch * p.nsenses + l) * p.lse_stride + my_q] : 0.f;
            lse2 = lse * kLog2e;
        }
        if (wave_has_rows && kb <= my_last_kb) {
            const char *kbuf = smem + cur * C::STAGE;
            const char *cbuf = kbuf + C::KTILE;
            f32x16 st = st_half<ET>(kbuf, qf, k_lane, 0);
            settle_acc(st);   // wait for the matrix pipe in this block (bp_common.h)
            const bool diag = (kb == my_last_kb);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float e = fast_exp2(fmaf(st[r], c2, -lse2));
                if (diag && st_key(kb * C::BK, r, hh) > my_q) e = 0.f;
                st[r] = e;
            }
            accumulate_pv<ET>(acc, st, cbuf, 0, tr, nb_live);
        }
        if (step + 1 < nsteps) stash(cur ^ 1);
        __syncthreads();
    }

    if (!wave_has_rows || my_q >= S) return;
    uint16_t *og = reinterpret_cast<uint16_t *>(p.o) + batch * p.o_bs + (int64_t)my_q * p.o_rs;
    store_acc_row<ET, true>(og, acc, col_base, p.dout, hh);
}

hipError_t launch_sense_mix_gather_mx8(const MixMx8Params &p, int dtype, hipStream_t stream) {
    const dim3 grid(xcd_grid(p.m.b * p.m.n_chunks, p.m.n_qtiles)), block(512);
    return with_dtype(dtype, [&](auto et) {
        return with_kd(p.m.dk, [&](auto kd) {
            hipLaunchKernelGGL((sense_mix_gather_mx8_kernel<decltype(et), kd>), grid, block, 0, stream, p);
            return hipGetLastError();
        });
    });
}

}  // namespace bp
