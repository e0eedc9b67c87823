// Fused Backpack sense combination for gfx950 -- alpha is never written to memory:
//
//     out[b,t,:] = sum_l sum_{s<=t} exp(scale * q_l[t].k_l[s] - lse[b,l,t]) * C[b,s,l,:]
//
// The reference does this with eager ops (training/src/models/backpack.py:116-122 softmax, :313
// `torch.sum(contextualization @ content, dim=1)`), materialising alpha (B,k,S,S) and a per-sense
// (B,k,S,d) temporary.  Here it is ONE contraction over the index (key s, sense l): because the
// per-(sense, query) log-sum-exp is known up front (a cheap LSE-only pass of the flash kernel over
// the k "heads" of width d_k), every probability is final when it is produced, so all k senses
// accumulate into the same O tile and nothing is ever rescaled.
//
// Schedule (one workgroup = 8 waves = 256 queries x 256 output columns of one sample):
//   for each sense l:   Q_l fragments + lse_l of my 32 queries -> registers
//     for each 32-key block up to the diagonal:
//       S^T = K_l Q_l^T        (KD MFMAs, d_k zero-padded to 16*KD)
//       P^T = exp2(S^T*c - lse*log2e), causal zeroing on the diagonal block, -> 16-bit in registers
//       O^T += C_l^T P^T       (16 MFMAs: 8 column blocks x 2 key halves), C^T via ds_read_b64_tr_b16
// K_l / C_l tiles are shared by the 8 waves through double-buffered LDS and fetched one step
// ahead into registers.  All query tiles of one (sample, column chunk) run on one XCD.
#include "bp_common.h"
#include "bp_kernels.h"
#include "staged_tile.h"

namespace bp {

template <int KD>
struct MixCfg {
    static constexpr int BM = 256;             // queries per workgroup
    static constexpr int BK = 32;              // keys per step
    static constexpr int NB = 8;               // 32-column blocks per workgroup
    static constexpr int BNC = NB * 32;        // output columns per workgroup
    static constexpr int NT = 512;
    static constexpr int KROW = k_pitch(KD);
    static constexpr int CROW = NB * 64;       // bytes, XOR-swizzled 64-B chunks
    static constexpr int KTILE = BK * KROW;
    static constexpr int CTILE = BK * CROW;
    static constexpr int STAGE = KTILE + CTILE;
    static constexpr int KCH = KD * 2;
    static constexpr int CCH = NB * 4;
    static constexpr int K_ITERS = tile_iters(BK, KCH, NT);   // 1
    static constexpr int C_ITERS = tile_iters(BK, CCH, NT);   // 2
};

template <class ET, int KD, bool VEC_QK, bool VEC_C>
__global__ __launch_bounds__(512) void sense_mix_kernel(const MixParams p) {
    using C = MixCfg<KD>;
    __shared__ __attribute__((aligned(16))) char smem[2 * C::STAGE];

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
    const uint16_t *cg = reinterpret_cast<const uint16_t *>(p.c) + batch * p.c_bs;

    const int k_end = min(S, qt * C::BM + C::BM);
    const int nkb = (k_end + C::BK - 1) / C::BK;
    const int nsteps = p.nsenses * nkb;

    const QueryRows R = query_rows(L, qt * C::BM, S);
    const int q0 = R.q0, my_q = R.my_q;
    const bool wave_has_rows = R.wave_has_rows;
    const int my_last_kb = q0 / C::BK;   // diagonal block of this wave (q0 is a multiple of 32)
    const float c2 = p.scale_log2e;
    // column blocks that exist in this chunk (wave-uniform)
    const int nb_live = min(C::NB, (p.dout - col_base + 31) / 32);

    constexpr std::integral_constant<int, KD> kd;
    u32x4 kreg[C::K_ITERS];
    u32x4 creg[C::C_ITERS];
    auto fetch = [&](int step) {
        const int l = step / nkb;
        const int kb = step - l * nkb;
        k_fetch<VEC_QK, C::BK, C::NT>(kreg, kg + (int64_t)l * p.qk_ss, p.qk_rs, kb * C::BK, S, p.dk, kd, L.tid);
        c_fetch<VEC_C, C::NB, C::BK, C::NT>(creg, cg + (int64_t)l * p.c_ss, p.c_rs, kb * C::BK, S, col_base, p.dout, L.tid);
    };
    auto stash = [&](int buf) {
        char *kb_ = smem + buf * C::STAGE;
        k_stash<C::BK, C::NT>(kreg, kb_, kd, L.tid);
        c_stash<C::NB, C::BK, C::NT>(creg, kb_ + C::KTILE, L.tid);
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

    fetch(0);
    stash(0);
    __syncthreads();
    for (int step = 0; step < nsteps; ++step) {
        const int cur = step & 1;
        const int l = step / nkb;
        const int kb = step - l * nkb;
        if (step + 1 < nsteps) fetch(step + 1);
        if (kb == 0 && wave_has_rows) {
            // new sense: my query's fragments and its log-sum-exp
            load_q_frags<VEC_QK>(qf, qg + (int64_t)l * p.qk_ss, p.qk_rs, my_q, S, p.dk, hh);
            const float lse = (my_q < S) ? p.lse[((int64_t)batch * p.nsenses + l) * p.lse_stride + my_q] : 0.f;
            lse2 = lse * kLog2e;
        }
        if (wave_has_rows && kb <= my_last_kb) {
            const char *kbuf = smem + cur * C::STAGE;
            const char *cbuf = kbuf + C::KTILE;
            f32x16 st = st_half<ET>(kbuf, qf, k_lane, 0);
            settle_acc(st);   // wait for the matrix pipe in this block (bp_common.h)
            const bool diag = (kb == my_last_kb);
            const float *kw = p.kw != nullptr ? p.kw + batch * p.kw_bs + (int64_t)l * p.kw_ss : nullptr;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float e = fast_exp2(fmaf(st[r], c2, -lse2));
                const int key = st_key(kb * C::BK, r, hh);
                if (diag && key > my_q) e = 0.f;
                if (kw != nullptr) e *= kw[min(key, S - 1)];   // intervention hook: alpha[:, key] scaled
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

hipError_t launch_sense_mix(const MixParams &p, int dtype, bool vec_qk, bool vec_c, hipStream_t stream) {
    const dim3 grid(xcd_grid(p.b * p.n_chunks, p.n_qtiles)), block(512);
    return with_dtype(dtype, [&](auto et) {
        return with_kd(p.dk, [&](auto kd) {
            return with_flag(vec_qk, [&](auto vq) {
                return with_flag(vec_c, [&](auto vc) {
                    hipLaunchKernelGGL((sense_mix_kernel<decltype(et), kd, vq, vc>), grid, block, 0, stream, p);
                    return hipGetLastError();
                });
            });
        });
    });
}

}  // namespace bp
