// The ragged dP^T slab product of the packed sense-mix backward (bp_sense_dp_slab_varlen) for gfx950.
//
// The backward of the sense mix needs  dP_l[t, s] = dout[t, :] . C[s, l, :],  a d_out-deep contraction (768 for Small).  The
// fixed-length path forms it slab by slab (128 queries) with one batched BLAS GEMM into a (B, S*k, 128) buffer that
// sense_dq_kernel / sense_dk_kernel read (sense_mix_bwd_kernel.h).  On a packed batch the product is ragged -- sample b
// contributes min(len_b, t0 + 128) * k rows, or none -- and no BLAS call serves it without padding the content.  Here:
//
//     dpt[cu[b]*k + r, q] = C_flat[cu[b]*k + r, :] . dout[cu[b] + t0 + q, :]      r < min(len_b, t0 + 128) * k,  q < 128
//
// C_flat is the (total * k, d_out) view of the packed content: the flat content row offset cu[b] * k is also the slab's row
// offset, so no prefix sums are needed, and the rows have the 256-byte layout the two consumers read today.
//
//   * one launch per slab covers all samples: grid (128-row tiles of min(max_seqlen, t0 + 128) * k, B); a workgroup whose
//     sample ends in front of the slab or in front of its tile returns at once;
//   * a workgroup = 4 waves = 128 content rows x 128 queries; wave (wm, wq) owns 64 x 64 of it as 2 x 2 accumulators of
//     v_mfma_f32_32x32x16.  The product is formed TRANSPOSED, D = dout_tile C_tile^T with the content row along the lanes:
//     a lane then holds runs of four consecutive queries of ITS row and stores them as 8-byte pieces (with the content as
//     the A operand every lane would store single 16-bit elements);
//   * the depth is walked in steps of 64 through two LDS stages of two row images each (RowImage<128> of lds_image.h:
//     128 rows x 128 B for the queries, the same for the content rows; 2 x 32 KB), filled by LDS-DMA (bp_dma.h) with the
//     images' swizzle on the source side; step i + 1 is requested right behind the barrier that ends the reads of step
//     i - 1, so it travels under the 16 MFMAs per wave of step i;
//   * query rows at or behind len_b belong to the next sample and must read as ZERO (0 x anything of another sample would
//     still let its NaNs through): their slots, and the slots past d_out in the last step, are cleared with plain LDS
//     stores instead of being fetched.  Content rows past the tile's last valid row are fetched from that row (this
//     sample's, finite whenever the sample is) and never stored; content columns past d_out from column 0, where they
//     meet the cleared query slots.
// fp32 accumulation over the whole depth, one rounding to 16 bits.  No atomics, every element has one owner.
#include "bp_common.h"
#include "bp_dma.h"
#include "bp_kernels.h"

namespace bp {

struct DpSlabCfg {
    static constexpr int NT = 256, NWAVE = 4;
    static constexpr int TM = 128, TQ = 128, BKC = 64;    // content rows, queries, depth step
    static constexpr int ROW = BKC * 2;                   // bytes per image row
    static constexpr int IMG = TM * ROW;                  // 16 KB: one operand of one step
    static constexpr int STAGE = 2 * IMG;                 // queries | content rows
    static constexpr int PIECES = IMG / 1024 / NWAVE;     // 1-KB DMA pieces per wave, image and step
    static constexpr int LDS_BYTES = 2 * STAGE;
    static_assert(TM == TQ, "one piece table serves both images");
    static_assert(LDS_BYTES <= 64 * 1024, "two workgroups per CU");
};

template <class ET>
__global__ __launch_bounds__(256) void sense_dp_slab_varlen_kernel(const DpSlabParams p) {
    using C = DpSlabCfg;
    using E = Elem<ET>;
    using Img = RowImage<C::ROW>;
    __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];

    const int batch = blockIdx.y;
    const int64_t first_row = p.cu[batch];
    const int len = p.cu[batch + 1] - (int)first_row;
    const int nrows = min(len, p.t0 + C::TQ) * p.nsenses;   // rows of the sample's slab
    const int r0 = blockIdx.x * C::TM;
    if (p.t0 >= len || r0 >= nrows) return;
    const int nq = min(C::TQ, len - p.t0);                  // queries of the slab that exist

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const int wm = wave & 1, wq = wave >> 1;
    const uint32_t lds0 = lds_base_addr(smem);

    // my DMA pieces: slot g of either image holds (row, col) = Img::src(g); the query row of the slab, the content row of the tile
    const uint16_t *dg = reinterpret_cast<const uint16_t *>(p.dout) + (first_row + p.t0) * p.do_rs;
    const uint16_t *cg = reinterpret_cast<const uint16_t *>(p.c) + (first_row * p.nsenses + r0) * p.c_rs;
    const int last_c_row = nrows - 1 - r0;
    const uint16_t *q_src[C::PIECES], *c_src[C::PIECES];
    int col[C::PIECES];
    bool q_live[C::PIECES];
#pragma unroll
    for (int j = 0; j < C::PIECES; ++j) {
        const TileSrc s = Img::src((wave * C::PIECES + j) * 64 + lane);
        col[j] = s.col;
        q_live[j] = s.row < nq;
        q_src[j] = dg + (int64_t)min(s.row, nq - 1) * p.do_rs;
        c_src[j] = cg + (int64_t)min(s.row, last_c_row) * p.c_rs;
    }
    auto issue = [&](int ks) {
        const int k0 = ks * C::BKC;
        const int stage = (ks & 1) * C::STAGE;
#pragma unroll
        for (int j = 0; j < C::PIECES; ++j) {
            const int piece = (wave * C::PIECES + j) * 1024;
            const bool in_depth = k0 + col[j] < p.dout_cols;
            if (q_live[j] && in_depth) dma16_d(q_src[j] + k0 + col[j], lds0 + stage + piece);
            else lds_write_16B(smem, stage + piece + lane * 16, u32x4{0u, 0u, 0u, 0u});
            dma16_d(c_src[j] + (in_depth ? k0 + col[j] : 0), lds0 + stage + C::IMG + piece);
        }
    };

    f32x16 acc[2][2];   // [32-query block][32-row block] of my 64 x 64
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    int read_off[C::BKC / 16];
#pragma unroll
    for (int s = 0; s < C::BKC / 16; ++s) read_off[s] = Img::read_off(l31, hh, s);

    const int nks = (p.dout_cols + C::BKC - 1) / C::BKC;
    issue(0);
    for (int ks = 0; ks < nks; ++ks) {
        wait_vmcnt<0>();
        __syncthreads();   // step ks has landed (DMA and cleared slots); everybody is done reading the other stage
        if (ks + 1 < nks) issue(ks + 1);
        const char *q_img = smem + (ks & 1) * C::STAGE + wq * 64 * C::ROW;
        const char *c_img = smem + (ks & 1) * C::STAGE + C::IMG + wm * 64 * C::ROW;
#pragma unroll
        for (int s = 0; s < C::BKC / 16; ++s) {
            u32x4 qf[2], cf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                qf[i] = lds_read_16B(q_img, read_off[s] + i * 32 * C::ROW);
                cf[i] = lds_read_16B(c_img, read_off[s] + i * 32 * C::ROW);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = E::mfma(qf[i], cf[j], acc[i][j]);
        }
    }
    // the loop's back edge lies between the last MFMAs and the packs below (bp_common.h, settle_acc)
    settle_acc(acc[1][1]);
    pin_acc(acc[0][0]);
    pin_acc(acc[0][1]);
    pin_acc(acc[1][0]);

    // register r of acc[i][j]: query wq*64 + i*32 + (r & 3) + 8 (r >> 2) + 4 hh of content row wm*64 + j*32 + l31
    uint16_t *out = reinterpret_cast<uint16_t *>(p.dpt) + (first_row * p.nsenses + r0) * C::TQ;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = wm * 64 + j * 32 + l31;
        if (r0 + row >= nrows) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const u32x2 w = {E::pack2(acc[i][j][4 * g + 0], acc[i][j][4 * g + 1]), E::pack2(acc[i][j][4 * g + 2], acc[i][j][4 * g + 3])};
                *reinterpret_cast<u32x2 *>(out + (int64_t)row * C::TQ + wq * 64 + i * 32 + 8 * g + 4 * hh) = w;
            }
    }
}

hipError_t launch_sense_dp_slab_varlen(const DpSlabParams &p, int dtype, hipStream_t stream) {
    const int visible = p.max_s < p.t0 + DpSlabCfg::TQ ? p.max_s : p.t0 + DpSlabCfg::TQ;
    const dim3 grid(((int64_t)visible * p.nsenses + DpSlabCfg::TM - 1) / DpSlabCfg::TM, p.b);
    return with_dtype(dtype, [&](auto et) {
        hipLaunchKernelGGL((sense_dp_slab_varlen_kernel<decltype(et)>), grid, dim3(DpSlabCfg::NT), 0, stream, p);
        return hipGetLastError();
    });
}

}  // namespace bp
