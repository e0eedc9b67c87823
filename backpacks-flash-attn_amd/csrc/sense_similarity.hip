// bp_sense_similarity: the cosine measures of sense vectors (lexical similarity: the reference's training/src/run_simlex.py:189-271
// and the neighbour lists of training/src/visualize_sim.py:197-222) of nq query words against ncand candidate words of the
// per-token sense table, in ONE pass over the candidates' rows.  For query n and candidate c, r = row(c):
//   g[l', l] = sum_e query[n, l', e] * table[r, l, e]      A[l'] = sum_e query[n, l', e]^2      B[l] = sum_e table[r, l, e]^2
//   cos[l', l] = g[l', l] / (sqrtf(A[l']) * sqrtf(B[l]))
//   per_sense[n, l, c] = cos[l, l];  min_pair / max_pair over the diagonal;  min_all / max_all over all (l', l)
//   flat[n, c] = (sum_l g[l, l]) / (sqrtf(sum_l' A[l']) * sqrtf(sum_l B[l])), the three sums ascending in l
// A measure whose cosines hold a NaN (a zero vector: 0 / 0) is NaN.  Contract in include/bp_hip.h; restated by
// _eager_sense_similarity (src/utils/sense_similarity.py) and by tests/sense_similarity_ref.py.
//
// Algorithmic bytes: ncand * k * d * 2 of table rows, read ONCE whatever nq is, plus 4 * nq * ncand per (nq, ncand) output and
// 4 * nq * k * ncand for per_sense; the nq * k * d * 2 bytes of the queries are re-read per workgroup and stay in L2.
//
// Schedule.  The candidates are flattened to rows (c, l), the queries to rows (n, l'); nq * k <= 64 query rows
// (BP_SIMILARITY_MAX_QUERY_ROWS).  A 256-thread workgroup takes 256 consecutive table rows, a wave 64 of them as TWO row tiles
// on the N side of v_mfma_f32_32x32x16: lane (l31, hh) owns table row l31 of a tile and K elements 16 s + 8 hh .. + 7 of step
// s -- its 16-byte global load IS the operand fragment, and the same registers give the row's squared norm on the VALU
// (v_dot2, then one exchange with lane ^ 32).  The query rows are the M side: one or two tiles of 32 (NQT), staged through
// LDS in chunks of 256 columns (rows padded by 16 bytes against bank conflicts) by all four waves, which also sum the query
// rows' squared norms on the way.  Accumulators: NQT x 2 tiles x 16 registers.  A sense count is a power of two (1 .. 64), so
// a candidate's k rows lie inside one wave's 64 -- for k = 64 they are the wave's two tiles.
// Epilogue: the wave parks its (query rows, 64) block of dots in LDS (over the query chunk, behind a barrier), then lane i
// owns table row i of the 64: it walks l' in order (scale by the norms, min / max and a NaN flag in its registers), and the
// reduction over l runs across the k lanes of the candidate (xor exchanges for min / max, a serial walk in ascending l for
// the sums of `flat`).  Rows past ncand * k are computed on zeros and not stored.
// No workspace, no atomics, vector stores only; every loop is bounded by d, k, nq or a constant; two calls agree bit for bit.
#include "bp_common.h"
#include "bp_kernels.h"

namespace bp {

namespace {

constexpr int SS_THREADS = 256;
constexpr int SS_WAVES = SS_THREADS / 64;
constexpr int SS_ROWS = 64;                  // table rows of a wave: two row tiles
constexpr int SS_PIECES = 32;                // 16-byte pieces of a query row per LDS chunk: 256 columns, 16 K steps
constexpr int SS_QS = SS_PIECES * 16 + 16;   // bytes of a query row in LDS
constexpr int SS_BATCH = 4;                  // K steps whose table fragments are in flight together: 8 loads a lane
static_assert(kSimilarityMaxQueryRows == 64, "the launcher instantiates one or two query row tiles of 32");

// c + lo^2 + hi^2 of a packed pair in one VALU instruction (v_dot2_f32_{bf16,f16}); the products are exact in fp32
template <class ET> struct SqPair;
template <> struct SqPair<BF16> {
    static BP_DEV float add(uint32_t w, float c) {
        const bf16x2 v = __builtin_bit_cast(bf16x2, w);
        return __builtin_amdgcn_fdot2_f32_bf16(v, v, c, false);
    }
};
template <> struct SqPair<F16> {
    static BP_DEV float add(uint32_t w, float c) {
        const f16x2 v = __builtin_bit_cast(f16x2, w);
        return __builtin_amdgcn_fdot2(v, v, c, false);
    }
};

template <class ET> BP_DEV float sq_sum(const u32x4 &w, float c) {
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];   // by-value copies (bp_common.h, as_f32)
    c = SqPair<ET>::add(w0, c);
    c = SqPair<ET>::add(w1, c);
    c = SqPair<ET>::add(w2, c);
    return SqPair<ET>::add(w3, c);
}

BP_DEV u32x4 keep_if(bool ok, const u32x4 &w) {
    return u32x4{ok ? w[0] : 0u, ok ? w[1] : 0u, ok ? w[2] : 0u, ok ? w[3] : 0u};
}

}  // namespace

template <class ET, int NQT>          // NQT: query row tiles of 32, ceil(nq * k / 32)
__global__ __launch_bounds__(SS_THREADS) void sense_similarity_kernel(const SimilarityParams p) {
    using E = Elem<ET>;
    constexpr int QROWS = 32 * NQT;
    constexpr int Q_BYTES = QROWS * SS_QS, G_BYTES = SS_WAVES * QROWS * SS_ROWS * 4;
    __shared__ __attribute__((aligned(16))) char smem[G_BYTES > Q_BYTES ? G_BYTES : Q_BYTES];
    __shared__ float q_n2[QROWS], q_sq[QROWS], q_fs[QROWS], row_b[SS_WAVES][SS_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
    const int k = p.groups, logk = p.logk, qr = p.nq * k, nc = p.d >> 3;
    const int64_t total = (int64_t)p.ncand << logk;
    const int64_t wave_row0 = ((int64_t)blockIdx.x * SS_WAVES + wave) * SS_ROWS;

    // the lane's table row of either tile; a row past the end points at row 0 and is read as zeros
    const uint16_t *trow[2];
    bool live[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t fr = wave_row0 + 32 * j + l31;
        live[j] = fr < total;
        const int64_t c = live[j] ? fr >> logk : 0;
        const int l = live[j] ? (int)(fr & (k - 1)) : 0;
        int64_t r = c;
        if (p.cand_index != nullptr) {
            const uint32_t ur = (uint32_t)p.cand_index[c];             // clamp as unsigned: a bad index reads the last row
            r = ur < (uint32_t)p.table_rows ? ur : (uint32_t)(p.table_rows - 1);
        }
        trow[j] = static_cast<const uint16_t *>(p.table) + r * p.t_rs + l * p.t_gs;
    }
    // the query row this thread helps to stage: TPR threads a row, pieces qsub, qsub + TPR, ... of every chunk
    constexpr int TPR = SS_THREADS / QROWS, PPT = SS_PIECES / TPR;
    const int qrow = tid / TPR, qsub = tid % TPR;
    const bool qlive = qrow < qr;
    const uint16_t *qptr = static_cast<const uint16_t *>(p.query)
                           + (qlive ? (int64_t)(qrow >> logk) * p.q_qs + (int64_t)(qrow & (k - 1)) * p.q_gs : 0);

    f32x16 acc[NQT][2];
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[qt][j][r] = 0.f;
    float bsq[2] = {0.f, 0.f}, asq = 0.f;

    for (int c0 = 0; c0 < nc; c0 += SS_PIECES) {
        __syncthreads();                                               // the previous chunk has been read
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int piece = qsub + i * TPR;
            const bool ok = qlive && c0 + piece < nc;
            const u32x4 w = keep_if(ok, ld_global_16B(qptr + (ok ? (c0 + piece) * 8 : 0)));
            asq = sq_sum<ET>(w, asq);
            lds_write_16B(smem, qrow * SS_QS + piece * 16, w);
        }
        __syncthreads();
        const int steps = nc - c0 >= SS_PIECES ? SS_PIECES / 2 : (nc - c0 + 1) >> 1;
        for (int s0 = 0; s0 < steps; s0 += SS_BATCH) {
            u32x4 tf[SS_BATCH][2];
#pragma unroll
            for (int i = 0; i < SS_BATCH; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int piece = c0 + 2 * (s0 + i) + hh;
                    const bool ok = live[j] && piece < nc;
                    tf[i][j] = keep_if(ok, ld_global_16B(trow[j] + (ok ? piece * 8 : 0)));
                }
#pragma unroll
            for (int i = 0; i < SS_BATCH; ++i) {
#pragma unroll
                for (int j = 0; j < 2; ++j) bsq[j] = sq_sum<ET>(tf[i][j], bsq[j]);
#pragma unroll
                for (int qt = 0; qt < NQT; ++qt) {
                    const u32x4 a = lds_read_16B(smem, (32 * qt + l31) * SS_QS + (2 * (s0 + i) + hh) * 16);
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[qt][j] = E::mfma(a, tf[i][j], acc[qt][j]);
                }
            }
        }
    }
    settle_acc(acc[NQT - 1][1]);   // the loops' exit branches separate the last MFMAs from their readers (bp_common.h)
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (qt != NQT - 1 || j != 1) pin_acc(acc[qt][j]);

    // squared norms: a table row's two halves; a query row's TPR partial sums (neighbouring lanes)
    const float bn0 = xhalf_sum(bsq[0]), bn1 = xhalf_sum(bsq[1]);
#pragma unroll
    for (int off = 1; off < TPR; off <<= 1) asq += __shfl_xor(asq, off);
    if (qsub == 0) q_n2[qrow] = asq;
    __syncthreads();                                                   // every wave has read its last query chunk

    // the wave's dots as (query row, table row) in LDS: register r of a lane is query row (r & 3) + 8 (r >> 2) + 4 hh
    float *g = reinterpret_cast<float *>(smem) + wave * (QROWS * SS_ROWS);
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                g[(32 * qt + (r & 3) + 8 * (r >> 2) + 4 * hh) * SS_ROWS + 32 * j + l31] = acc[qt][j][r];
    row_b[wave][32 * hh + l31] = hh == 0 ? bn0 : bn1;
    if (tid < qr) q_sq[tid] = sqrtf(q_n2[tid]);
    if (tid < p.nq) {
        float s = 0.f;
        for (int l = 0; l < k; ++l) s += q_n2[tid * k + l];
        q_fs[tid] = sqrtf(s);
    }
    __syncthreads();

    // lane i owns table row i of the wave's 64: sense l of candidate c, whose k rows are lanes gbase .. gbase + k - 1
    const int64_t fr = wave_row0 + lane;
    const bool valid = fr < total;
    const int64_t c = fr >> logk;
    const int l = (int)(fr & (k - 1)), gbase = lane & ~(k - 1);
    const float bn = row_b[wave][lane];
    const float sb = sqrtf(bn);
    float sum_b = 0.f;
    for (int i = 0; i < k; ++i) sum_b += __shfl(bn, gbase + i);
    const float sfb = sqrtf(sum_b);
    const float inf = __builtin_inff(), nan = as_f32(0x7fc00000u);

    for (int n = 0; n < p.nq; ++n) {
        float amin = inf, amax = -inf, dcos = 0.f, dg = 0.f;
        int abad = 0;
        for (int lq = 0; lq < k; ++lq) {
            const int m = n * k + lq;
            const float gv = g[m * SS_ROWS + lane];
            const float cs = gv / (q_sq[m] * sb);
            abad |= cs != cs ? 1 : 0;
            amin = fminf(amin, cs);
            amax = fmaxf(amax, cs);
            if (lq == l) { dcos = cs; dg = gv; }
        }
        int pbad = dcos != dcos ? 1 : 0;
        float pmin = pbad ? inf : dcos, pmax = pbad ? -inf : dcos;
        for (int off = 1; off < k; off <<= 1) {
            amin = fminf(amin, __shfl_xor(amin, off));
            amax = fmaxf(amax, __shfl_xor(amax, off));
            pmin = fminf(pmin, __shfl_xor(pmin, off));
            pmax = fmaxf(pmax, __shfl_xor(pmax, off));
            abad |= __shfl_xor(abad, off);
            pbad |= __shfl_xor(pbad, off);
        }
        float num = 0.f;
        for (int i = 0; i < k; ++i) num += __shfl(dg, gbase + i);
        const float fl = num / (q_fs[n] * sfb);
        if (valid) {
            if (p.per_sense != nullptr) p.per_sense[n * p.ps_qs + l * p.ps_gs + c] = dcos;
            if (l == 0) {
                const int64_t at = n * p.o_qs + c;
                if (p.flat != nullptr) p.flat[at] = fl;
                if (p.min_pair != nullptr) p.min_pair[at] = pbad ? nan : pmin;
                if (p.max_pair != nullptr) p.max_pair[at] = pbad ? nan : pmax;
                if (p.min_all != nullptr) p.min_all[at] = abad ? nan : amin;
                if (p.max_all != nullptr) p.max_all[at] = abad ? nan : amax;
            }
        }
    }
}

hipError_t launch_sense_similarity(const SimilarityParams &p, int dtype, hipStream_t stream) {
    const int64_t rows = (int64_t)p.ncand * p.groups;
    const int64_t blocks = (rows + SS_WAVES * SS_ROWS - 1) / (SS_WAVES * SS_ROWS);
    return with_dtype(dtype, [&](auto et) {
        return with_bound<1, 2>((p.nq * p.groups + 31) / 32, hipErrorNotSupported, [&](auto nqt) {
            hipLaunchKernelGGL((sense_similarity_kernel<decltype(et), nqt>), dim3((unsigned)blocks), dim3(SS_THREADS), 0,
                               stream, p);
            return hipGetLastError();
        });
    });
}

}  // namespace bp
