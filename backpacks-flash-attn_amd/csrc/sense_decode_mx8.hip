// bp_sense_decode_mx8: the decode step of the sense contraction (bp_sense_decode / bp_sense_decode_weighted) with the
// value stream -- the sense-table row of every cached position -- read from the MXFP8 twin of the table: 1 byte per
// element in q8 and one E8M0 scale byte per block of 32 columns in scale8 (include/bp_hip.h, "MXFP8 sense table").
//
// Grid, key ranges, workspace layout and the second launch (decode_combine_kernel, sense_decode.hip's code object) are
// decode_core.h's.  Per tile of 64 keys:
//   A, S  scores from the 16-bit key cache and the online softmax: a COPY of decode_split_kernel's phases (the append of
//         the new key and row index and the clamps included), not a shared device function, so that the existing
//         instantiations keep their code.
//   B     thread (c, r) owns 16 output columns c*16.. (half a scale block) and keys r, r + R, ... of the tile,
//         R = min(256 / (d_out / 16), 64): its load of a value row is still one 16-byte vector, and a row is covered by half
//         as many lanes as in the 16-bit kernel, so twice as many keys are in flight per pass.  Per key the thread fetches
//         the block's scale byte (two neighbouring threads share it), folds it into the key's probability with one
//         exponent add, p' = ldexp(p, scale - 127) -- exact, and 1 instruction per key where scaling the elements would
//         take 16 -- unpacks the 16 bytes with eight v_cvt_pk_f32_fp8 and accumulates acc += p' * e in 16 fp32 registers.
// The R key residues are summed in a fixed order through LDS, as in decode_core.h, and the partial (m, l, acc[d]) goes to
// the same workspace rows.  Keys reach threads in another order than in the 16-bit kernel (R differs), so the two kernels
// agree to rounding, not bit for bit; each is bit-identical across calls.
#include "decode_core.h"

namespace bp {

template <class ET, int G, int NQ, bool WEIGHTED>
__global__ __launch_bounds__(DEC_THREADS) void decode_split_mx8_kernel(DecodeMx8Params pp) {
    using E = Elem<ET>;
    const DecodeParams &p = pp.d;
    constexpr int KPW = 64 / G;                   // keys per wave per pass
    constexpr int KPB = 4 * KPW;                  // keys per workgroup per pass
    constexpr int NP = (DEC_TILE + KPB - 1) / KPB;
    constexpr int NARR = WEIGHTED ? 4 : 3;        // [2][64] arrays in front of the reduction block
    __shared__ __attribute__((aligned(16))) float smem[NARR * 2 * DEC_TILE + DEC_THREADS * 16];
    float *sc = smem;                             // [2][64] scores
    float *pb = smem + 2 * DEC_TILE;              // [2][64] probabilities
    int *rows = reinterpret_cast<int *>(smem + 4 * DEC_TILE);   // [2][64] table rows
    float *kw = smem + 6 * DEC_TILE;              // [2][64] key weights (weighted form)
    float *red = smem + NARR * 2 * DEC_TILE;      // [R][NC][16] final reduction

    const int split = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = dec_length(p, b);
    const int n = L + 1;
    const int chunk = (n + p.nsplit - 1) / p.nsplit;
    const int j0 = split * chunk;
    if (j0 >= n) return;                          // uniform: the combine skips this split the same way
    const int j1 = min(n, j0 + chunk);

    const uint16_t *q = static_cast<const uint16_t *>(p.q) + b * p.q_bs + g * p.q_gs;
    const uint16_t *kn = static_cast<const uint16_t *>(p.k_new) + b * p.kn_bs + g * p.kn_gs;
    uint16_t *kc = static_cast<uint16_t *>(p.k_cache) + b * p.kc_bs + g * p.kc_gs;
    const int qc = p.dk >> 3;                     // 8-element chunks of a key
    const int li = lane & (G - 1);

    float qf[NQ][8];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int c = li + i * G;
        u32x4 w = c < qc ? ld_global_16B(q + c * 8) : u32x4{0u, 0u, 0u, 0u};
        unpack8<E>(w, qf[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[i][e] *= p.scale_log2e;
    }

    const int nc = p.dv >> 4;                     // 16-column chunks of a value row
    const int R = min(DEC_THREADS / nc, DEC_TILE);
    const int vc = tid % nc, vr = tid / nc;
    const bool v_active = vr < R;
    const uint8_t *q8 = static_cast<const uint8_t *>(p.v) + g * p.vc_gs + vc * 16;
    const uint8_t *s8 = pp.scale8 + g * pp.s_gs + (vc >> 1);
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    for (int jt = j0, buf = 0; jt < j1; jt += DEC_TILE, buf ^= 1) {
        const int tl = min(DEC_TILE, j1 - jt);
        // ---- A: scores of the tile's keys ----
        u32x4 kv[NP][NQ];
#pragma unroll
        for (int ps = 0; ps < NP; ++ps) {
            const int jj = ps * KPB + wave * KPW + lane / G;
            const int j = jt + jj;
            const bool valid = jj < tl;
            const uint16_t *krow = (j == L) ? kn : kc + (int64_t)j * p.kc_rs;
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                const int c = li + i * G;
                kv[ps][i] = (valid && c < qc) ? ld_global_16B(krow + c * 8) : u32x4{0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (int ps = 0; ps < NP; ++ps) {
            const int jj = ps * KPB + wave * KPW + lane / G;
            const int j = jt + jj;
            const bool valid = jj < tl;
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                float kf[8];
                unpack8<E>(kv[ps][i], kf);
#pragma unroll
                for (int e = 0; e < 8; ++e) d = fmaf(qf[i][e], kf[e], d);
            }
#pragma unroll
            for (int off = G / 2; off > 0; off >>= 1) d += __shfl_xor(d, off);
            if (valid && j == L) {                // append the new key: this workgroup alone covers position L
#pragma unroll
                for (int i = 0; i < NQ; ++i) {
                    const int c = li + i * G;
                    if (c < qc) *reinterpret_cast<u32x4 *>(kc + (int64_t)L * p.kc_rs + c * 8) = kv[ps][i];
                }
            }
            if (valid && li == 0) {
                sc[buf * DEC_TILE + jj] = d;
                int row;
                if (j == L) {
                    row = p.new_row[b];
                    if (g == 0) p.row_index[b * p.ri_bs + L] = row;
                } else {
                    row = p.row_index[b * p.ri_bs + j];
                }
                const uint32_t ur = (uint32_t)row;   // clamp as unsigned: a bad index reads the last row
                rows[buf * DEC_TILE + jj] = (int)(ur < (uint32_t)p.table_rows ? ur : (uint32_t)(p.table_rows - 1));
                if constexpr (WEIGHTED) kw[buf * DEC_TILE + jj] = p.key_weight[b * p.kw_bs + g * p.kw_gs + j];
            }
        }
        __syncthreads();
        // ---- S: online softmax, the same reduction in every wave ----
        const float x = lane < tl ? sc[buf * DEC_TILE + lane] : -INFINITY;
        float tmax = x;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, off));
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = m_run == -INFINITY ? 0.f : exp2f(m_run - m_new);
        const float pl = lane < tl ? exp2f(x - m_new) : 0.f;
        float ls = pl;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) ls += __shfl_xor(ls, off);
        l_run = l_run * alpha + ls;
        m_run = m_new;
        if (wave == 0) pb[buf * DEC_TILE + lane] = pl;
        __syncthreads();
        // ---- B: acc = alpha * acc + sum_j (p_j 2^(scale_j - 127)) e4m3_j ----
        if (v_active) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] *= alpha;
            for (int jj0 = vr; jj0 < tl; jj0 += 4 * R) {
                u32x4 w[4];
                float pj[4];
                int sb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int jj = jj0 + u * R;
                    pj[u] = 0.f;
                    sb[u] = 127;
                    w[u] = u32x4{0u, 0u, 0u, 0u};
                    if (jj < tl) {
                        const int64_t row = rows[buf * DEC_TILE + jj];
                        pj[u] = pb[buf * DEC_TILE + jj];
                        if constexpr (WEIGHTED) pj[u] *= kw[buf * DEC_TILE + jj];
                        w[u] = *reinterpret_cast<const u32x4 *>(q8 + row * p.vc_rs);
                        sb[u] = s8[row * pp.s_rs];
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float ps = ldexpf(pj[u], sb[u] - 127);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint32_t wi = w[u][i];  // by value: see as_f32
                        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)wi, false);
                        const f32x2 up = __builtin_amdgcn_cvt_pk_f32_fp8((int)wi, true);
                        acc[4 * i] = fmaf(ps, lo[0], acc[4 * i]);
                        acc[4 * i + 1] = fmaf(ps, lo[1], acc[4 * i + 1]);
                        acc[4 * i + 2] = fmaf(ps, up[0], acc[4 * i + 2]);
                        acc[4 * i + 3] = fmaf(ps, up[1], acc[4 * i + 3]);
                    }
                }
            }
        }
    }
    // ---- reduce the R key residues of every column chunk (fixed order) and leave the partial ----
    if (v_active) {
        f32x4 *dst = reinterpret_cast<f32x4 *>(red + (vr * nc + vc) * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[i] = f32x4{acc[4 * i], acc[4 * i + 1], acc[4 * i + 2], acc[4 * i + 3]};
    }
    __syncthreads();
    const int64_t prow = ((int64_t)b * p.groups + g) * p.nsplit + split;
    if (tid < nc) {
        f32x4 s[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < R; ++r) {
            const f32x4 *src = reinterpret_cast<const f32x4 *>(red + (r * nc + tid) * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) s[i] += src[i];
        }
        f32x4 *out = reinterpret_cast<f32x4 *>(p.ws_acc + prow * p.dv + tid * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = s[i];
    }
    if (tid == 0) *reinterpret_cast<f32x2 *>(p.ws_ml + prow * 2) = f32x2{m_run, l_run};
}

template <bool WEIGHTED>
static hipError_t launch_split_mx8(const DecodeMx8Params &p, int dtype, hipStream_t stream) {
    // the senses' width buckets, as launch_decode
    return with_dtype(dtype, [&](auto et) {
        return with_bound<1, 2, 4, 8, 16, 32, 64, 128>(p.d.dk >> 3, hipErrorNotSupported, [&](auto qc) {
            constexpr int G = qc < 64 ? int(qc) : 64;
            hipLaunchKernelGGL((decode_split_mx8_kernel<decltype(et), G, qc / G, WEIGHTED>),
                               dim3(p.d.nsplit, p.d.groups, p.d.b), dim3(DEC_THREADS), 0, stream, p);
            return hipGetLastError();
        });
    });
}

hipError_t launch_sense_decode_mx8(const DecodeMx8Params &p, int dtype, hipStream_t stream) {
    const hipError_t e = p.d.key_weight != nullptr ? launch_split_mx8<true>(p, dtype, stream)
                                                   : launch_split_mx8<false>(p, dtype, stream);
    return e != hipSuccess ? e : launch_sense_decode_combine(p.d, dtype, stream);
}

}  // namespace bp
