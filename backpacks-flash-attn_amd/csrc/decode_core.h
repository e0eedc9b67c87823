// Single-query decode against a cache: the shared body of bp_flash_decode (csrc/flash_decode.hip) and bp_sense_decode
// (csrc/sense_decode.hip).
//
// One output row attends to keys j = 0 .. L of its cache, L = cache_seqlens[b] (read on the device, so a captured graph
// serves every step); key L is the NEW one, taken from the k_new operand (and, for the trunk, v_new) and appended to the
// cache by the one workgroup whose key range holds it -- no workgroup reads cache row L, so the append is race-free.
//
// Split-KV: grid (nsplit, groups, batch).  Split s of (b, g) takes keys [s*chunk, min(n, (s+1)*chunk)), n = L + 1,
// chunk = ceil(n / nsplit), and leaves its partial (m, l, acc[d]) in an fp32 workspace; decode_combine_kernel merges the
// partials of a row in split order (and, for the senses, sums the senses): deterministic, no atomics.  Memory-bound
// GEMV-shaped work (cdna_hip_programming.md, "Attention decode"): keys and value rows go straight to VGPRs with 16-byte
// loads, LDS only carries 64 scores / probabilities per tile and the final cross-thread reduction.
//
// Per tile of 64 keys:
//   A  scores: G lanes per key (G = 8-element chunks of d_k rounded up to a power of two), q pre-scaled by
//      scale * log2(e) in registers, reduction by lane exchanges inside the group; the 64 scores go to LDS.
//   S  online softmax: every wave reduces the same 64 scores the same way (identical m, l in every wave); wave 0 stores
//      the probabilities.
//   B  values: thread (c, r) owns 8 output columns c*8.. and keys r, r + R, ... of the tile (R = 256 / (d / 8)).
//      Trunk: value row = V cache row j of head g; senses: value row = table[row_index[b, j], g, :].
#pragma once
#include "bp_common.h"
#include "bp_kernels.h"

namespace bp {

constexpr int DEC_THREADS = 256;
constexpr int DEC_TILE = 64;

template <class E> BP_DEV void unpack8(u32x4 w, float (&f)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = E::lo_f32(w[i]);
        f[2 * i + 1] = E::hi_f32(w[i]);
    }
}

BP_DEV int dec_length(const DecodeParams &p, int b) {
    const int L = p.seqlens[b];
    return L < 0 ? 0 : (L >= p.max_seqlen ? p.max_seqlen - 1 : L);   // never index outside the cache
}

// Weighted form (senses only, bp_sense_decode_weighted): decode_split_kernel<Weighted<ET>, G, NQ, true> multiplies the
// probability of key j by key_weight[b, g, j] in phase B; the weight never enters the softmax (m and l are the plain
// kernel's).  The flag rides on the element tag, so the plain instantiations keep their names and their code.
template <class ET> struct Weighted {};
template <class T> struct DecodeTag { using elem = T; static constexpr bool weighted = false; };
template <class T> struct DecodeTag<Weighted<T>> { using elem = T; static constexpr bool weighted = true; };

template <class ET, int G, int NQ, bool SENSE>
__global__ __launch_bounds__(DEC_THREADS) void decode_split_kernel(DecodeParams p) {
    constexpr bool WEIGHTED = DecodeTag<ET>::weighted;
    static_assert(SENSE || !WEIGHTED, "key weights belong to the sense contraction");
    using E = Elem<typename DecodeTag<ET>::elem>;
    constexpr int KPW = 64 / G;                   // keys per wave per pass
    constexpr int KPB = 4 * KPW;                  // keys per workgroup per pass
    constexpr int NP = (DEC_TILE + KPB - 1) / KPB;
    constexpr int NARR = WEIGHTED ? 4 : 3;        // [2][64] arrays in front of the reduction block
    __shared__ __attribute__((aligned(16))) float smem[NARR * 2 * DEC_TILE + DEC_THREADS * 8];
    float *sc = smem;                             // [2][64] scores
    float *pb = smem + 2 * DEC_TILE;              // [2][64] probabilities
    int *rows = reinterpret_cast<int *>(smem + 4 * DEC_TILE);   // [2][64] table rows (senses)
    float *kw = smem + 6 * DEC_TILE;              // [2][64] key weights (weighted form)
    float *red = smem + NARR * 2 * DEC_TILE;      // [R][NC][8] final reduction

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

    const int nc = p.dv >> 3;                     // 8-column chunks of a value row
    const int R = DEC_THREADS / nc;
    const int vc = tid % nc, vr = tid / nc;
    const bool v_active = vr < R;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
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
                if constexpr (SENSE) {
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
        // ---- B: acc = alpha * acc + sum_j p_j * value_j ----
        if (v_active) {
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] *= alpha;
            for (int jj0 = vr; jj0 < tl; jj0 += 4 * R) {
                u32x4 w[4];
                float pj[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int jj = jj0 + u * R;
                    pj[u] = 0.f;
                    w[u] = u32x4{0u, 0u, 0u, 0u};
                    if (jj < tl) {
                        const int j = jt + jj;
                        pj[u] = pb[buf * DEC_TILE + jj];
                        if constexpr (WEIGHTED) pj[u] *= kw[buf * DEC_TILE + jj];
                        const uint16_t *vrow;
                        if constexpr (SENSE) {
                            vrow = static_cast<const uint16_t *>(p.v) + (int64_t)rows[buf * DEC_TILE + jj] * p.vc_rs
                                   + g * p.vc_gs;
                        } else {
                            vrow = (j == L) ? static_cast<const uint16_t *>(p.v_new) + b * p.vn_bs + g * p.vn_gs
                                            : static_cast<const uint16_t *>(p.v) + b * p.vc_bs + (int64_t)j * p.vc_rs
                                                  + g * p.vc_gs;
                        }
                        w[u] = ld_global_16B(vrow + vc * 8);
                        if constexpr (!SENSE) {
                            if (j == L) {     // append the new value row (only this thread holds chunk vc of key L)
                                uint16_t *dst = static_cast<uint16_t *>(p.v) + b * p.vc_bs
                                                + (int64_t)L * p.vc_rs + g * p.vc_gs + vc * 8;
                                *reinterpret_cast<u32x4 *>(dst) = w[u];
                            }
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float vf[8];
                    unpack8<E>(w[u], vf);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj[u], vf[e], acc[e]);
                }
            }
        }
    }
    // ---- reduce the R key residues of every column chunk (fixed order) and leave the partial ----
    if (v_active) {
        f32x4 *dst = reinterpret_cast<f32x4 *>(red + (vr * nc + vc) * 8);
        dst[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
        dst[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
    }
    __syncthreads();
    const int64_t prow = ((int64_t)b * p.groups + g) * p.nsplit + split;
    if (tid < nc) {
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < R; ++r) {
            const f32x4 *src = reinterpret_cast<const f32x4 *>(red + (r * nc + tid) * 8);
            s0 += src[0];
            s1 += src[1];
        }
        f32x4 *out = reinterpret_cast<f32x4 *>(p.ws_acc + prow * p.dv + tid * 8);
        out[0] = s0;
        out[1] = s1;
    }
    if (tid == 0) *reinterpret_cast<f32x2 *>(p.ws_ml + prow * 2) = f32x2{m_run, l_run};
}

// Merge the splits (and, for the senses, the `groups` senses) of every output row.  Grid (rows, ceil(nc / 8)), one
// workgroup per 8 column chunks; thread (c, r) sums partials r, r + 32, ... of its chunk, then a fixed-order LDS sum.
template <class ET, bool SENSE>
__global__ __launch_bounds__(DEC_THREADS) void decode_combine_kernel(DecodeParams p) {
    using E = Elem<ET>;
    constexpr int CW = 8;
    __shared__ __attribute__((aligned(16))) float smem[64 * 64 + DEC_THREADS * 8];
    float *wt = smem;                             // [gpo][nsplit] weights
    float *red = smem + 64 * 64;
    const int row = blockIdx.x, tid = threadIdx.x;
    // trunk: row = (b, h), one group (the head itself); senses: row = b, every sense
    const int gpo = SENSE ? p.groups : 1;
    const int b = SENSE ? row : row / p.groups;
    const int64_t pbase = (int64_t)row * gpo;    // first partial group of this row
    const int n = dec_length(p, b) + 1;
    const int chunk = (n + p.nsplit - 1) / p.nsplit;
    const int nact = (n + chunk - 1) / chunk;
    for (int l = tid; l < gpo; l += DEC_THREADS) {
        const float *ml = p.ws_ml + (pbase + l) * p.nsplit * 2;
        float M = -INFINITY;
        for (int s = 0; s < nact; ++s) M = fmaxf(M, ml[2 * s]);
        float lsum = 0.f;
        for (int s = 0; s < nact; ++s) lsum += ml[2 * s + 1] * exp2f(ml[2 * s] - M);
        const float inv = 1.f / lsum;
        for (int s = 0; s < p.nsplit; ++s) wt[l * p.nsplit + s] = s < nact ? exp2f(ml[2 * s] - M) * inv : 0.f;
        if (!SENSE && p.lse != nullptr && blockIdx.y == 0)
            p.lse[b * p.lse_bs + row % p.groups] = (M + log2f(lsum)) * 0.69314718055994530942f;
    }
    __syncthreads();
    const int nc = p.dv >> 3;
    const int cw = nc < CW ? nc : CW;
    const int R = DEC_THREADS / cw;
    const int c = blockIdx.y * CW + tid % cw, r = tid / cw;
    const bool active = c < nc && r < R;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    const int terms = gpo * p.nsplit;
    if (active) {
        for (int i = r; i < terms; i += R) {
            const float w = wt[i];
            if (i % p.nsplit >= nact) continue;
            const f32x4 *src = reinterpret_cast<const f32x4 *>(p.ws_acc + (pbase * p.nsplit + i) * p.dv + c * 8);
            s0 += w * src[0];
            s1 += w * src[1];
        }
        f32x4 *dst = reinterpret_cast<f32x4 *>(red + (r * cw + tid % cw) * 8);
        dst[0] = s0;
        dst[1] = s1;
    }
    __syncthreads();
    if (tid < cw && blockIdx.y * CW + tid < nc) {
        f32x4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = {0.f, 0.f, 0.f, 0.f};
        for (int rr = 0; rr < R; ++rr) {
            const f32x4 *src = reinterpret_cast<const f32x4 *>(red + (rr * cw + tid) * 8);
            t0 += src[0];
            t1 += src[1];
        }
        const int cc = blockIdx.y * CW + tid;
        const int gh = SENSE ? 0 : row % p.groups;
        uint16_t *o = static_cast<uint16_t *>(p.o) + b * p.o_bs + gh * p.o_gs + cc * 8;
        *reinterpret_cast<u32x4 *>(o) = u32x4{E::pack2(t0[0], t0[1]), E::pack2(t0[2], t0[3]),
                                              E::pack2(t1[0], t1[1]), E::pack2(t1[2], t1[3])};
    }
}

// nsplit: about two workgroups per CU over the whole grid (256 CUs), at most 64 splits and no more than one per 64 keys
// of cache capacity.  The *_ws_floats queries and the launches share it.
inline int decode_nsplit_impl(int batch, int groups, int max_seqlen) {
    const int64_t rows = (int64_t)batch * groups;
    int want = (int)((512 + rows - 1) / rows);
    const int cap = (max_seqlen + DEC_TILE - 1) / DEC_TILE;
    if (want > cap) want = cap;
    if (want > 64) want = 64;
    return want < 1 ? 1 : want;
}

template <class ET, bool SENSE>
hipError_t launch_decode_combine(const DecodeParams &p, int nout, hipStream_t st) {
    const int nc = p.dv >> 3;
    hipLaunchKernelGGL((decode_combine_kernel<ET, SENSE>), dim3(nout, (nc + 7) / 8), dim3(DEC_THREADS), 0, st, p);
    return hipGetLastError();
}

template <class ET, int G, int NQ, bool SENSE>
hipError_t launch_decode_pair(const DecodeParams &p, int nout, hipStream_t st) {
    hipLaunchKernelGGL((decode_split_kernel<ET, G, NQ, SENSE>), dim3(p.nsplit, p.groups, p.b), dim3(DEC_THREADS), 0, st, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_decode_combine<ET, SENSE>(p, nout, st);
}

// G: 8-column chunks of the query row per key group (a power of two); the trunk (d_h <= 128) needs up to 16, the senses
// (d_k <= 640) go on to 64 and past that take the row in NQ = 2 passes
template <bool SENSE>
hipError_t launch_decode(const DecodeParams &p, int dtype, int nout, hipStream_t st) {
    return with_dtype(dtype, [&](auto et) {
        return with_bound<1, 2, 4, 8, 16, 32, 64, 128>(p.dk >> 3, hipErrorNotSupported, [&](auto qc) {
            constexpr int G = qc < 64 ? int(qc) : 64;
            if constexpr (!SENSE && qc > 16) return hipErrorNotSupported;
            else return launch_decode_pair<decltype(et), G, qc / G, SENSE>(p, nout, st);
        });
    });
}

}  // namespace bp
