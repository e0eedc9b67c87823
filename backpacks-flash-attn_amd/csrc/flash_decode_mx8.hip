// bp_flash_decode_mx8: bp_flash_decode on the MXFP8 KV cache (include/bp_hip.h, "MXFP8 KV cache") -- one byte tensor per
// layer; a position's row holds K elements (H, D), V elements (H, D), K scales (H, D / 32), V scales (H, D / 32).  Keys AND
// values are 8-bit, and the new token's K/V is quantised and appended in the same launch.
//
// Grid (nsplit, H, B), key ranges, the fp32 workspace rows and the second launch (decode_combine_kernel<ET, false>,
// flash_decode.hip's code object) are decode_core.h's.  The split kernel is written for 1-byte rows.  Per tile of 128 keys:
//   A  scores: a lane loads 16 key bytes (one 16-byte load) and the scale byte of their block, so G = D / 16 lanes (rounded
//      up to a power of two) cover a key: 16 keys per wave and pass at D = 64, four times the 16-bit kernel's, and a tile of
//      128 keys keeps as many bytes in flight per barrier as its 64.  The lane dots its bytes (eight v_cvt_pk_f32_fp8) with
//      its fp32 query slice, pre-scaled by scale * log2(e), multiplies the partial by the block scale ONCE (ldexp, exact)
//      and lane exchanges inside the group finish the key; the 128 scores go to LDS.
//   S  online softmax: every wave reduces the same 128 scores the same way, two per lane (identical m, l in every wave);
//      wave 0 stores the probabilities.
//   B  values, as sense_decode_mx8.hip: thread (c, r) owns 16 output columns c*16.. (half a scale block) and keys r, r + R,
//      ... of the tile, R = min(256 / (D / 16), 128); p' = ldexp(p, scale - 127), eight v_cvt_pk_f32_fp8, 16 fp32
//      accumulators.
// The new token (key L = cache_seqlens[b], always the last key of the last active split): the lanes that own key L in phase
// A read k_new (16-bit), take the block maximum with the neighbouring lane (two lanes share a block), quantise by the
// header's rule (mx8_block.h), store bytes and scale byte into row L and dot the ROUNDED bytes like any other key; the
// threads that own key L in phase B do the same with v_new.  A position therefore contributes the same numbers in the step
// that appends it and in every later one.  No workgroup reads cache row L, only this one writes it: race-free.
// The R key residues are summed in a fixed order through LDS and the partial (m, l, acc[d]) goes to the workspace: no
// atomics, bit-identical across calls.
#include "decode_core.h"
#include "mx8_block.h"

namespace bp {

constexpr int KV8_TILE = 128;

template <class ET, int D>
__global__ __launch_bounds__(DEC_THREADS) void flash_decode_mx8_kernel(KvDecodeMx8Params pp) {
    using E = Elem<ET>;
    const DecodeParams &p = pp.d;
    constexpr int NCH = D / 16;                   // 16-byte chunks of a key / value row: 2, 4, 6, 8
    constexpr int G = NCH <= 2 ? 2 : NCH <= 4 ? 4 : 8;   // lanes per key
    constexpr int KPW = 64 / G;                   // keys per wave per pass
    constexpr int KPB = 4 * KPW;                  // keys per workgroup per pass
    constexpr int NP = KV8_TILE / KPB;            // passes per tile: 1, 2, 4, 4
    constexpr int R = DEC_THREADS / NCH < KV8_TILE ? DEC_THREADS / NCH : KV8_TILE;   // key residues of phase B
    constexpr int NKT = (KV8_TILE + R - 1) / R;   // keys per thread per tile in phase B
    constexpr int NB = D / 32;                    // scale bytes of a (key, head)
    __shared__ __attribute__((aligned(16))) float smem[4 * KV8_TILE + R * D];
    float *sc = smem;                             // [2][128] scores
    float *pb = smem + 2 * KV8_TILE;              // [2][128] probabilities
    float *red = smem + 4 * KV8_TILE;             // [R][D] final reduction

    const int split = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = dec_length(p, b);
    const int n = L + 1;
    const int chunk = (n + p.nsplit - 1) / p.nsplit;
    const int j0 = split * chunk;
    if (j0 >= n) return;                          // uniform: the combine skips this split the same way
    const int j1 = min(n, j0 + chunk);

    // byte offsets of head g inside a row
    const int hd = p.groups * D;
    const int k_el = g * D, v_el = hd + g * D, k_sc = 2 * hd + g * NB, v_sc = 2 * hd + (p.groups + g) * NB;
    uint8_t *crow = pp.cache + (int64_t)b * pp.c_bs;

    const int li = lane & (G - 1);
    const bool chunk_ok = li < NCH;               // D = 96: lanes 6, 7 of a group carry zeros
    const int kslot = wave * KPW + lane / G;      // this lane's key inside a pass

    float qf[16];
    {
        const uint16_t *q = static_cast<const uint16_t *>(p.q) + b * p.q_bs + g * p.q_gs + li * 16;
        const u32x4 z = {0u, 0u, 0u, 0u};
        unpack8<E>(chunk_ok ? ld_global_16B(q) : z, *reinterpret_cast<float (*)[8]>(qf));
        unpack8<E>(chunk_ok ? ld_global_16B(q + 8) : z, *reinterpret_cast<float (*)[8]>(qf + 8));
#pragma unroll
        for (int e = 0; e < 16; ++e) qf[e] *= p.scale_log2e;
    }

    const int vc = tid % NCH, vr = tid / NCH;
    const bool v_active = vr < R;
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    for (int jt = j0, buf = 0; jt < j1; jt += KV8_TILE, buf ^= 1) {
        const int tl = min(KV8_TILE, j1 - jt);
        const int jl = L - jt;                    // the new key's place in this tile, when 0 <= jl < tl
        const bool has_new = jl >= 0 && jl < tl;  // uniform
        // ---- A: scores of the tile's keys ----
        u32x4 kb[NP];
        int ks[NP];
#pragma unroll
        for (int ps = 0; ps < NP; ++ps) {
            const int jj = ps * KPB + kslot;
            const int j = jt + jj;
            kb[ps] = u32x4{0u, 0u, 0u, 0u};
            ks[ps] = 127;
            if (jj < tl && chunk_ok && j != L) {
                const uint8_t *row = crow + (int64_t)j * pp.c_rs;
                kb[ps] = *reinterpret_cast<const u32x4 *>(row + k_el + li * 16);
                ks[ps] = row[k_sc + (li >> 1)];
            }
        }
        if (has_new) {
            const bool mine = chunk_ok && (jl % KPB) == kslot;   // pairs of lanes (li, li ^ 1) decide alike
            if (mine) {                           // quantise and append the new key; attend to the rounded bytes
                const uint16_t *kn = static_cast<const uint16_t *>(p.k_new) + b * p.kn_bs + g * p.kn_gs + li * 16;
                float f[16];
                float amax = fmaxf(mx8_unpack8_amax<E>(ld_global_16B(kn), f), mx8_unpack8_amax<E>(ld_global_16B(kn + 8), f + 8));
                amax = fmaxf(amax, __shfl_xor(amax, 1));
                const int s = mx8_scale_byte(amax);
                const u32x4 nk = {mx8_pack4(f[0], f[1], f[2], f[3], s), mx8_pack4(f[4], f[5], f[6], f[7], s),
                                  mx8_pack4(f[8], f[9], f[10], f[11], s), mx8_pack4(f[12], f[13], f[14], f[15], s)};
                uint8_t *row = crow + (int64_t)L * pp.c_rs;
                *reinterpret_cast<u32x4 *>(row + k_el + li * 16) = nk;
                if ((li & 1) == 0) row[k_sc + (li >> 1)] = (uint8_t)s;
                const int psn = jl / KPB;
#pragma unroll
                for (int ps = 0; ps < NP; ++ps)
                    if (ps == psn) { kb[ps] = nk; ks[ps] = s; }
            }
        }
#pragma unroll
        for (int ps = 0; ps < NP; ++ps) {
            const int jj = ps * KPB + kslot;
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float kf[4];
                mx8_unpack4(kb[ps][i], kf);
#pragma unroll
                for (int e = 0; e < 4; ++e) d = fmaf(qf[4 * i + e], kf[e], d);
            }
            d = ldexpf(d, ks[ps] - 127);          // the block scale, once per lane
#pragma unroll
            for (int off = G / 2; off > 0; off >>= 1) d += __shfl_xor(d, off);
            if (jj < tl && li == 0) sc[buf * KV8_TILE + jj] = d;
        }
        __syncthreads();
        // ---- S: online softmax, the same reduction in every wave (two scores per lane) ----
        const float x0 = lane < tl ? sc[buf * KV8_TILE + lane] : -INFINITY;
        const float x1 = lane + 64 < tl ? sc[buf * KV8_TILE + 64 + lane] : -INFINITY;
        float tmax = fmaxf(x0, x1);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, off));
        const float m_new = fmaxf(m_run, tmax);
        const float alpha = m_run == -INFINITY ? 0.f : exp2f(m_run - m_new);
        const float p0 = lane < tl ? exp2f(x0 - m_new) : 0.f;
        const float p1 = lane + 64 < tl ? exp2f(x1 - m_new) : 0.f;
        float ls = p0 + p1;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) ls += __shfl_xor(ls, off);
        l_run = l_run * alpha + ls;
        m_run = m_new;
        if (wave == 0) {
            pb[buf * KV8_TILE + lane] = p0;
            pb[buf * KV8_TILE + 64 + lane] = p1;
        }
        __syncthreads();
        // ---- B: acc = alpha * acc + sum_j (p_j 2^(scale_j - 127)) e4m3_j ----
        if (v_active) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] *= alpha;
            u32x4 w[NKT];
            float pj[NKT];
            int sb[NKT];
#pragma unroll
            for (int u = 0; u < NKT; ++u) {
                const int jj = vr + u * R;
                pj[u] = 0.f;
                sb[u] = 127;
                w[u] = u32x4{0u, 0u, 0u, 0u};
                if (jj < tl) {
                    const int j = jt + jj;
                    pj[u] = pb[buf * KV8_TILE + jj];
                    if (j != L) {
                        const uint8_t *row = crow + (int64_t)j * pp.c_rs;
                        w[u] = *reinterpret_cast<const u32x4 *>(row + v_el + vc * 16);
                        sb[u] = row[v_sc + (vc >> 1)];
                    }
                }
            }
            if (has_new && (jl % R) == vr) {      // threads (vc, vc ^ 1) of one residue decide alike
                const uint16_t *vn = static_cast<const uint16_t *>(p.v_new) + b * p.vn_bs + g * p.vn_gs + vc * 16;
                float f[16];
                float amax = fmaxf(mx8_unpack8_amax<E>(ld_global_16B(vn), f), mx8_unpack8_amax<E>(ld_global_16B(vn + 8), f + 8));
                amax = fmaxf(amax, __shfl_xor(amax, 1));
                const int s = mx8_scale_byte(amax);
                const u32x4 nv = {mx8_pack4(f[0], f[1], f[2], f[3], s), mx8_pack4(f[4], f[5], f[6], f[7], s),
                                  mx8_pack4(f[8], f[9], f[10], f[11], s), mx8_pack4(f[12], f[13], f[14], f[15], s)};
                uint8_t *row = crow + (int64_t)L * pp.c_rs;
                *reinterpret_cast<u32x4 *>(row + v_el + vc * 16) = nv;
                if ((vc & 1) == 0) row[v_sc + (vc >> 1)] = (uint8_t)s;
                const int un = jl / R;
#pragma unroll
                for (int u = 0; u < NKT; ++u)
                    if (u == un) { w[u] = nv; sb[u] = s; }
            }
#pragma unroll
            for (int u = 0; u < NKT; ++u) {
                const float ps = ldexpf(pj[u], sb[u] - 127);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float vf[4];
                    mx8_unpack4(w[u][i], vf);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * i + e] = fmaf(ps, vf[e], acc[4 * i + e]);
                }
            }
        }
    }
    // ---- reduce the R key residues of every column (fixed order) and leave the partial ----
    if (v_active) {
        f32x4 *dst = reinterpret_cast<f32x4 *>(red + vr * D + vc * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[i] = f32x4{acc[4 * i], acc[4 * i + 1], acc[4 * i + 2], acc[4 * i + 3]};
    }
    __syncthreads();
    const int64_t prow = ((int64_t)b * p.groups + g) * p.nsplit + split;
    if (tid < D / 4) {                            // four columns per thread
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < R; ++r) s += *reinterpret_cast<const f32x4 *>(red + r * D + tid * 4);
        *reinterpret_cast<f32x4 *>(p.ws_acc + prow * D + tid * 4) = s;
    }
    if (tid == 0) *reinterpret_cast<f32x2 *>(p.ws_ml + prow * 2) = f32x2{m_run, l_run};
}

hipError_t launch_flash_decode_mx8(const KvDecodeMx8Params &p, int dtype, hipStream_t stream) {
    const hipError_t e = with_dtype(dtype, [&](auto et) {
        return with_bound<32, 64, 96, 128>(p.d.dk, hipErrorNotSupported, [&](auto d) {
            if (p.d.dk != d) return hipErrorNotSupported;     // head_dim % 32 == 0 only
            hipLaunchKernelGGL((flash_decode_mx8_kernel<decltype(et), d>), dim3(p.d.nsplit, p.d.groups, p.d.b),
                               dim3(DEC_THREADS), 0, stream, p);
            return hipGetLastError();
        });
    });
    return e != hipSuccess ? e : launch_flash_decode_combine(p.d, dtype, stream);
}

}  // namespace bp
