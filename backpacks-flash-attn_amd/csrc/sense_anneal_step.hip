// bp_sense_anneal_step: one cached step of the annealed sense weights (src/models/intervened_models.py, step_key_weight)
// in two launches.  Per sample b with L = its cached length, x_L the new token, row(b, j) the sense rows of position j:
//   sims[b,l,j] += relu(T[row(b,j),l,:] . E[x_L])                                  j <  L   (A)
//   sims[b,l,L]  = sum_{j <= L} relu(T[new_row[b],l,:] . E[x_j]),  x_j = ids[b,j]   j == L  (B)
//   weight[b,l,j] = cw[x_j,l] s + (1 - s),  s = sigmoid(6 - scale sims[b,l,j]) [(1 + j / 100)],   ids[b,L] = x_L
//
// Main kernel: grid (ceil(max_seqlen / 16), batch), 1024 threads, AS_POS = 16 positions per workgroup; workgroups past L
// leave at once (the lengths are read on the device: one captured graph serves every step).  Why 16: it is one M tile of
// v_mfma_f32_16x16x32, and the k x d_out block of the new token that (B) needs in LDS is re-read from L2 once per
// workgroup -- 24 KB on Small against the 16 x 25.5 KB the workgroup streams, 6 % on top where 4 positions would pay 24 %.
//   staging   the 16 waves copy T[new_row[b]] (k rows, zero rows up to a multiple of 16) to LDS with 16-byte loads; a row
//             takes d_out * 2 + 16 bytes, so the 16 rows a ds_read_b128 group touches fall into different banks.
//   (B)       D (16 positions x 16 senses) += A (positions x 32 columns) B (32 columns x senses) per sense tile NT =
//             ceil(k / 16): lane (m = lane & 15, q = lane >> 4) supplies A as columns 8 q .. 8 q + 7 of E[x_{j0+m}], one
//             16-byte global load straight to VGPRs (an LM-head row is read once per workgroup), and B as the same columns
//             of staged row 16 t + m, one 16-byte LDS read.  The 32-column steps of d_out are dealt round-robin to the 16
//             waves; every wave leaves its partial D (lane holds D[4 q + r][m]) in LDS, the workgroup adds the 16 in a
//             fixed order, applies the relu and the mask j <= L, sums the 16 positions with four lane exchanges and
//             writes ws[b, blockIdx.x, l].  Position L takes part with x_L = new_ids[b] (ids[b,L] is not read), so the pair
//             (L, L) comes exactly once, here.
//   (A)       the row walk of sense_rows_dot.hip, wave w on position j0 + w if it lies below L: E[x_L] in
//             registers, 16-byte chunks lane, lane + 64, ... of each sense row, six lane exchanges per dot.  The workgroup
//             then updates its (senses, 16) block of sims and weight, 64-byte segments along the unit stride.
// Tail kernel: grid (batch), 64 threads, thread l: sims[b,l,L] = ws[b,0,l] + ws[b,1,l] + ... in block order, the weight
// of position L, ids[b,L] = x_L.  Every block <= L / 16 writes all k of its partials in the same launch pair, so the
// workspace is never zeroed.  No atomics, fixed order everywhere: bit-identical across calls.
#include "bp_common.h"
#include "bp_kernels.h"

namespace bp {

constexpr int AS_THREADS = 1024;
constexpr int AS_WAVES = AS_THREADS / 64;    // = AS_POS: (A) gives every wave one position

template <class ET> struct Mfma16;    // v_mfma_f32_16x16x32: A[lane & 15][8 (lane >> 4) + t], B[8 (lane >> 4) + t][lane & 15],
template <> struct Mfma16<BF16> {     // D reg r = D[4 (lane >> 4) + r][lane & 15]
    static BP_DEV f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
template <> struct Mfma16<F16> {
    static BP_DEV f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};
// settle_acc of bp_common.h for the 4-register accumulator of the 16x16x32 shape (4 passes; the same 12 slots cover it)
BP_DEV void settle_acc(f32x4 &v) { asm volatile("s_nop 7\n\ts_nop 3" : "+v"(v)); }

BP_DEV int64_t clamp_row(int64_t i, int64_t rows) { return (uint64_t)i < (uint64_t)rows ? i : rows - 1; }
BP_DEV int anneal_length(const AnnealStepParams &p, int b) {
    const int L = p.seqlens[b];
    return L < 0 ? 0 : (L >= p.max_seqlen ? p.max_seqlen - 1 : L);     // never index outside the cache
}
// mask_annealing's score and create_content_soft_mask for one (token, sense, position)
BP_DEV float anneal_weight(const AnnealStepParams &p, float sims, float picked, int j) {
    float s = 1.f / (1.f + expf(-(6.f - p.scale * sims)));
    if (p.upweight) s *= 1.f + (float)j / 100.f;
    return picked * s + (1.f - s);
}

template <class ET, int NCH, int NT>  // NCH: 16-byte chunks of a row per lane in (A), ceil(d_out / 512); NT: sense tiles of 16
__global__ __launch_bounds__(AS_THREADS) void sense_anneal_step_kernel(AnnealStepParams p) {
    using E = Elem<ET>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KP = NT * 16;
    const int pitch = p.dout * 2 + 16;
    float *part = reinterpret_cast<float *>(smem + KP * pitch);        // [16 waves][16 positions][KP]
    float *res = part + AS_WAVES * AS_POS * KP;                               // [KP][16 positions]
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = anneal_length(p, b);
    const int j0 = blockIdx.x * AS_POS;
    if (j0 > L) return;                                                // uniform over the workgroup
    const int nc = p.dout >> 3;
    const uint16_t *table = static_cast<const uint16_t *>(p.table), *emb = static_cast<const uint16_t *>(p.emb);
    const int64_t x_new = p.new_ids[b * p.nid_s];

    // ---- staging: the new token's sense rows ----
    const uint16_t *tnew = table + clamp_row((uint32_t)p.new_row[b], p.table_rows) * p.t_rs;
    for (int l = wave; l < KP; l += AS_WAVES)
        for (int c = lane; c < nc; c += 64)
            lds_write_16B(smem, l * pitch + c * 16, l < p.groups ? ld_global_16B(tnew + l * p.t_gs + c * 8) : u32x4{0u, 0u, 0u, 0u});
    __syncthreads();

    // ---- (B): 16 LM-head rows against the staged block ----
    {
        const int m = lane & 15, q = lane >> 4, j = j0 + m;
        const bool live = j <= L;
        const int64_t tok = clamp_row(j == L ? x_new : (live ? p.ids[b * p.ids_bs + j] : 0), p.vocab);
        const uint16_t *erow = emb + tok * p.e_rs;
        f32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int nsteps = (nc + 3) >> 2;
        for (int s = wave; s < nsteps; s += AS_WAVES) {
            const int c = s * 4 + q;
            const bool in = c < nc;
            const u32x4 a = live && in ? ld_global_16B(erow + c * 8) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const u32x4 w = in ? lds_read_16B(smem, (t * 16 + m) * pitch + c * 16) : u32x4{0u, 0u, 0u, 0u};
                acc[t] = Mfma16<ET>::mfma(a, w, acc[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            settle_acc(acc[t]);
            const f32x4 d = acc[t];
            part[(wave * AS_POS + 4 * q + 0) * KP + t * 16 + m] = d[0];
            part[(wave * AS_POS + 4 * q + 1) * KP + t * 16 + m] = d[1];
            part[(wave * AS_POS + 4 * q + 2) * KP + t * 16 + m] = d[2];
            part[(wave * AS_POS + 4 * q + 3) * KP + t * 16 + m] = d[3];
        }
    }
    __syncthreads();
    if (tid < KP * AS_POS) {                                           // KP * 16 is a multiple of 64: uniform over a wave
        const int n = tid >> 4, m = tid & 15;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < AS_WAVES; ++w) v += part[(w * AS_POS + m) * KP + n];
        v = j0 + m <= L ? fmaxf(v, 0.f) : 0.f;
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (m == 0 && n < p.groups) p.ws[((int64_t)b * p.nblk + blockIdx.x) * p.groups + n] = v;
    }

    // ---- (A): the cached positions' own rows against E[x_L] ----
    if (j0 >= L) return;                                               // nothing cached in this block (uniform)
    const uint16_t *vec = emb + clamp_row(x_new, p.vocab) * p.e_rs;
    float vf[NCH][8];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = lane + i * 64;
        const u32x4 w = c < nc ? ld_global_16B(vec + c * 8) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            vf[i][2 * e] = E::lo_f32(w[e]);
            vf[i][2 * e + 1] = E::hi_f32(w[e]);
        }
    }
    if (j0 + wave < L) {                                               // uniform over the wave
        const int jw = wave;
        const uint16_t *trow = table + clamp_row((uint32_t)p.row_index[b * p.ri_bs + j0 + jw], p.table_rows) * p.t_rs;
#pragma unroll 4
        for (int l = 0; l < p.groups; ++l) {
            u32x4 w[NCH];
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = lane + i * 64;
                w[i] = c < nc ? ld_global_16B(trow + l * p.t_gs + c * 8) : u32x4{0u, 0u, 0u, 0u};
            }
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    d = fmaf(E::lo_f32(w[i][e]), vf[i][2 * e], d);
                    d = fmaf(E::hi_f32(w[i][e]), vf[i][2 * e + 1], d);
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off);
            if (lane == 0) res[l * AS_POS + jw] = d;
        }
    }
    __syncthreads();
    for (int i = tid; i < p.groups * AS_POS; i += AS_THREADS) {
        const int l = i >> 4, j = j0 + (i & 15);
        if (j >= L) continue;
        float *sp = p.sims + b * p.s_bs + l * p.s_gs + j;
        const float sv = *sp + fmaxf(res[i], 0.f);
        *sp = sv;
        const int64_t tok = clamp_row(p.ids[b * p.ids_bs + j], p.cw_rows);
        p.weight[b * p.w_bs + l * p.w_gs + j] = anneal_weight(p, sv, p.cw[tok * p.cw_rs + l], j);
    }
}

__global__ __launch_bounds__(64) void sense_anneal_tail_kernel(AnnealStepParams p) {
    const int b = blockIdx.x, l = threadIdx.x;
    const int L = anneal_length(p, b);
    const int64_t x_new = p.new_ids[b * p.nid_s];
    if (l < p.groups) {
        const float *w = p.ws + (int64_t)b * p.nblk * p.groups + l;
        float s = 0.f;
        for (int blk = 0; blk <= L / AS_POS; ++blk) s += w[(int64_t)blk * p.groups];
        p.sims[b * p.s_bs + l * p.s_gs + L] = s;
        p.weight[b * p.w_bs + l * p.w_gs + L] = anneal_weight(p, s, p.cw[clamp_row(x_new, p.cw_rows) * p.cw_rs + l], L);
    }
    if (l == 0) p.ids[b * p.ids_bs + L] = x_new;
}

int64_t anneal_step_lds_bytes(int nsenses, int d_out) {
    const int64_t kp = (nsenses + 15) / 16 * 16;
    return kp * (d_out * 2 + 16) + (AS_WAVES * AS_POS * kp + kp * AS_POS) * (int64_t)sizeof(float);
}

hipError_t launch_sense_anneal_step(const AnnealStepParams &p, int dtype, hipStream_t stream) {
    const size_t lds = (size_t)anneal_step_lds_bytes(p.groups, p.dout);
    const hipError_t e = with_dtype(dtype, [&](auto et) {
        return with_bound<1, 2, 3, 4>((p.dout + 511) / 512, hipErrorNotSupported, [&](auto nch) {
            return with_bound<1, 2, 3, 4>((p.groups + 15) / 16, hipErrorNotSupported, [&](auto nt) {
                hipLaunchKernelGGL((sense_anneal_step_kernel<decltype(et), nch, nt>), dim3(p.nblk, p.b), dim3(AS_THREADS),
                                   lds, stream, p);
                return hipGetLastError();
            });
        });
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sense_anneal_tail_kernel, dim3(p.b), dim3(64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace bp
