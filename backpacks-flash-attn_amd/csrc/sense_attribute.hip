// bp_sense_attribute: the shares of (position, sense) pairs in a logit.  For query n = (sample b, position i) with vectors
// vec[n, v, :] (fp32: E[w], or a sum of embedding rows)
//   out[n, v, l, j] = p_j * sum_c table[row(b, j), l, c] * vec[n, v, c],   p = softmax_{j <= i}(scale q_l(i) . k_l(j)),
// zeros behind i.  Nothing of size k S^2 or S k d exists: the only workspace is the (m, Z) pair of every (query, sense).
//   pass 1  grid (nsenses, nq), 256 threads: q_l in LDS, a lane per key, two sweeps over keys 0 .. i (max, then the sum of
//           exp(s - m)); lane partials in ascending key order, a butterfly within the wave, the four waves in order.
//   pass 2  grid (ceil(seqlen / 4), nq), one wave per position, the row loop of sense_rows_dot.hip: lane l forms the score
//           and the probability of sense l; then per sense every lane takes 16-byte chunks lane, lane + 64, ... of the table
//           row against `vec` held in registers (NV * NCH * 8 fp32), a lane-exchange reduction per vector, and lane 0
//           leaves p * dot in LDS.  The workgroup stores its (nvec, nsenses, 4) block, positions along the unit stride.
// Both passes form a score with attr_score and an exponential with attr_exp, so e_j <= 1 and the largest is exactly 1.
// Queries are read on the device (clamped), so a captured launch serves any queries.  No atomics; fixed reduction order.
#include "bp_common.h"
#include "bp_kernels.h"

namespace bp {

constexpr int AT_THREADS = 256;
constexpr int AT_POS = 4;             // positions per workgroup of pass 2, one per wave

// scale * q . k over `nc` 16-byte chunks: one accumulator, ascending columns.  THE score of both passes.
template <class ET> BP_DEV float attr_score(const uint16_t *q, const uint16_t *k, int nc, float scale) {
    using E = Elem<ET>;
    float acc = 0.f;
    for (int c = 0; c < nc; ++c) {
        const u32x4 a = *reinterpret_cast<const u32x4 *>(q + c * 8);
        const u32x4 b = ld_global_16B(k + c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc = fmaf(E::lo_f32(a[e]), E::lo_f32(b[e]), acc);
            acc = fmaf(E::hi_f32(a[e]), E::hi_f32(b[e]), acc);
        }
    }
    return scale * acc;
}

BP_DEV float attr_exp(float s, float m) { return expf(s - m); }   // exp(0) == 1 exactly; 0 below -104

BP_DEV int attr_clamp(int x, int n) { return x < 0 ? 0 : (x >= n ? n - 1 : x); }

template <class ET>
__global__ __launch_bounds__(AT_THREADS) void sense_attribute_stats_kernel(AttributeParams p) {
    __shared__ __attribute__((aligned(16))) uint16_t qs[kWideMaxDk];
    __shared__ float red[AT_THREADS / 64];
    const int l = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = attr_clamp(p.query_sample[n], p.b), i = attr_clamp(p.query_pos[n], p.s);
    const int nc = p.dk >> 3;
    const uint16_t *q = static_cast<const uint16_t *>(p.q) + b * p.qk_bs + i * p.qk_rs + l * p.qk_ss;
    const uint16_t *k = static_cast<const uint16_t *>(p.k) + b * p.qk_bs + l * p.qk_ss;
    if (tid < nc) *reinterpret_cast<u32x4 *>(qs + tid * 8) = ld_global_16B(q + tid * 8);
    __syncthreads();

    float m = -INFINITY;
    for (int j = tid; j <= i; j += AT_THREADS) m = fmaxf(m, attr_score<ET>(qs, k + j * p.qk_rs, nc, p.scale));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();

    float z = 0.f;
    for (int j = tid; j <= i; j += AT_THREADS) z += attr_exp(attr_score<ET>(qs, k + j * p.qk_rs, nc, p.scale), m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off);
    if (lane == 0) red[wave] = z;
    __syncthreads();
    if (tid == 0) {
        float *ws = p.ws + ((int64_t)n * p.groups + l) * 2;
        ws[0] = m;
        ws[1] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

template <class ET, int NCH, int NV>  // NCH: 16-byte chunks of a row per lane, ceil(d_out / 512); NV: vectors held, >= nvec
__global__ __launch_bounds__(AT_THREADS) void sense_attribute_kernel(AttributeParams p) {
    using E = Elem<ET>;
    __shared__ float res[NV * 64 * AT_POS];
    __shared__ float prob[64 * AT_POS];
    const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = attr_clamp(p.query_sample[n], p.b), i = attr_clamp(p.query_pos[n], p.s);
    const int j0 = blockIdx.x * AT_POS, j = j0 + wave;
    const int groups = p.groups, cells = groups * AT_POS;
    float *out = p.out + n * p.o_qs;
    float *probs = p.probs != nullptr ? p.probs + n * p.p_qs : nullptr;

    if (j0 > i) {                                                      // uniform over the workgroup: only the zeros
        for (int t = tid; t < p.nvec * cells; t += AT_THREADS) {
            const int jj = j0 + t % AT_POS, l = t / AT_POS % groups, v = t / cells;
            if (jj < p.s) out[v * p.o_vs + l * p.o_gs + jj] = 0.f;
        }
        if (probs != nullptr && tid < cells) {
            const int jj = j0 + tid % AT_POS, l = tid / AT_POS;
            if (jj < p.s) probs[l * p.p_gs + jj] = 0.f;
        }
        return;
    }

    if (j <= i) {                                                      // uniform over the wave
        const int nc = p.dout >> 3;
        const float *vec = p.vec + n * p.v_qs;
        float vf[NV][NCH][8];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int ch = lane + c * 64;
                const bool live = v < p.nvec && ch < nc;
                const float4 lo = live ? *reinterpret_cast<const float4 *>(vec + v * p.v_vs + ch * 8) : float4{0.f, 0.f, 0.f, 0.f};
                const float4 hi = live ? *reinterpret_cast<const float4 *>(vec + v * p.v_vs + ch * 8 + 4) : float4{0.f, 0.f, 0.f, 0.f};
                vf[v][c][0] = lo.x; vf[v][c][1] = lo.y; vf[v][c][2] = lo.z; vf[v][c][3] = lo.w;
                vf[v][c][4] = hi.x; vf[v][c][5] = hi.y; vf[v][c][6] = hi.z; vf[v][c][7] = hi.w;
            }
        }
        float pj = 0.f;                                                // lane l: the probability of sense l at position j
        if (lane < groups) {
            const uint16_t *q = static_cast<const uint16_t *>(p.q) + b * p.qk_bs + i * p.qk_rs + lane * p.qk_ss;
            const uint16_t *k = static_cast<const uint16_t *>(p.k) + b * p.qk_bs + j * p.qk_rs + lane * p.qk_ss;
            const float *ws = p.ws + ((int64_t)n * groups + lane) * 2;
            pj = attr_exp(attr_score<ET>(q, k, p.dk >> 3, p.scale), ws[0]) / ws[1];
            prob[lane * AT_POS + wave] = pj;
        }
        const uint32_t ur = (uint32_t)p.row_index[b * p.ri_bs + j];    // clamp as unsigned: a bad index reads the last row
        const int64_t r = ur < (uint32_t)p.table_rows ? ur : (uint32_t)(p.table_rows - 1);
        const uint16_t *trow = static_cast<const uint16_t *>(p.table) + r * p.t_rs;
        for (int l = 0; l < groups; ++l) {
            u32x4 w[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int ch = lane + c * 64;
                w[c] = ch < nc ? ld_global_16B(trow + l * p.t_gs + ch * 8) : u32x4{0u, 0u, 0u, 0u};
            }
            const float pl = __shfl(pj, l);
            float d[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                d[v] = 0.f;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        d[v] = fmaf(E::lo_f32(w[c][e]), vf[v][c][2 * e], d[v]);
                        d[v] = fmaf(E::hi_f32(w[c][e]), vf[v][c][2 * e + 1], d[v]);
                    }
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) d[v] += __shfl_xor(d[v], off);
                if (lane == 0) res[(v * groups + l) * AT_POS + wave] = pl * d[v];
            }
        }
    } else {                                                           // behind i inside a block that i cuts, or behind the row
        for (int t = lane; t < NV * groups; t += 64) res[t * AT_POS + wave] = 0.f;
        if (lane < groups) prob[lane * AT_POS + wave] = 0.f;
    }
    __syncthreads();
    for (int t = tid; t < p.nvec * cells; t += AT_THREADS) {
        const int jj = j0 + t % AT_POS, l = t / AT_POS % groups, v = t / cells;
        if (jj < p.s) out[v * p.o_vs + l * p.o_gs + jj] = res[t];
    }
    if (probs != nullptr && tid < cells) {
        const int jj = j0 + tid % AT_POS, l = tid / AT_POS;
        if (jj < p.s) probs[l * p.p_gs + jj] = prob[tid];
    }
}

hipError_t launch_sense_attribute(const AttributeParams &p, int dtype, hipStream_t stream) {
    return with_dtype(dtype, [&](auto et) {
        hipLaunchKernelGGL((sense_attribute_stats_kernel<decltype(et)>), dim3(p.groups, p.nq), dim3(AT_THREADS), 0, stream, p);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        return with_bound<1, 2, 3, 4>((p.dout + 511) / 512, hipErrorNotSupported, [&](auto nch) {
            return with_bound<1, 2, 4>(p.nvec, hipErrorNotSupported, [&](auto nv) {
                hipLaunchKernelGGL((sense_attribute_kernel<decltype(et), nch, nv>),
                                   dim3((p.s + AT_POS - 1) / AT_POS, p.nq), dim3(AT_THREADS), 0, stream, p);
                return hipGetLastError();
            });
        });
    });
}

}  // namespace bp
