// bp_sense_rows_dot: the gathered GEMV of the annealed intervention's running similarity sums,
//   out[b, l, j] = sum_c table[row(b, j), l, c] * vec[b, c],   j = 0 .. L_b,  row(b, L_b) = new_row[b],
// over exactly the rows bp_sense_decode reads (k * d_out * 2 bytes per position).  Memory-bound: grid (ceil(max_seqlen /
// 4), batch), one wave per position; the wave walks the position's senses, every lane takes 16-byte chunks lane, lane +
// 64, ... of the row straight to VGPRs against `vec` held in registers, and a lane-exchange reduction leaves the dot
// in LDS; the workgroup then stores its (senses, 4) block with the positions along the unit stride.  The lengths are read
// on the device (workgroups past L_b leave at once), so a captured graph serves every step.  Fixed reduction order.
#include "bp_common.h"
#include "bp_kernels.h"

namespace bp {

constexpr int RD_THREADS = 256;
constexpr int RD_POS = 4;             // positions per workgroup, one per wave

template <class ET, int NCH>          // NCH: 16-byte chunks of a row per lane, ceil(d_out / 512)
__global__ __launch_bounds__(RD_THREADS) void sense_rows_dot_kernel(RowsDotParams p) {
    using E = Elem<ET>;
    __shared__ float res[64 * RD_POS];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int L = p.seqlens[b];
    L = L < 0 ? 0 : (L >= p.max_seqlen ? p.max_seqlen - 1 : L);      // never index outside the cache
    const int j0 = blockIdx.x * RD_POS;
    if (j0 > L) return;                                                // uniform over the workgroup
    const int j = j0 + wave;
    const int nc = p.dout >> 3;

    const uint16_t *vec = static_cast<const uint16_t *>(p.vec) + b * p.v_bs;
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
    if (j <= L) {                                                      // uniform over the wave
        const int row = j == L ? p.new_row[b] : p.row_index[b * p.ri_bs + j];
        const uint32_t ur = (uint32_t)row;                             // clamp as unsigned: a bad index reads the last row
        const int64_t r = ur < (uint32_t)p.table_rows ? ur : (uint32_t)(p.table_rows - 1);
        const uint16_t *trow = static_cast<const uint16_t *>(p.table) + r * p.t_rs;
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
            if (lane == 0) res[l * RD_POS + wave] = d;
        }
    }
    __syncthreads();
    if (tid < p.groups * RD_POS) {
        const int l = tid / RD_POS, jj = j0 + tid % RD_POS;
        if (jj <= L) p.out[b * p.o_bs + l * p.o_gs + jj] = res[tid];
    }
}

hipError_t launch_sense_rows_dot(const RowsDotParams &p, int dtype, hipStream_t stream) {
    return with_dtype(dtype, [&](auto et) {
        return with_bound<1, 2, 3, 4>((p.dout + 511) / 512, hipErrorNotSupported, [&](auto nch) {
            hipLaunchKernelGGL((sense_rows_dot_kernel<decltype(et), nch>),
                               dim3((p.max_seqlen + RD_POS - 1) / RD_POS, p.b), dim3(RD_THREADS), 0, stream, p);
            return hipGetLastError();
        });
    });
}

}  // namespace bp
