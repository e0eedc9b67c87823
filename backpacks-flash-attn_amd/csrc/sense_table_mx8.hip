// bp_sense_table_quantize / bp_sense_table_dequantize: a 16-bit sense table (rows, k, d) to and from its MXFP8 twin
// (include/bp_hip.h, "MXFP8 sense table"): E4M3 elements in q8, one E8M0 scale byte per block of 32 columns in scale8.
//
// Both are one pass over the table, no LDS, no atomics: pure bandwidth.
//   quantise    4 lanes own one block of 32 columns, 8 columns each (one 16-byte load).  The block maximum goes round the
//               group in two lane exchanges; its fp32 exponent field IS floor(log2(amax)) + 127, so the scale byte is that
//               field minus 8 (the E4M3 emax), held at 0 from below.  Every element is scaled by an exact power of two
//               (v_ldexp_f32), clamped to +-448 in fp32, converted two at a time (v_cvt_pk_fp8_f32, round to nearest even)
//               and stored as one 8-byte word per lane; lane 0 of the group stores the scale byte.
//   dequantise  a lane owns 16 columns (half a block): one 16-byte load of q8, the block's scale byte, eight
//               v_cvt_pk_f32_fp8, an exponent add per element and two 16-byte stores.  Exact wherever the 16-bit type holds
//               the value (always in bf16), round to nearest even elsewhere (fp16 beyond its range).
#include "bp_common.h"
#include "bp_kernels.h"

namespace bp {

constexpr int MX8_THREADS = 256;

template <class ET>
__global__ __launch_bounds__(MX8_THREADS) void sense_table_quantize_kernel(Mx8TableParams p) {
    using E = Elem<ET>;
    const int64_t t = (int64_t)blockIdx.x * MX8_THREADS + threadIdx.x;
    const int64_t blk = t >> 2;
    const int li = (int)(t & 3);
    const int nb = p.d >> 5;
    const int64_t per_row = (int64_t)p.k * nb;
    if (blk >= p.rows * per_row) return;          // whole groups of 4 lanes leave together
    const int64_t row = blk / per_row;
    const int rem = (int)(blk - row * per_row);
    const int g = rem / nb, bi = rem - g * nb;

    const uint16_t *src = static_cast<const uint16_t *>(p.table) + row * p.t_rs + g * p.t_gs + bi * 32 + li * 8;
    const u32x4 w = ld_global_16B(src);
    float f[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = E::lo_f32(w[i]);
        f[2 * i + 1] = E::hi_f32(w[i]);
    }
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    // exponent field of a non-negative finite float; a subnormal maximum has field 0 and lands on scale byte 0 as well
    const int field = (int)(as_u32(amax) >> 23);
    const int s = amax == 0.f ? 127 : max(field - 8, 0);
    uint32_t o[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fminf(fmaxf(ldexpf(f[4 * i + e], 127 - s), -448.f), 448.f);
        int packed = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
        packed = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], packed, true);
        o[i] = (uint32_t)packed;
    }
    uint8_t *dst = p.q8 + row * p.q_rs + g * p.q_gs + bi * 32 + li * 8;
    *reinterpret_cast<u32x2 *>(dst) = u32x2{o[0], o[1]};
    if (li == 0) p.scale8[row * p.s_rs + g * p.s_gs + bi] = (uint8_t)s;
}

template <class ET>
__global__ __launch_bounds__(MX8_THREADS) void sense_table_dequantize_kernel(Mx8TableParams p) {
    using E = Elem<ET>;
    const int64_t t = (int64_t)blockIdx.x * MX8_THREADS + threadIdx.x;
    const int nh = p.d >> 4;                      // 16-column halves of the blocks of a row
    const int64_t per_row = (int64_t)p.k * nh;
    if (t >= p.rows * per_row) return;
    const int64_t row = t / per_row;
    const int rem = (int)(t - row * per_row);
    const int g = rem / nh, hi = rem - g * nh;

    const u32x4 w = *reinterpret_cast<const u32x4 *>(p.q8 + row * p.q_rs + g * p.q_gs + hi * 16);
    const int ex = (int)p.scale8[row * p.s_rs + g * p.s_gs + (hi >> 1)] - 127;
    uint32_t o[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t wi = w[i];                 // by value: see as_f32
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)wi, false);
        const f32x2 up = __builtin_amdgcn_cvt_pk_f32_fp8((int)wi, true);
        o[2 * i] = E::pack2(ldexpf(lo[0], ex), ldexpf(lo[1], ex));
        o[2 * i + 1] = E::pack2(ldexpf(up[0], ex), ldexpf(up[1], ex));
    }
    uint16_t *dst = static_cast<uint16_t *>(p.table) + row * p.t_rs + g * p.t_gs + hi * 16;
    *reinterpret_cast<u32x4 *>(dst) = u32x4{o[0], o[1], o[2], o[3]};
    *reinterpret_cast<u32x4 *>(dst + 8) = u32x4{o[4], o[5], o[6], o[7]};
}

static int64_t mx8_grid(const Mx8TableParams &p, int cols_per_thread) {
    const int64_t threads = p.rows * p.k * (p.d / cols_per_thread);
    return (threads + MX8_THREADS - 1) / MX8_THREADS;
}

hipError_t launch_sense_table_quantize(const Mx8TableParams &p, int dtype, hipStream_t stream) {
    const int64_t grid = mx8_grid(p, 8);
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    return with_dtype(dtype, [&](auto et) {
        hipLaunchKernelGGL((sense_table_quantize_kernel<decltype(et)>), dim3((unsigned)grid), dim3(MX8_THREADS), 0, stream, p);
        return hipGetLastError();
    });
}

hipError_t launch_sense_table_dequantize(const Mx8TableParams &p, int dtype, hipStream_t stream) {
    const int64_t grid = mx8_grid(p, 16);
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    return with_dtype(dtype, [&](auto et) {
        hipLaunchKernelGGL((sense_table_dequantize_kernel<decltype(et)>), dim3((unsigned)grid), dim3(MX8_THREADS), 0, stream, p);
        return hipGetLastError();
    });
}

}  // namespace bp
