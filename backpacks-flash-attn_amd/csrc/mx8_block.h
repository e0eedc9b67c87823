// The MXFP8 block rule of include/bp_hip.h ("MXFP8 sense table") as device functions, shared by the kernels of the 8-bit
// trunk KV cache (flash_decode_mx8.hip, kv_cache_mx8.hip).  A block is 32 consecutive columns: E4M3 elements and one E8M0
// scale byte, value = e4m3 * 2^(scale - 127).
#pragma once
#include "bp_common.h"

namespace bp {

// Scale byte of a block whose largest magnitude is `amax` (finite, >= 0).  The fp32 exponent field of amax IS
// floor(log2(amax)) + 127, so the byte is that field minus 8 (the E4M3 emax), held at 0 from below (a subnormal maximum has
// field 0 and lands there as well); an all-zero block takes 127.
BP_DEV int mx8_scale_byte(float amax) {
    const int field = (int)(as_u32(amax) >> 23);
    return amax == 0.f ? 127 : max(field - 8, 0);
}

// Four values of a block with scale byte s as four E4M3 bytes (lowest byte first): an exact power-of-two scaling, the clamp
// to +-448 in fp32, round to nearest even (two v_cvt_pk_fp8_f32).
BP_DEV uint32_t mx8_pack4(float a, float b, float c, float d, int s) {
    const int ex = 127 - s;
    const float v0 = fminf(fmaxf(ldexpf(a, ex), -448.f), 448.f), v1 = fminf(fmaxf(ldexpf(b, ex), -448.f), 448.f);
    const float v2 = fminf(fmaxf(ldexpf(c, ex), -448.f), 448.f), v3 = fminf(fmaxf(ldexpf(d, ex), -448.f), 448.f);
    int packed = __builtin_amdgcn_cvt_pk_fp8_f32(v0, v1, 0, false);
    packed = __builtin_amdgcn_cvt_pk_fp8_f32(v2, v3, packed, true);
    return (uint32_t)packed;
}

// The four E4M3 bytes of a word as fp32, unscaled (two v_cvt_pk_f32_fp8).  By value: see as_f32.
BP_DEV void mx8_unpack4(uint32_t w, float (&f)[4]) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const f32x2 up = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    f[0] = lo[0]; f[1] = lo[1]; f[2] = up[0]; f[3] = up[1];
}

// 16 E4M3 bytes of one block (half of it) with scale exponent ex = scale byte - 127 as 16 values of the 16-bit type E:
// elements 0..7 in lo, 8..15 in hi.  The instruction sequence of sense_table_dequantize_kernel (two v_cvt_pk_f32_fp8, an
// exact v_ldexp_f32 per element, one pack per pair), so the bits are bp_sense_table_dequantize's: exact wherever the type
// holds the value (always in bf16), round to nearest even elsewhere.
template <class E> BP_DEV void mx8_widen16(u32x4 w, int ex, u32x4 &lo, u32x4 &hi) {
    uint32_t o[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float f[4];
        const uint32_t wi = w[i];                 // by value: see as_f32
        mx8_unpack4(wi, f);
        o[2 * i] = E::pack2(ldexpf(f[0], ex), ldexpf(f[1], ex));
        o[2 * i + 1] = E::pack2(ldexpf(f[2], ex), ldexpf(f[3], ex));
    }
    lo = u32x4{o[0], o[1], o[2], o[3]};
    hi = u32x4{o[4], o[5], o[6], o[7]};
}

// 8 consecutive 16-bit elements as fp32, and their largest magnitude
template <class E> BP_DEV float mx8_unpack8_amax(u32x4 w, float *f) {
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t wi = w[i];                 // by value: see as_f32
        f[2 * i] = E::lo_f32(wi);
        f[2 * i + 1] = E::hi_f32(wi);
        amax = fmaxf(amax, fmaxf(fabsf(f[2 * i]), fabsf(f[2 * i + 1])));
    }
    return amax;
}

// Bytes of one position of the trunk's MXFP8 KV cache (include/bp_hip.h, "MXFP8 KV cache"): K and V elements, K and V
// scales, rounded up to 16
inline int64_t kv_mx8_row_bytes(int nheads, int head_dim) {
    const int64_t used = 2LL * nheads * head_dim + 2LL * nheads * (head_dim / 32);
    return (used + 15) / 16 * 16;
}

}  // namespace bp
