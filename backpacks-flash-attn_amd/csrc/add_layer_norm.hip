// Fused dropout + residual-add + LayerNorm forward for gfx950 (the reference's dropout_add_layer_norm:
// flash_attn/ops/layer_norm.py:102-230, csrc/layer_norm/ln_api.cpp:83-254, ln_fwd_kernels.cuh:20-162 -- no
// rowscale / colscale / subset):
//
//     x  = dropout(x0) / (1 - p) + x1     (x1 optional; x stored in the residual dtype, usually fp32)
//     z  = (x - mean(x)) * rsqrt(var(x) + eps) * gamma + beta      (fp32 math, stored in x0's dtype)
//
// x0 may be 16-bit or fp32 (under AMP the embedding output that enters the first LayerNorm is fp32 while the
// blocks' outputs are 16-bit; the reference's otype = itype rule, ln_api.cpp:104).  Dropout bits: bp_philox.h, one
// stream per call, counter (row, column / 4) -- the unit a lane owns; the backward regenerates them from the same
// two generator words instead of reading a mask back (the optional `dmask` output exists for callers that ask
// for it, layer_norm.py:207 return_dropout_mask).
//
// This is the memory-bound step on either side of every attention / MLP call:
// unfused it is three torch kernels (add -> cast -> LayerNorm) moving 15 KB per 768-wide row, fused it
// moves the algorithmic 9 KB once.  One wave per row, 4 rows per workgroup; a lane owns CH chunks of
// 4 consecutive columns (8-byte 16-bit loads, 16-byte fp32 loads, all coalesced), keeps them in
// registers for the two reductions (mean, then centred sum of squares as the reference does), and
// reduces across the wave with xor-shuffles.
#include "bp_common.h"
#include "bp_kernels.h"
#include "bp_philox.h"

namespace bp {

BP_DEV float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

template <class ET> BP_DEV float to_f32(uint16_t h);
template <> BP_DEV float to_f32<BF16>(uint16_t h) { return as_f32((uint32_t)h << 16); }
template <> BP_DEV float to_f32<F16>(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }

// Element widths are template parameters: one load / store form per instantiation.
template <class ET, bool F32> BP_DEV void load4(const void *base, int64_t idx, float (&v)[4]) {
    if constexpr (F32) {
        const u32x4 w = *reinterpret_cast<const u32x4 *>(static_cast<const char *>(base) + idx * 4);
        v[0] = as_f32(w[0]); v[1] = as_f32(w[1]); v[2] = as_f32(w[2]); v[3] = as_f32(w[3]);
    } else {
        const u32x2 w = *reinterpret_cast<const u32x2 *>(static_cast<const char *>(base) + idx * 2);
        v[0] = to_f32<ET>(w[0] & 0xffffu); v[1] = to_f32<ET>(w[0] >> 16);
        v[2] = to_f32<ET>(w[1] & 0xffffu); v[3] = to_f32<ET>(w[1] >> 16);
    }
}

template <class ET, bool F32> BP_DEV void store4(void *base, int64_t idx, const float (&v)[4]) {
    if constexpr (F32) {
        u32x4 w = {as_u32(v[0]), as_u32(v[1]), as_u32(v[2]), as_u32(v[3])};
        *reinterpret_cast<u32x4 *>(static_cast<char *>(base) + idx * 4) = w;
    } else {
        u32x2 w = {Elem<ET>::pack2(v[0], v[1]), Elem<ET>::pack2(v[2], v[3])};
        *reinterpret_cast<u32x2 *>(static_cast<char *>(base) + idx * 2) = w;
    }
}

// Streaming (non-temporal) forms for the forward's row data: every byte is touched once per launch.  The launcher picks
// which accesses carry the hint (see launch_flags).
template <class ET, bool F32, bool NT> BP_DEV void load4s(const void *base, int64_t idx, float (&v)[4]) {
    if constexpr (!NT) {
        load4<ET, F32>(base, idx, v);
    } else if constexpr (F32) {
        const u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(static_cast<const char *>(base) + idx * 4));
        v[0] = as_f32(w[0]); v[1] = as_f32(w[1]); v[2] = as_f32(w[2]); v[3] = as_f32(w[3]);
    } else {
        const u32x2 w = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(static_cast<const char *>(base) + idx * 2));
        v[0] = to_f32<ET>(w[0] & 0xffffu); v[1] = to_f32<ET>(w[0] >> 16);
        v[2] = to_f32<ET>(w[1] & 0xffffu); v[3] = to_f32<ET>(w[1] >> 16);
    }
}
template <class ET, bool F32, bool NT> BP_DEV void store4s(void *base, int64_t idx, const float (&v)[4]) {
    if constexpr (!NT) {
        store4<ET, F32>(base, idx, v);
    } else if constexpr (F32) {
        u32x4 w = {as_u32(v[0]), as_u32(v[1]), as_u32(v[2]), as_u32(v[3])};
        __builtin_nontemporal_store(w, reinterpret_cast<u32x4 *>(static_cast<char *>(base) + idx * 4));
    } else {
        u32x2 w = {Elem<ET>::pack2(v[0], v[1]), Elem<ET>::pack2(v[2], v[3])};
        __builtin_nontemporal_store(w, reinterpret_cast<u32x2 *>(static_cast<char *>(base) + idx * 2));
    }
}

// RES_F32: dtype of the residual stream (x1 in, x_out) is fp32, else ET.  W_F32: gamma/beta are fp32.
// NTL / NTS / NTZ: non-temporal loads of x0 and the residual / store of the residual / store of z
// SCALED: rowscale / colscale present (reference ln_fwd_kernels.cuh:99,123-125: x0 * rowscale[row], dropout, * colscale[col])
template <class ET, int CH, bool RES_F32, bool W_F32, bool NTL = false, bool NTS = false, bool NTZ = NTS, bool SCALED = false>
__global__ __launch_bounds__(256) void add_layer_norm_kernel(const LnParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const int64_t base = row * p.cols;
    const bool drop = p.drop_thr != 0u;
    DropoutStream rng = {0u, 0u};
    if (drop) rng = dropout_stream(p.rng_state, 0u);

    float x[CH][4];
    float sum = 0.f;
    float row_scale = 1.f;
    if (SCALED && p.rowscale != nullptr)
        row_scale = p.x0_f32 ? static_cast<const float *>(p.rowscale)[row]
                             : to_f32<ET>(static_cast<const uint16_t *>(p.rowscale)[row]);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int col = (c * 64 + lane) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) x[c][i] = 0.f;
        if (col < p.cols) {
            if (p.x0_f32) load4s<ET, true, NTL>(p.x0, base + col, x[c]);
            else load4s<ET, false, NTL>(p.x0, base + col, x[c]);
            if (SCALED) {
#pragma unroll
                for (int i = 0; i < 4; ++i) x[c][i] *= row_scale;
            }
            if (drop) {
                uint32_t lo, hi, m = 0u;
                dropout_bits4(rng, (uint32_t)row, (uint32_t)(col >> 2), lo, hi);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool keep = dropout_u16(lo, hi, i) < p.drop_thr;
                    x[c][i] = keep ? x[c][i] * p.drop_scale : 0.f;
                    m |= (keep ? 1u : 0u) << (8 * i);
                }
                if (p.dmask != nullptr) *reinterpret_cast<uint32_t *>(p.dmask + base + col) = m;
            }
            if (SCALED && p.colscale != nullptr) {
                float cs[4];
                load4<ET, W_F32>(p.colscale, col, cs);
#pragma unroll
                for (int i = 0; i < 4; ++i) x[c][i] *= cs[i];
            }
            if (p.x1 != nullptr) {
                float r[4];
                load4s<ET, RES_F32, NTL>(p.x1, base + col, r);
#pragma unroll
                for (int i = 0; i < 4; ++i) x[c][i] += r[i];
            }
            if (p.x_out != nullptr) {
                // stored in the residual dtype; z below is computed from the UNROUNDED fp32 sum, exactly as
                // the reference does (ln_fwd_kernels.cuh:131-133: x.data = x_ij; xf[...] = x_ij)
                store4s<ET, RES_F32, NTS>(p.x_out, base + col, x[c]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) sum += x[c][i];
        }
    }
    const float inv_n = 1.f / (float)p.cols;
    const float mu = wave_sum(sum) * inv_n;
    float m2 = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int col = (c * 64 + lane) * 4;
        if (col < p.cols) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float d = x[c][i] - mu;
                m2 += d * d;
            }
        }
    }
    const float rs = rsqrtf(wave_sum(m2) * inv_n + p.eps);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int col = (c * 64 + lane) * 4;
        if (col < p.cols) {
            float g[4], b[4], z[4];
            load4<ET, W_F32>(p.gamma, col, g);
            load4<ET, W_F32>(p.beta, col, b);
#pragma unroll
            for (int i = 0; i < 4; ++i) z[i] = (x[c][i] - mu) * rs * g[i] + b[i];
            if (p.x0_f32) store4s<ET, true, NTZ>(p.z, base + col, z);
            else store4s<ET, false, NTZ>(p.z, base + col, z);
        }
    }
}

hipError_t launch_add_layer_norm(const LnParams &p, int dtype, hipStream_t stream) {
    const dim3 g((unsigned)((p.rows + 3) / 4)), t(256);
    const int chunks = (p.cols + 255) / 256;
    // non-temporal loads and residual store: x0 and the incoming residual are read once and never again, the outgoing
    // residual is next read a GEMM and an attention launch later; z stays cacheable for the GEMM that follows
    // (profiles/r04_d_ab_layernorm_nontemporal.jsonl)
    constexpr bool NTL = true, NTS = true, NTZ = false;
    // residual dtype: x1's when given, else x_out's (the API guarantees they agree when both exist)
    const bool res_f32 = (p.x1 != nullptr) ? p.x1_f32 != 0 : p.xo_f32 != 0;
    const bool scaled = p.rowscale != nullptr || p.colscale != nullptr;
    return with_dtype(dtype, [&](auto et) {
        return with_flag(res_f32, [&](auto res) {
            return with_flag(p.w_f32 != 0, [&](auto w) {
                return with_flag(scaled, [&](auto sc) {
                    return with_bound<1, 2, 3, 4, 6, 8, 12, 16, 24, 32>(chunks, hipErrorInvalidValue, [&](auto ch) {
                        hipLaunchKernelGGL((add_layer_norm_kernel<decltype(et), ch, res, w, NTL, NTS, NTZ, sc>), g, t, 0,
                                           stream, p);
                        return hipGetLastError();
                    });
                });
            });
        });
    });
}

// =====================================================================================================
// Inference chain (bp_add_layer_norm_chain): the forms a chain of pre-norm blocks runs in eval() without an autograd
// graph.  16-bit x0 / x0b / z, fp32 residual stream, no dropout, no scales, no mask -- and which operands exist is a
// template parameter, not a branch.  In the kernel above every load sits behind a run-time branch and in front of a store it
// may alias, so a wave's loads go out one after the other, each waiting for the one before (six round trips per 768-wide
// row); here a wave first issues EVERY load of its row (phase 1), then does the arithmetic of the kernel above in the order
// of the kernel above (phase 2: the same bits), then stores.
//   EMB   x0 is not read but rebuilt from the embedding tables: word[tok[row]] (+ pos[position of row], added in fp32 and
//         rounded once to ET, as torch's 16-bit add rounds); ids clamped to the tables as unsigned values; table rows stay
//         cacheable (they repeat), the row streams are non-temporal as above
//   X0B   a second 16-bit branch output joins last: x = (x0 + x1) + x0b -- what two launches compute when the first
//         stores x0 + x1 exactly in fp32 and the second adds its own x0 to that, without the fp32 round trip
//   X1 / XOUT   residual in / out present.  x_out may be x1 itself: a lane's store of an element depends on its own load
//         of that element, and no other lane touches it.
// =====================================================================================================
template <bool NT> BP_DEV u32x2 ldg8(const void *base, int64_t idx) {   // four 16-bit elements from element idx
    const u32x2 *at = reinterpret_cast<const u32x2 *>(static_cast<const char *>(base) + idx * 2);
    if constexpr (NT) return __builtin_nontemporal_load(at);
    else return *at;
}
template <class ET> BP_DEV void unpack4(u32x2 w, float (&v)[4]) {
    v[0] = to_f32<ET>(w[0] & 0xffffu); v[1] = to_f32<ET>(w[0] >> 16);
    v[2] = to_f32<ET>(w[1] & 0xffffu); v[3] = to_f32<ET>(w[1] >> 16);
}

template <class ET, int CH, bool W_F32, bool EMB, bool X0B, bool X1, bool XOUT>
__global__ __launch_bounds__(256) void add_layer_norm_chain_kernel(const LnParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const int64_t base = row * p.cols;
    const bool has_pos = EMB && p.wpe != nullptr;
    int64_t tok_base = 0, pos_base = 0;
    if constexpr (EMB) {
        tok_base = (int64_t)min((uint64_t)p.tok[row], (uint64_t)p.last_tok) * p.cols;
        if (has_pos) {
            const uint32_t at = (uint32_t)row % p.pos_len;   // (rows < 2^32)
            pos_base = (int64_t)min((uint64_t)(p.pos != nullptr ? p.pos[at] : (int64_t)at), (uint64_t)p.last_pos) * p.cols;
        }
    }

    // phase 1: every load of the row in flight
    u32x2 a[CH], e[CH], b2[CH];
    u32x4 r[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int col = (c * 64 + lane) * 4;
        a[c] = u32x2{0u, 0u}; e[c] = u32x2{0u, 0u}; b2[c] = u32x2{0u, 0u}; r[c] = u32x4{0u, 0u, 0u, 0u};
        if (col < p.cols) {
            if constexpr (EMB) {
                a[c] = ldg8<false>(p.wte, tok_base + col);
                if (has_pos) e[c] = ldg8<false>(p.wpe, pos_base + col);
            } else {
                a[c] = ldg8<true>(p.x0, base + col);
            }
            if constexpr (X1)
                r[c] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(static_cast<const char *>(p.x1) + (base + col) * 4));
            if constexpr (X0B) b2[c] = ldg8<true>(p.x0b, base + col);
        }
    }

    // phase 2: the sums, element by element in the order of add_layer_norm_kernel
    float x[CH][4];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int col = (c * 64 + lane) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) x[c][i] = 0.f;
        if (col < p.cols) {
            unpack4<ET>(a[c], x[c]);
            if (has_pos) {
                float q[4];
                unpack4<ET>(e[c], q);
#pragma unroll
                for (int i = 0; i < 4; ++i) x[c][i] = to_f32<ET>(Elem<ET>::from_float(x[c][i] + q[i]));
            }
            if constexpr (X1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) x[c][i] += as_f32(r[c][i]);
            }
            if constexpr (X0B) {
                float q[4];
                unpack4<ET>(b2[c], q);
#pragma unroll
                for (int i = 0; i < 4; ++i) x[c][i] += q[i];
            }
            if constexpr (XOUT) store4s<ET, true, true>(p.x_out, base + col, x[c]);
#pragma unroll
            for (int i = 0; i < 4; ++i) sum += x[c][i];
        }
    }
    const float inv_n = 1.f / (float)p.cols;
    const float mu = wave_sum(sum) * inv_n;
    float m2 = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int col = (c * 64 + lane) * 4;
        if (col < p.cols) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float d = x[c][i] - mu;
                m2 += d * d;
            }
        }
    }
    const float rs = rsqrtf(wave_sum(m2) * inv_n + p.eps);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int col = (c * 64 + lane) * 4;
        if (col < p.cols) {
            float g[4], b[4], z[4];
            load4<ET, W_F32>(p.gamma, col, g);
            load4<ET, W_F32>(p.beta, col, b);
#pragma unroll
            for (int i = 0; i < 4; ++i) z[i] = (x[c][i] - mu) * rs * g[i] + b[i];
            store4s<ET, false, false>(p.z, base + col, z);      // z stays cacheable for the GEMM that follows
        }
    }
}

// cols <= 2048 (the model widths): wider rows are hipErrorNotSupported
hipError_t launch_add_layer_norm_chain(const LnParams &p, int dtype, hipStream_t stream) {
    const dim3 g((unsigned)((p.rows + 3) / 4)), t(256);
    const int chunks = (p.cols + 255) / 256;
    const bool emb = p.wte != nullptr;
    return with_dtype(dtype, [&](auto et) {
        return with_flag(p.w_f32 != 0, [&](auto w) {
            return with_flag(p.x0b != nullptr, [&](auto x0b) {
                return with_flag(p.x_out != nullptr, [&](auto xout) {
                    return with_bound<1, 2, 3, 4, 6, 8>(chunks, hipErrorNotSupported, [&](auto ch) {
                        using ET = decltype(et);
                        if (emb) {   // (bp_api.hip: the embedding source comes without a residual input)
                            hipLaunchKernelGGL((add_layer_norm_chain_kernel<ET, ch, w, true, x0b, false, xout>), g, t, 0, stream, p);
                            return hipGetLastError();
                        }
                        return with_flag(p.x1 != nullptr, [&](auto x1) {
                            hipLaunchKernelGGL((add_layer_norm_chain_kernel<ET, ch, w, false, x0b, x1, xout>), g, t, 0, stream, p);
                            return hipGetLastError();
                        });
                    });
                });
            });
        });
    });
}

// =====================================================================================================
// Backward (reference: DropoutAddLayerNormFn.backward, flash_attn/ops/layer_norm.py:131-152;
// csrc/layer_norm/ln_bwd_kernels.cuh, eval path: no dropout / rowscale / colscale)
//
//     xhat = (x - mu) rs            dy = dz * gamma
//     dx   = rs (dy - mean(dy) - xhat mean(dy xhat)) + dx_in         (dx0 = dx1 = dx: x = x0 + x1)
//     dgamma = sum_rows dz xhat     dbeta = sum_rows dz
//
// mu and rs are recomputed from the saved x (read anyway), so the forward stores no statistics.  One wave
// per row, each wave strides over rows and keeps its lanes' columns of dgamma / dbeta in registers; the
// four waves of a workgroup fold theirs through LDS into one partial row of the workspace and a second
// small kernel sums the partial rows (deterministic: no atomics).
// =====================================================================================================
BP_DEV void wave_sum2(float &a, float &b) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        a += __shfl_xor(a, m);
        b += __shfl_xor(b, m);
    }
}

// SCALED: the forward had a rowscale and / or a colscale: dx0 = dx * rowscale * mask / (1 - p) * colscale,
// dcolscale = sum over rows of dx * rowscale * mask / (1 - p) * x0 (reference ln_bwd_kernels.cuh:183-195)
template <class ET, int CH, bool RES_F32, bool W_F32, bool SCALED = false>
__global__ __launch_bounds__(256) void add_layer_norm_bwd_kernel(const LnBwdParams p) {
    __shared__ float fold[SCALED ? 3 : 2][CH * 256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_n = 1.f / (float)p.cols;
    const bool drop = p.drop_thr != 0u;
    DropoutStream rng = {0u, 0u};
    if (drop) rng = dropout_stream(p.rng_state, 0u);

    float g[CH][4], dg[CH][4], db[CH][4];
    float cs[SCALED ? CH : 1][4], dcs[SCALED ? CH : 1][4];
    const bool has_cs = SCALED && p.colscale != nullptr;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int col = (c * 64 + lane) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) { g[c][i] = 0.f; dg[c][i] = 0.f; db[c][i] = 0.f; }
        if (SCALED) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { cs[c][i] = 1.f; dcs[c][i] = 0.f; }
        }
        if (col < p.cols) {
            load4<ET, W_F32>(p.gamma, col, g[c]);
            if (has_cs) load4<ET, W_F32>(p.colscale, col, cs[c]);
        }
    }

    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < p.rows; row += (int64_t)p.n_wg * 4) {
        const int64_t base = row * p.cols;
        float x[CH][4], dy[CH][4];
        float sum = 0.f;
        float row_scale = 1.f;
        if (SCALED && p.rowscale != nullptr)
            row_scale = p.x0_f32 ? static_cast<const float *>(p.rowscale)[row]
                                 : to_f32<ET>(static_cast<const uint16_t *>(p.rowscale)[row]);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int col = (c * 64 + lane) * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) { x[c][i] = 0.f; dy[c][i] = 0.f; }
            if (col < p.cols) {
                load4<ET, RES_F32>(p.x, base + col, x[c]);
                if (p.x0_f32) load4<ET, true>(p.dz, base + col, dy[c]);      // dz for now (z has x0's dtype)
                else load4<ET, false>(p.dz, base + col, dy[c]);
#pragma unroll
                for (int i = 0; i < 4; ++i) sum += x[c][i];
            }
        }
        const float mu = wave_sum(sum) * inv_n;
        float m2 = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int col = (c * 64 + lane) * 4;
            if (col < p.cols) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float d = x[c][i] - mu;
                    m2 += d * d;
                }
            }
        }
        const float rs = rsqrtf(wave_sum(m2) * inv_n + p.eps);
        float s1 = 0.f, s2 = 0.f;   // sum dy, sum dy * xhat
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int col = (c * 64 + lane) * 4;
            if (col < p.cols) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float xhat = (x[c][i] - mu) * rs;
                    const float dz = dy[c][i];
                    dg[c][i] += dz * xhat;
                    db[c][i] += dz;
                    const float d = dz * g[c][i];
                    s1 += d;
                    s2 += d * xhat;
                    x[c][i] = xhat;
                    dy[c][i] = d;
                }
            }
        }
        wave_sum2(s1, s2);
        const float c1 = s2 * inv_n, c2 = s1 * inv_n;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int col = (c * 64 + lane) * 4;
            if (col < p.cols) {
                float dx[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) dx[i] = rs * (dy[c][i] - c2 - x[c][i] * c1);
                if (p.dx_in != nullptr) {
                    float r[4];
                    load4<ET, RES_F32>(p.dx_in, base + col, r);
#pragma unroll
                    for (int i = 0; i < 4; ++i) dx[i] += r[i];
                }
                if (p.dx1 != nullptr) store4<ET, RES_F32>(p.dx1, base + col, dx);
                if (SCALED) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) dx[i] *= row_scale;
                }
                if (drop) {   // x0 entered through dropout: its gradient passes the same mask and scale
                    uint32_t lo, hi;
                    dropout_bits4(rng, (uint32_t)row, (uint32_t)(col >> 2), lo, hi);
#pragma unroll
                    for (int i = 0; i < 4; ++i) dx[i] = dropout_u16(lo, hi, i) < p.drop_thr ? dx[i] * p.drop_scale : 0.f;
                }
                if (has_cs) {
                    float x0v[4];
                    if (p.x0_f32) load4<ET, true>(p.x0, base + col, x0v);
                    else load4<ET, false>(p.x0, base + col, x0v);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        dcs[c][i] += dx[i] * x0v[i];
                        dx[i] *= cs[c][i];
                    }
                }
                if (p.x0_f32) store4<ET, true>(p.dx0, base + col, dx);
                else store4<ET, false>(p.dx0, base + col, dx);
            }
        }
    }

    // fold the four waves' column sums (wave after wave: fixed order) and publish one partial row
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int c = 0; c < CH; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int idx = (c * 64 + lane) * 4 + i;
                    fold[0][idx] = (w == 0 ? 0.f : fold[0][idx]) + dg[c][i];
                    fold[1][idx] = (w == 0 ? 0.f : fold[1][idx]) + db[c][i];
                    if (SCALED) fold[2][idx] = (w == 0 ? 0.f : fold[2][idx]) + dcs[c][i];
                }
        }
        __syncthreads();
    }
    for (int col = threadIdx.x; col < p.cols; col += 256) {
        p.ws[(int64_t)blockIdx.x * p.cols + col] = fold[0][col];
        p.ws[((int64_t)kLnBwdMaxWg + blockIdx.x) * p.cols + col] = fold[1][col];
        if (SCALED && has_cs) p.ws[((int64_t)2 * kLnBwdMaxWg + blockIdx.x) * p.cols + col] = fold[2][col];
    }
}

// Sum of the partial rows: 64 columns per workgroup, 16 row slices per column (1024 threads) so that the
// serial part is n_wg / 16 coalesced loads per thread, then a fixed-order fold through LDS.
template <class ET, bool W_F32>
__global__ __launch_bounds__(1024) void ln_bwd_reduce_kernel(const LnBwdParams p) {
    __shared__ float part[3][16][64];
    const int c = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + c;
    const bool has_cs = p.dcolscale != nullptr;
    float a = 0.f, b = 0.f, e = 0.f;
    if (col < p.cols) {
        for (int r = slice; r < p.n_wg; r += 16) {
            a += p.ws[(int64_t)r * p.cols + col];
            b += p.ws[((int64_t)kLnBwdMaxWg + r) * p.cols + col];
            if (has_cs) e += p.ws[((int64_t)2 * kLnBwdMaxWg + r) * p.cols + col];
        }
    }
    part[0][slice][c] = a;
    part[1][slice][c] = b;
    part[2][slice][c] = e;
    __syncthreads();
    if (slice != 0 || col >= p.cols) return;
    for (int s = 1; s < 16; ++s) {
        a += part[0][s][c];
        b += part[1][s][c];
        e += part[2][s][c];
    }
    if (W_F32) {
        static_cast<float *>(p.dgamma)[col] = a;
        static_cast<float *>(p.dbeta)[col] = b;
        if (has_cs) static_cast<float *>(p.dcolscale)[col] = e;
    } else {
        static_cast<uint16_t *>(p.dgamma)[col] = Elem<ET>::from_float(a);
        static_cast<uint16_t *>(p.dbeta)[col] = Elem<ET>::from_float(b);
        if (has_cs) static_cast<uint16_t *>(p.dcolscale)[col] = Elem<ET>::from_float(e);
    }
}

// cols % 4 == 0 and <= 2048 (the model widths 384 / 640 / 768 and up); larger rows: hipErrorNotSupported
hipError_t launch_add_layer_norm_bwd(const LnBwdParams &p, int dtype, hipStream_t stream) {
    const dim3 g((unsigned)p.n_wg), t(256);
    const int chunks = (p.cols + 255) / 256;
    const bool scaled = p.rowscale != nullptr || p.colscale != nullptr;
    return with_dtype(dtype, [&](auto et) {
        return with_flag(p.res_f32 != 0, [&](auto res) {
            return with_flag(p.w_f32 != 0, [&](auto w) {
                using ET = decltype(et);
                const hipError_t e = with_flag(scaled, [&](auto sc) {
                    return with_bound<1, 2, 3, 4, 6, 8>(chunks, hipErrorNotSupported, [&](auto ch) {
                        hipLaunchKernelGGL((add_layer_norm_bwd_kernel<ET, ch, res, w, sc>), g, t, 0, stream, p);
                        return hipGetLastError();
                    });
                });
                if (e != hipSuccess) return e;
                hipLaunchKernelGGL((ln_bwd_reduce_kernel<ET, w>), dim3((p.cols + 63) / 64), dim3(1024), 0, stream, p);
                return hipGetLastError();
            });
        });
    });
}

}  // namespace bp
