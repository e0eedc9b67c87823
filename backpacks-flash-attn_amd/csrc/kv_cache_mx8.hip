// bp_kv_cache_quantize: the prefill's fill of the MXFP8 KV cache (include/bp_hip.h, "MXFP8 KV cache") -- the K/V of the
// prompts, a strided 16-bit view (B, S, 2, H, D) or a packed one (total, 2, H, D) with cu_seqlens, quantised into rows
// [b, 0:len_b) of the byte cache.  One pass, no LDS, no atomics: pure bandwidth.
//
// Grid (position chunks, batch).  4 lanes own one block of 32 columns of one (position, K or V, head), 8 columns each (one
// 16-byte load), as in sense_table_quantize_kernel: the block maximum goes round the group in two lane exchanges, every
// lane stores its 8 bytes as one word and lane 0 of the group the scale byte (mx8_block.h has the rule).  Positions at or
// behind len_b and the pad bytes of a row are not written.  cu_seqlens is read here and nowhere on the host, and it is not
// trusted: a negative length counts as 0, a length is clamped to min(max_seqlen, max_positions), and a source row outside
// [0, total_rows) is skipped.
#include "bp_common.h"
#include "bp_kernels.h"
#include "mx8_block.h"

namespace bp {

constexpr int KVQ_THREADS = 256;

template <class ET>
__global__ __launch_bounds__(KVQ_THREADS) void kv_cache_quantize_kernel(KvQuantParams p) {
    using E = Elem<ET>;
    const int b = blockIdx.y;
    int64_t first = 0;
    int len = p.limit;
    if (p.cu != nullptr) {
        first = p.cu[b];
        const int64_t l = (int64_t)p.cu[b + 1] - first;
        len = l < 0 ? 0 : (l < p.limit ? (int)l : p.limit);
    }
    const int nb = p.d >> 5;                      // blocks of a head's row
    const int per_pos = 8 * p.h * nb;             // threads of a position: 2 (K, V) x H x nb blocks x 4 lanes
    const int64_t t = (int64_t)blockIdx.x * KVQ_THREADS + threadIdx.x;
    const int64_t pos = t / per_pos;
    if (pos >= len) return;                       // whole groups of 4 lanes leave together (per_pos % 4 == 0)
    const int rem = (int)(t - pos * per_pos);
    const int li = rem & 3, blk = rem >> 2;
    const int hb = p.h * nb;
    const int which = blk / hb, r2 = blk - which * hb;
    const int head = r2 / nb, bi = r2 - head * nb;

    const uint16_t *src = static_cast<const uint16_t *>(p.kv);
    if (p.cu != nullptr) {
        const int64_t row = first + pos;
        if (row < 0 || row >= p.total_rows) return;   // the same for the 4 lanes of a group
        src += row * p.kv_rs;
    } else {
        src += b * p.kv_bs + pos * p.kv_rs;
    }
    src += which * p.kv_ts + head * p.kv_hs + bi * 32 + li * 8;
    float f[8];
    float amax = mx8_unpack8_amax<E>(ld_global_16B(src), f);
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    const int s = mx8_scale_byte(amax);
    uint8_t *row = p.cache + b * p.c_bs + pos * p.c_rs;
    const int hd = p.h * p.d;
    *reinterpret_cast<u32x2 *>(row + which * hd + head * p.d + bi * 32 + li * 8) =
        u32x2{mx8_pack4(f[0], f[1], f[2], f[3], s), mx8_pack4(f[4], f[5], f[6], f[7], s)};
    if (li == 0) row[2 * hd + (which * p.h + head) * nb + bi] = (uint8_t)s;
}

hipError_t launch_kv_cache_quantize(const KvQuantParams &p, int dtype, hipStream_t stream) {
    if (p.limit <= 0) return hipSuccess;          // nothing may be written
    const int64_t threads = (int64_t)p.limit * 8 * p.h * (p.d >> 5);
    const int64_t grid = (threads + KVQ_THREADS - 1) / KVQ_THREADS;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    return with_dtype(dtype, [&](auto et) {
        hipLaunchKernelGGL((kv_cache_quantize_kernel<decltype(et)>), dim3((unsigned)grid, (unsigned)p.b), dim3(KVQ_THREADS), 0,
                           stream, p);
        return hipGetLastError();
    });
}

}  // namespace bp
