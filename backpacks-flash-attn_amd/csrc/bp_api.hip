// C ABI of libbackpack_hip.so (see include/bp_hip.h for the contract of every entry point).
// Host-side only: argument validation in the spirit of mha_fwd's TORCH_CHECKs
// (reference csrc/flash_attn/fmha_api.cpp:206-252), parameter packing, kernel dispatch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <initializer_list>

#include "../../include/bp_hip.h"
#include "bp_common.h"
#include "bp_kernels.h"

namespace {

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned16(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (!aligned16(p)) return false;
    return true;
}
// optional operands: only the ones given (non-NULL) must be aligned
inline bool aligned16_or_null(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (p != nullptr && !aligned16(p)) return false;
    return true;
}
inline bool mult8(int64_t x) { return (x & 7) == 0; }
inline bool strides8(std::initializer_list<int64_t> strides) {
    for (int64_t s : strides)
        if (!mult8(s)) return false;
    return true;
}
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

inline bool scale_ok(float s) { return isfinite(s) && s > 0.f; }
inline int launch_status(hipError_t e) { return e == hipSuccess ? BP_OK : BP_ERR_LAUNCH; }

// queue_ws == NULL means "a record of the library's own ring" (include/bp_hip.h).  A graph captured that way would
// replay on a record every other NULL launch also cycles through, so it is refused instead of documented as unsafe.
inline bool null_queue_ws_on_capturing_stream(const void *queue_ws, hipStream_t st) {
    if (queue_ws != nullptr) return false;
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &status) != hipSuccess) return false;
    return status != hipStreamCaptureStatusNone;
}

// dropout argument check shared by the *_dropout entry points: p in [0, 1), a generator state when p > 0.
// thr: keep iff a 16-bit uniform < thr (bp_philox.h); 0 = dropout off.
inline bool dropout_args(float p, const uint64_t *rng_state, uint32_t &thr, float &rp_keep) {
    thr = 0u; rp_keep = 1.f;
    if (!(p >= 0.f && p < 1.f)) return false;
    if (p == 0.f) return true;
    if (rng_state == nullptr) return false;
    long t = lrintf((1.f - p) * 65536.f);
    thr = (uint32_t)(t < 1 ? 1 : t > 65535 ? 65535 : t);
    // rescale by the reference's 1 / (1 - p) (fmha_api.cpp:303 `rp_dropout`, ln_api.cpp:149), not by the keep rate the
    // 16-bit threshold realises (thr / 65536): the two differ by <= 2^-17 / (1 - p) relative, which the reference's own
    // fp32 LayerNorm test resolves (tests/ops/test_dropout_layer_norm.py compares with x0 * mask / (1 - p); 65536 / thr
    // was tried in round 3 and failed it by 8e-6 relative)
    rp_keep = 1.f / (1.f - p);
    return true;
}

// 16-byte friendly shapes take the LDS-DMA ring kernel; anything else (odd head dims, unaligned
// views) the register-staged kernel with its element-wise loader.
inline hipError_t dispatch_flash(const bp::FlashParams &p, int dtype, bool vec, hipStream_t st) {
    return vec ? bp::launch_flash_fwd_dma(p, dtype, st) : bp::launch_flash_fwd(p, dtype, st);
}

// The q and k halves of a (B, S, 2, k, d_k) qk operand are 16-byte friendly.
inline bool qk_vec16(int d_k, const uint16_t *q, int64_t two_stride, int64_t bs, int64_t rs, int64_t ss) {
    return d_k % 8 == 0 && aligned16({q, q + two_stride}) && strides8({bs, rs, ss});
}

// The kernel family of every sense entry point (LSE pre-pass, alpha, mix, gathering mix).  Senses up to 128 wide take
// the narrow kernels (flash_fwd*.hip, attn_probs.hip, sense_mix*.hip), wider ones the wide kernels (sense_wide*.hip).
// Within each, 16-byte friendly operands (vec_qk, vec_c) take the LDS-DMA ring kernel, anything else the
// register-staged kernel with its element-wise loader; the wide ring kernels take the reference's two few-sense
// configurations only (sense_wide_dma_takes).  d_out == 0: no content operand (the LSE pre-pass, alpha).  gather: the
// gathering mix, which has no staged kernels (its caller refuses those shapes) and a tighter sequence limit of its own.
enum class SenseKernel { NarrowRing, NarrowStaged, WideRing, WideStaged };

inline SenseKernel sense_route(int d_k, int seqlen, int d_out, bool vec_qk, bool vec_c, bool weighted, bool gather) {
    if (d_k > 128)
        return bp::sense_wide_dma_takes(seqlen, d_k, d_out, vec_qk, vec_c, weighted) ? SenseKernel::WideRing
                                                                                       : SenseKernel::WideStaged;
    // the mix ring kernels number their jobs group * kMixMaxTiles + tile (mix_ring.h): tiles of 256 queries
    const bool ring_fits = d_out == 0 || gather || seqlen <= bp::kMixMaxTiles * 256;
    return vec_qk && vec_c && ring_fits ? SenseKernel::NarrowRing : SenseKernel::NarrowStaged;
}

inline bool is_wide(SenseKernel k) { return k == SenseKernel::WideRing || k == SenseKernel::WideStaged; }

// Parameters of the forward mix kernels; the weighted form adds key weights, the gathering form a row index.
inline bp::MixParams mix_params(const void *qk, const void *content, void *out, float *lse_ws,
                                int batch, int seqlen, int nsenses, int d_k, int d_out,
                                int64_t qk_bs, int64_t qk_rs, int64_t qk_two, int64_t qk_ss,
                                int64_t c_bs, int64_t c_rs, int64_t c_ss, int64_t o_bs, int64_t o_rs,
                                float softmax_scale, void *queue_ws) {
    const uint16_t *qp = static_cast<const uint16_t *>(qk);
    bp::MixParams p{};
    p.q = qp; p.k = qp + qk_two; p.c = content; p.o = out; p.lse = lse_ws;
    p.qk_bs = qk_bs; p.qk_rs = qk_rs; p.qk_ss = qk_ss;
    p.c_bs = c_bs; p.c_rs = c_rs; p.c_ss = c_ss;
    p.o_bs = o_bs; p.o_rs = o_rs;
    p.lse_stride = round_up(seqlen, 16);
    p.b = batch; p.s = seqlen; p.nsenses = nsenses; p.dk = d_k; p.dout = d_out;
    p.n_qtiles = (seqlen + 255) / 256;
    p.n_chunks = (d_out + 255) / 256;
    p.scale_log2e = softmax_scale * bp::kLog2e;
    p.queues = static_cast<bp::MixQueues *>(queue_ws);
    return p;
}

}  // namespace

extern "C" {

const char *bp_strerror(int code) {
    switch (code) {
        case BP_OK: return "ok";
        case BP_ERR_DTYPE: return "unsupported dtype (expected fp16 or bf16)";
        case BP_ERR_HEAD_DIM: return "head dimension must be in [1, 128] (sense width of bp_sense_lse / _alpha / _mix: [1, 640])";
        case BP_ERR_SHAPE: return "invalid shape or null pointer";
        case BP_ERR_SCALE: return "softmax_scale must be finite and > 0";
        case BP_ERR_LAUNCH: return "HIP kernel launch failed";
        case BP_ERR_DOUT: return "d_out must be >= 1";
        case BP_ERR_DROPOUT: return "dropout: p must be in [0, 1), rng_state non-NULL when p > 0, 16-byte friendly shapes only";
        case BP_ERR_QUEUE_WS: return "queue_ws must be caller-owned (non-NULL) while the stream is being captured";
        case BP_ERR_WORKSPACE: return "workspace smaller than the *_ws_floats() query of this entry point";
        case BP_ERR_SAMPLING: return "token sampling: top_p must be in (0, 1], rng_state non-NULL when do_sample; repetition_penalty finite and > 0 and, "
                                     "unless 1, with sequences; an eos_token_id with finished flags; finite frequency / presence penalties and, like n-gram "
                                     "blocking, with sequences; a non-NULL aligned suppress_ids when n_suppress > 0; phrase lists with non-NULL ids and offsets and "
                                     "with sequences, stop phrases with finished flags";
        case BP_ERR_GEMM: return "a call into hipBLASLt or the HIP runtime failed";
        default: return "unknown error";
    }
}

int bp_abi_version(void) { return BP_ABI_VERSION; }

int bp_build_flags(void) {
    int flags = 0;
#ifdef BP_FWD_WHATIF
    flags |= 1;
#endif
#if defined(BP_BWD_WHATIF) && BP_BWD_WHATIF != 0
    flags |= 2;
#endif
    return flags;
}

int bp_flash_fwd(const void *q, const void *k, const void *v, void *out, float *softmax_lse,
                 const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k,
                 int batch, int nheads, int head_dim, int max_seqlen_q, int max_seqlen_k,
                 int64_t q_row_stride, int64_t q_head_stride,
                 int64_t k_row_stride, int64_t k_head_stride,
                 int64_t v_row_stride, int64_t v_head_stride,
                 int64_t o_row_stride, int64_t o_head_stride,
                 int64_t lse_stride, float softmax_scale, int is_causal, int dtype,
                 bp_stream_t stream) {
    return bp_flash_fwd_dropout(q, k, v, out, softmax_lse, cu_seqlens_q, cu_seqlens_k, batch, nheads, head_dim,
                                max_seqlen_q, max_seqlen_k, q_row_stride, q_head_stride, k_row_stride,
                                k_head_stride, v_row_stride, v_head_stride, o_row_stride, o_head_stride,
                                lse_stride, softmax_scale, is_causal, dtype, 0.f, nullptr, stream);
}

int bp_flash_fwd_dropout(const void *q, const void *k, const void *v, void *out, float *softmax_lse,
                         const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k,
                         int batch, int nheads, int head_dim, int max_seqlen_q, int max_seqlen_k,
                         int64_t q_row_stride, int64_t q_head_stride,
                         int64_t k_row_stride, int64_t k_head_stride,
                         int64_t v_row_stride, int64_t v_head_stride,
                         int64_t o_row_stride, int64_t o_head_stride,
                         int64_t lse_stride, float softmax_scale, int is_causal, int dtype,
                         float p_dropout, const uint64_t *rng_state, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (head_dim < 1 || head_dim > 128) return BP_ERR_HEAD_DIM;
    if (batch <= 0 || nheads <= 0 || max_seqlen_q <= 0 || max_seqlen_k < 0) return BP_ERR_SHAPE;
    if (q == nullptr || k == nullptr || softmax_lse == nullptr) return BP_ERR_SHAPE;
    if ((v == nullptr) != (out == nullptr)) return BP_ERR_SHAPE;
    if ((cu_seqlens_q == nullptr) != (cu_seqlens_k == nullptr)) return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;

    bp::FlashParams p{};
    p.q = q; p.k = k; p.v = v; p.o = out; p.lse = softmax_lse;
    p.cu_q = cu_seqlens_q; p.cu_k = cu_seqlens_k;
    p.q_rs = q_row_stride; p.q_hs = q_head_stride;
    p.k_rs = k_row_stride; p.k_hs = k_head_stride;
    p.v_rs = v_row_stride; p.v_hs = v_head_stride;
    p.o_rs = o_row_stride; p.o_hs = o_head_stride;
    p.q_bs = (int64_t)max_seqlen_q * q_row_stride; p.o_bs = (int64_t)max_seqlen_q * o_row_stride;
    p.k_bs = (int64_t)max_seqlen_k * k_row_stride; p.v_bs = (int64_t)max_seqlen_k * v_row_stride;
    p.lse_stride = lse_stride;
    p.b = batch; p.h = nheads; p.d = head_dim;
    p.max_sq = max_seqlen_q; p.max_sk = max_seqlen_k;
    p.n_qtiles = (max_seqlen_q + 127) / 128;
    p.causal = is_causal ? 1 : 0;
    p.pair = (p.causal && p.n_qtiles > 1) ? 1 : 0;
    p.scale_log2e = softmax_scale * bp::kLog2e;
    p.rng_state = rng_state;
    if (!dropout_args(p_dropout, rng_state, p.drop_thr, p.drop_scale)) return BP_ERR_DROPOUT;
    if (p.drop_thr != 0u && v == nullptr) return BP_ERR_DROPOUT;   // dropout acts on P V: nothing to drop in an LSE pass

    bool vec = head_dim % 8 == 0 && aligned16({q, k}) &&
               strides8({q_row_stride, q_head_stride, k_row_stride, k_head_stride});
    if (v != nullptr)
        vec = vec && aligned16({v, out}) && strides8({v_row_stride, v_head_stride, o_row_stride, o_head_stride});
    if (p.drop_thr != 0u && !vec) return BP_ERR_DROPOUT;   // the element-wise loader path has no dropout
    return launch_status(dispatch_flash(p, dtype, vec, static_cast<hipStream_t>(stream)));
}

int bp_attn_probs(const void *q, const void *k, const float *softmax_lse, void *probs,
                  int batch, int nheads, int head_dim, int seqlen_q, int seqlen_k,
                  int64_t q_batch_stride, int64_t q_row_stride, int64_t q_head_stride,
                  int64_t k_batch_stride, int64_t k_row_stride, int64_t k_head_stride,
                  int64_t lse_stride,
                  int64_t p_batch_stride, int64_t p_head_stride, int64_t p_row_stride,
                  float softmax_scale, int is_causal, int dtype, bp_stream_t stream) {
    return bp_attn_probs_dropout(q, k, softmax_lse, probs, batch, nheads, head_dim, seqlen_q, seqlen_k,
                                 q_batch_stride, q_row_stride, q_head_stride, k_batch_stride, k_row_stride,
                                 k_head_stride, lse_stride, p_batch_stride, p_head_stride, p_row_stride,
                                 softmax_scale, is_causal, dtype, 0.f, nullptr, stream);
}

int bp_attn_probs_dropout(const void *q, const void *k, const float *softmax_lse, void *probs,
                          int batch, int nheads, int head_dim, int seqlen_q, int seqlen_k,
                          int64_t q_batch_stride, int64_t q_row_stride, int64_t q_head_stride,
                          int64_t k_batch_stride, int64_t k_row_stride, int64_t k_head_stride,
                          int64_t lse_stride,
                          int64_t p_batch_stride, int64_t p_head_stride, int64_t p_row_stride,
                          float softmax_scale, int is_causal, int dtype,
                          float p_dropout, const uint64_t *rng_state, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (head_dim < 1 || head_dim > 128) return BP_ERR_HEAD_DIM;
    if (batch <= 0 || nheads <= 0 || seqlen_q <= 0 || seqlen_k <= 0) return BP_ERR_SHAPE;
    if (q == nullptr || k == nullptr || softmax_lse == nullptr || probs == nullptr) return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;

    bp::ProbsParams p{};
    p.q = q; p.k = k; p.lse = softmax_lse; p.p = probs;
    p.q_bs = q_batch_stride; p.q_rs = q_row_stride; p.q_hs = q_head_stride;
    p.k_bs = k_batch_stride; p.k_rs = k_row_stride; p.k_hs = k_head_stride;
    p.lse_stride = lse_stride;
    p.p_bs = p_batch_stride; p.p_hs = p_head_stride; p.p_rs = p_row_stride;
    p.b = batch; p.h = nheads; p.d = head_dim; p.sq = seqlen_q; p.sk = seqlen_k;
    p.causal = is_causal ? 1 : 0;
    p.p_vec = ((reinterpret_cast<uintptr_t>(probs) & 7u) == 0 && (p_batch_stride & 3) == 0 &&
               (p_head_stride & 3) == 0 && (p_row_stride & 3) == 0) ? 1 : 0;
    p.p_vec16 = (aligned16(probs) && strides8({p_batch_stride, p_head_stride, p_row_stride})) ? 1 : 0;
    p.scale_log2e = softmax_scale * bp::kLog2e;
    p.rng_state = rng_state;
    float unused_scale;
    if (!dropout_args(p_dropout, rng_state, p.drop_thr, unused_scale)) return BP_ERR_DROPOUT;
    const bool vec = head_dim % 8 == 0 && aligned16({q, k}) &&
                     strides8({q_batch_stride, q_row_stride, q_head_stride, k_batch_stride, k_row_stride, k_head_stride});
    return launch_status(bp::launch_attn_probs(p, dtype, vec, static_cast<hipStream_t>(stream)));
}

// LSE of every (sense, query): the flash kernel in LSE-only mode with the k senses as heads.
static int sense_lse(const void *qk, float *lse_ws, int batch, int seqlen, int nsenses, int d_k,
                     int64_t qk_bs, int64_t qk_rs, int64_t qk_two, int64_t qk_ss,
                     float softmax_scale, int dtype, hipStream_t stream) {
    const uint16_t *qp = static_cast<const uint16_t *>(qk);
    const uint16_t *kp = qp + qk_two;
    bp::FlashParams p{};
    p.q = qp; p.k = kp; p.v = nullptr; p.o = nullptr; p.lse = lse_ws;
    p.cu_q = nullptr; p.cu_k = nullptr;
    p.q_rs = qk_rs; p.q_hs = qk_ss; p.k_rs = qk_rs; p.k_hs = qk_ss;
    p.q_bs = qk_bs; p.k_bs = qk_bs;
    p.lse_stride = round_up(seqlen, 16);
    p.b = batch; p.h = nsenses; p.d = d_k;
    p.max_sq = seqlen; p.max_sk = seqlen;
    p.n_qtiles = (seqlen + 127) / 128;
    p.causal = 1;
    p.pair = p.n_qtiles > 1 ? 1 : 0;
    p.scale_log2e = softmax_scale * bp::kLog2e;
    const bool vec = qk_vec16(d_k, qp, qk_two, qk_bs, qk_rs, qk_ss);
    const bp::MixParams m = mix_params(qk, nullptr, nullptr, lse_ws, batch, seqlen, nsenses, d_k, 0, qk_bs, qk_rs, qk_two,
                                       qk_ss, 0, 0, 0, 0, 0, softmax_scale, nullptr);
    switch (sense_route(d_k, seqlen, 0, vec, true, false, false)) {
        case SenseKernel::WideRing:     // d_k = 160 / 640: sense_wide_dma.hip
            return launch_status(bp::launch_sense_lse_wide_dma(m, lse_ws, dtype, stream));
        case SenseKernel::WideStaged:   // wide senses (sense_wide.hip): the reference's vecs-4 / vecs-1 ablations
            return launch_status(bp::launch_sense_lse_wide(m, lse_ws, dtype, vec, stream));
        case SenseKernel::NarrowRing:
        case SenseKernel::NarrowStaged: break;
    }
    return launch_status(dispatch_flash(p, dtype, vec, stream));   // narrow: the flash kernel, the ring one exactly when vec
}

int bp_sense_lse(const void *qk, float *lse, int batch, int seqlen, int nsenses, int d_k,
                 int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride,
                 int64_t qk_sense_stride, float softmax_scale, int dtype, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (d_k < 1 || d_k > bp::kWideMaxDk) return BP_ERR_HEAD_DIM;
    if (batch <= 0 || nsenses <= 0 || seqlen <= 0) return BP_ERR_SHAPE;
    if (qk == nullptr || lse == nullptr) return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;
    return sense_lse(qk, lse, batch, seqlen, nsenses, d_k, qk_batch_stride, qk_row_stride,
                     qk_two_stride, qk_sense_stride, softmax_scale, dtype,
                     static_cast<hipStream_t>(stream));
}

int bp_sense_alpha(const void *qk, void *alpha, float *lse_ws, int lse_ready,
                   int batch, int seqlen, int nsenses, int d_k,
                   int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride,
                   int64_t qk_sense_stride, float softmax_scale, int dtype, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (d_k < 1 || d_k > bp::kWideMaxDk) return BP_ERR_HEAD_DIM;
    if (batch <= 0 || nsenses <= 0 || seqlen <= 0) return BP_ERR_SHAPE;
    if (qk == nullptr || alpha == nullptr || lse_ws == nullptr) return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!lse_ready) {
        int rc = sense_lse(qk, lse_ws, batch, seqlen, nsenses, d_k, qk_batch_stride, qk_row_stride,
                           qk_two_stride, qk_sense_stride, softmax_scale, dtype, st);
        if (rc != BP_OK) return rc;
    }
    const uint16_t *qp = static_cast<const uint16_t *>(qk);
    const int64_t S = seqlen;
    const bool vec = qk_vec16(d_k, qp, qk_two_stride, qk_batch_stride, qk_row_stride, qk_sense_stride);
    if (is_wide(sense_route(d_k, seqlen, 0, vec, true, false, false))) {   // one alpha kernel for wide senses: sense_wide.hip
        const bp::MixParams m = mix_params(qk, nullptr, nullptr, lse_ws, batch, seqlen, nsenses, d_k, 0, qk_batch_stride,
                                           qk_row_stride, qk_two_stride, qk_sense_stride, 0, 0, 0, 0, 0, softmax_scale,
                                           nullptr);
        return launch_status(bp::launch_sense_alpha_wide(m, alpha, dtype, vec, st));
    }
    return bp_attn_probs(qp, qp + qk_two_stride, lse_ws, alpha, batch, nsenses, d_k, seqlen, seqlen,
                         qk_batch_stride, qk_row_stride, qk_sense_stride,
                         qk_batch_stride, qk_row_stride, qk_sense_stride,
                         round_up(seqlen, 16),
                         (int64_t)nsenses * S * S, S * S, S,
                         softmax_scale, 1, dtype, stream);
}

int bp_sense_mix(const void *qk, const void *content, void *out, float *lse_ws, int lse_ready,
                 int batch, int seqlen, int nsenses, int d_k, int d_out,
                 int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride,
                 int64_t qk_sense_stride,
                 int64_t c_batch_stride, int64_t c_row_stride, int64_t c_sense_stride,
                 int64_t o_batch_stride, int64_t o_row_stride,
                 float softmax_scale, int dtype, void *queue_ws, bp_stream_t stream) {
    return bp_sense_mix_weighted(qk, content, nullptr, out, lse_ws, lse_ready, batch, seqlen, nsenses, d_k, d_out,
                                 qk_batch_stride, qk_row_stride, qk_two_stride, qk_sense_stride, c_batch_stride,
                                 c_row_stride, c_sense_stride, 0, 0, o_batch_stride, o_row_stride, softmax_scale,
                                 dtype, queue_ws, stream);
}

int bp_sense_mix_weighted(const void *qk, const void *content, const float *key_weight, void *out,
                          float *lse_ws, int lse_ready,
                          int batch, int seqlen, int nsenses, int d_k, int d_out,
                          int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride,
                          int64_t qk_sense_stride,
                          int64_t c_batch_stride, int64_t c_row_stride, int64_t c_sense_stride,
                          int64_t kw_batch_stride, int64_t kw_sense_stride,
                          int64_t o_batch_stride, int64_t o_row_stride,
                          float softmax_scale, int dtype, void *queue_ws, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (d_k < 1 || d_k > bp::kWideMaxDk) return BP_ERR_HEAD_DIM;
    if (queue_ws != nullptr && !aligned16(queue_ws)) return BP_ERR_SHAPE;
    if (d_out < 1) return BP_ERR_DOUT;
    if (batch <= 0 || nsenses <= 0 || seqlen <= 0) return BP_ERR_SHAPE;
    if (qk == nullptr || content == nullptr || out == nullptr || lse_ws == nullptr) return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (null_queue_ws_on_capturing_stream(queue_ws, st)) return BP_ERR_QUEUE_WS;
    if (!lse_ready) {
        int rc = sense_lse(qk, lse_ws, batch, seqlen, nsenses, d_k, qk_batch_stride, qk_row_stride,
                           qk_two_stride, qk_sense_stride, softmax_scale, dtype, st);
        if (rc != BP_OK) return rc;
    }

    bp::MixParams p = mix_params(qk, content, out, lse_ws, batch, seqlen, nsenses, d_k, d_out, qk_batch_stride,
                                 qk_row_stride, qk_two_stride, qk_sense_stride, c_batch_stride, c_row_stride,
                                 c_sense_stride, o_batch_stride, o_row_stride, softmax_scale, queue_ws);
    p.kw = key_weight; p.kw_bs = kw_batch_stride; p.kw_ss = kw_sense_stride;
    const bool vec_qk = qk_vec16(d_k, static_cast<const uint16_t *>(qk), qk_two_stride, qk_batch_stride, qk_row_stride,
                                 qk_sense_stride);
    const bool vec_c = d_out % 8 == 0 && aligned16({content, out}) &&
                       strides8({c_batch_stride, c_row_stride, c_sense_stride, o_batch_stride, o_row_stride});
    switch (sense_route(d_k, seqlen, d_out, vec_qk, vec_c, key_weight != nullptr, false)) {
        case SenseKernel::WideRing:   return launch_status(bp::launch_sense_mix_wide_dma(p, dtype, st));   // d_k = 160 / 640
        case SenseKernel::WideStaged: return launch_status(bp::launch_sense_mix_wide(p, dtype, vec_qk, vec_c, st));
        case SenseKernel::NarrowRing: return launch_status(bp::launch_sense_mix_dma(p, dtype, st));
        case SenseKernel::NarrowStaged: break;
    }
    return launch_status(bp::launch_sense_mix(p, dtype, vec_qk, vec_c, st));
}

int bp_sense_mix_gather(const void *qk, const void *table, const int32_t *row_index, void *out,
                        float *lse_ws, int lse_ready,
                        int batch, int seqlen, int nsenses, int d_k, int d_out, int64_t table_rows,
                        int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride,
                        int64_t qk_sense_stride,
                        int64_t t_row_stride, int64_t t_sense_stride, int64_t idx_batch_stride,
                        int64_t o_batch_stride, int64_t o_row_stride,
                        float softmax_scale, int dtype, void *queue_ws, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    // the ring kernels only: wide senses at the reference's two few-sense widths (sense_wide_dma.hip, row indices as u32 in
    // LDS: no limit on the row count); every other shape is gathered by the caller.  16-byte friendliness is checked below.
    const SenseKernel route = sense_route(d_k, seqlen, d_out, d_k % 8 == 0, true, false, true);
    const bool wide = route == SenseKernel::WideRing;
    if (d_k < 8 || (route != SenseKernel::NarrowRing && !wide)) return BP_ERR_HEAD_DIM;
    if (queue_ws != nullptr && !aligned16(queue_ws)) return BP_ERR_SHAPE;
    if (d_out < 8 || d_out % 8 != 0) return BP_ERR_DOUT;
    if (batch <= 0 || nsenses <= 0 || seqlen <= 0 || seqlen > bp::kMixGatherMaxKeys || table_rows <= 0 ||
        (!wide && table_rows > bp::kMixGatherMaxRows)) return BP_ERR_SHAPE;
    if (qk == nullptr || table == nullptr || row_index == nullptr || out == nullptr || lse_ws == nullptr) return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;
    if (!qk_vec16(d_k, static_cast<const uint16_t *>(qk), qk_two_stride, qk_batch_stride, qk_row_stride, qk_sense_stride) ||
        !aligned16({table, out}) || !strides8({t_row_stride, t_sense_stride, o_batch_stride, o_row_stride}))
        return BP_ERR_SHAPE;
    if (t_row_stride <= 0 || table_rows * t_row_stride * 2 >= (int64_t(1) << 32)) return BP_ERR_SHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (null_queue_ws_on_capturing_stream(queue_ws, st)) return BP_ERR_QUEUE_WS;
    if (!lse_ready) {
        int rc = sense_lse(qk, lse_ws, batch, seqlen, nsenses, d_k, qk_batch_stride, qk_row_stride,
                           qk_two_stride, qk_sense_stride, softmax_scale, dtype, st);
        if (rc != BP_OK) return rc;
    }
    bp::MixParams p = mix_params(qk, table, out, lse_ws, batch, seqlen, nsenses, d_k, d_out, qk_batch_stride,
                                 qk_row_stride, qk_two_stride, qk_sense_stride, 0, t_row_stride, t_sense_stride,
                                 o_batch_stride, o_row_stride, softmax_scale, queue_ws);
    p.row_index = row_index; p.idx_bs = idx_batch_stride; p.last_table_row = (uint32_t)(table_rows - 1);
    return launch_status(wide ? bp::launch_sense_mix_wide_dma(p, dtype, st) : bp::launch_sense_mix_dma(p, dtype, st));
}

// ---- packed batches: sample b owns rows [cu_seqlens[b], cu_seqlens[b + 1]) of (total, ...) operands -----------------------
// Narrow senses on the 16-byte path only (the ring kernels); cu_seqlens is never read on the host.
namespace {

// what the three packed entry points share: dtype, sense width, the qk layout.  BP_OK or the refusal.
int varlen_qk_args(const void *qk, const int32_t *cu_seqlens, int batch, int max_seqlen, int nsenses, int d_k,
                   int64_t qk_rs, int64_t qk_two, int64_t qk_ss, float softmax_scale, int dtype) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (d_k < 8 || d_k > 128 || d_k % 8 != 0) return BP_ERR_HEAD_DIM;
    if (batch <= 0 || nsenses <= 0 || max_seqlen <= 0) return BP_ERR_SHAPE;
    if (qk == nullptr || cu_seqlens == nullptr) return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;
    if (!qk_vec16(d_k, static_cast<const uint16_t *>(qk), qk_two, 0, qk_rs, qk_ss)) return BP_ERR_SHAPE;
    return BP_OK;
}

// the flash ring kernel in LSE-only mode with the senses as heads, sequences from cu_seqlens (as the trunk's ragged calls)
int sense_lse_varlen(const void *qk, float *lse_ws, const int32_t *cu_seqlens, int batch, int max_seqlen, int nsenses,
                     int d_k, int64_t qk_rs, int64_t qk_two, int64_t qk_ss, float softmax_scale, int dtype,
                     hipStream_t stream) {
    const uint16_t *qp = static_cast<const uint16_t *>(qk);
    bp::FlashParams p{};
    p.q = qp; p.k = qp + qk_two; p.v = nullptr; p.o = nullptr; p.lse = lse_ws;
    p.cu_q = cu_seqlens; p.cu_k = cu_seqlens;
    p.q_rs = qk_rs; p.q_hs = qk_ss; p.k_rs = qk_rs; p.k_hs = qk_ss;
    p.lse_stride = round_up(max_seqlen, 16);
    p.b = batch; p.h = nsenses; p.d = d_k;
    p.max_sq = max_seqlen; p.max_sk = max_seqlen;
    p.n_qtiles = (max_seqlen + 127) / 128;
    p.causal = 1;
    p.pair = p.n_qtiles > 1 ? 1 : 0;
    p.scale_log2e = softmax_scale * bp::kLog2e;
    return launch_status(bp::launch_flash_fwd_dma(p, dtype, stream));
}

int sense_mix_varlen(const void *qk, const void *content, bool gather, const int32_t *row_index, void *out, float *lse_ws,
                     int lse_ready, const int32_t *cu_seqlens, int batch, int max_seqlen, int nsenses, int d_k, int d_out,
                     int64_t table_rows, int64_t qk_rs, int64_t qk_two, int64_t qk_ss, int64_t c_rs, int64_t c_ss,
                     int64_t o_rs, float softmax_scale, int dtype, void *queue_ws, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (d_k < 8 || d_k > 128 || d_k % 8 != 0) return BP_ERR_HEAD_DIM;
    if (queue_ws != nullptr && !aligned16(queue_ws)) return BP_ERR_SHAPE;
    if (d_out < 8 || d_out % 8 != 0) return BP_ERR_DOUT;
    if (max_seqlen > bp::kMixMaxTiles * 256) return BP_ERR_SHAPE;
    if (gather && (max_seqlen > bp::kMixGatherMaxKeys || table_rows <= 0 || table_rows > bp::kMixGatherMaxRows ||
                   row_index == nullptr))
        return BP_ERR_SHAPE;
    if (content == nullptr || out == nullptr || lse_ws == nullptr) return BP_ERR_SHAPE;
    const int rc = varlen_qk_args(qk, cu_seqlens, batch, max_seqlen, nsenses, d_k, qk_rs, qk_two, qk_ss, softmax_scale, dtype);
    if (rc != BP_OK) return rc;
    if (!aligned16({content, out}) || !strides8({c_rs, c_ss, o_rs})) return BP_ERR_SHAPE;
    if (gather && (c_rs <= 0 || table_rows * c_rs * 2 >= (int64_t(1) << 32))) return BP_ERR_SHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (null_queue_ws_on_capturing_stream(queue_ws, st)) return BP_ERR_QUEUE_WS;
    if (!lse_ready) {
        const int lse_rc = sense_lse_varlen(qk, lse_ws, cu_seqlens, batch, max_seqlen, nsenses, d_k, qk_rs, qk_two, qk_ss,
                                            softmax_scale, dtype, st);
        if (lse_rc != BP_OK) return lse_rc;
    }
    bp::MixParams p = mix_params(qk, content, out, lse_ws, batch, max_seqlen, nsenses, d_k, d_out, 0, qk_rs, qk_two, qk_ss,
                                 0, c_rs, c_ss, 0, o_rs, softmax_scale, queue_ws);
    p.cu = cu_seqlens;
    if (gather) { p.row_index = row_index; p.last_table_row = (uint32_t)(table_rows - 1); }
    return launch_status(bp::launch_sense_mix_varlen(p, dtype, st));
}

}  // namespace

int bp_sense_lse_varlen(const void *qk, float *lse, const int32_t *cu_seqlens, int batch, int max_seqlen, int nsenses,
                        int d_k, int64_t qk_row_stride, int64_t qk_two_stride, int64_t qk_sense_stride,
                        float softmax_scale, int dtype, bp_stream_t stream) {
    const int rc = varlen_qk_args(qk, cu_seqlens, batch, max_seqlen, nsenses, d_k, qk_row_stride, qk_two_stride,
                                  qk_sense_stride, softmax_scale, dtype);
    if (rc != BP_OK) return rc;
    if (lse == nullptr) return BP_ERR_SHAPE;
    return sense_lse_varlen(qk, lse, cu_seqlens, batch, max_seqlen, nsenses, d_k, qk_row_stride, qk_two_stride,
                            qk_sense_stride, softmax_scale, dtype, static_cast<hipStream_t>(stream));
}

int bp_sense_mix_varlen(const void *qk, const void *content, void *out, float *lse_ws, int lse_ready,
                        const int32_t *cu_seqlens, int batch, int max_seqlen, int nsenses, int d_k, int d_out,
                        int64_t qk_row_stride, int64_t qk_two_stride, int64_t qk_sense_stride,
                        int64_t c_row_stride, int64_t c_sense_stride, int64_t o_row_stride,
                        float softmax_scale, int dtype, void *queue_ws, bp_stream_t stream) {
    return sense_mix_varlen(qk, content, false, nullptr, out, lse_ws, lse_ready, cu_seqlens, batch, max_seqlen, nsenses, d_k,
                            d_out, 0, qk_row_stride, qk_two_stride, qk_sense_stride, c_row_stride, c_sense_stride,
                            o_row_stride, softmax_scale, dtype, queue_ws, stream);
}

int bp_sense_mix_gather_varlen(const void *qk, const void *table, const int32_t *row_index, void *out,
                               float *lse_ws, int lse_ready,
                               const int32_t *cu_seqlens, int batch, int max_seqlen, int nsenses, int d_k, int d_out,
                               int64_t table_rows,
                               int64_t qk_row_stride, int64_t qk_two_stride, int64_t qk_sense_stride,
                               int64_t t_row_stride, int64_t t_sense_stride, int64_t o_row_stride,
                               float softmax_scale, int dtype, void *queue_ws, bp_stream_t stream) {
    return sense_mix_varlen(qk, table, true, row_index, out, lse_ws, lse_ready, cu_seqlens, batch, max_seqlen, nsenses, d_k,
                            d_out, table_rows, qk_row_stride, qk_two_stride, qk_sense_stride, t_row_stride, t_sense_stride,
                            o_row_stride, softmax_scale, dtype, queue_ws, stream);
}

int bp_sense_mix_dc(const void *qk, const void *dout, const float *lse, void *dcontent,
                    int batch, int seqlen, int nsenses, int d_k, int d_out,
                    int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride, int64_t qk_sense_stride,
                    int64_t do_batch_stride, int64_t do_row_stride,
                    int64_t c_batch_stride, int64_t c_row_stride, int64_t c_sense_stride,
                    float softmax_scale, int dtype, void *queue_ws, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (d_k < 8 || d_k > 128 || d_k % 8 != 0) return BP_ERR_HEAD_DIM;
    if (queue_ws != nullptr && !aligned16(queue_ws)) return BP_ERR_SHAPE;
    if (d_out < 8 || d_out % 8 != 0) return BP_ERR_DOUT;
    if (batch <= 0 || nsenses <= 0 || seqlen <= 0 || seqlen > 65536) return BP_ERR_SHAPE;
    if (qk == nullptr || dout == nullptr || lse == nullptr || dcontent == nullptr) return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;
    const uint16_t *qp = static_cast<const uint16_t *>(qk);
    if (!qk_vec16(d_k, qp, qk_two_stride, qk_batch_stride, qk_row_stride, qk_sense_stride) || !aligned16({dout, dcontent}) ||
        !strides8({do_batch_stride, do_row_stride, c_batch_stride, c_row_stride, c_sense_stride}))
        return BP_ERR_SHAPE;
    if (null_queue_ws_on_capturing_stream(queue_ws, static_cast<hipStream_t>(stream))) return BP_ERR_QUEUE_WS;
    bp::MixBwdParams p{};
    p.q = qp; p.k = qp + qk_two_stride; p.dout = dout; p.dc = dcontent; p.lse = lse;
    p.qk_bs = qk_batch_stride; p.qk_rs = qk_row_stride; p.qk_ss = qk_sense_stride;
    p.do_bs = do_batch_stride; p.do_rs = do_row_stride;
    p.c_bs = c_batch_stride; p.c_rs = c_row_stride; p.c_ss = c_sense_stride;
    p.lse_stride = round_up(seqlen, 16);
    p.b = batch; p.s = seqlen; p.nsenses = nsenses; p.dk = d_k; p.dout_cols = d_out;
    p.n_ktiles = (seqlen + 255) / 256;
    p.n_chunks = (d_out + 255) / 256;
    p.scale_log2e = softmax_scale * bp::kLog2e;
    p.queues = static_cast<bp::MixQueues *>(queue_ws);
    return launch_status(bp::launch_sense_mix_dc(p, dtype, static_cast<hipStream_t>(stream)));
}

int bp_sense_dq_dk(const void *qk, const void *dpt, const float *lse, float *dsum_ws, void *dqk, float *dk_acc,
                   int batch, int seqlen, int nsenses, int d_k, int t0,
                   int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride, int64_t qk_sense_stride,
                   int64_t dpt_batch_stride,
                   int64_t dqk_batch_stride, int64_t dqk_row_stride, int64_t dqk_sense_stride,
                   int64_t dka_batch_stride, int64_t dka_row_stride, int64_t dka_sense_stride,
                   float softmax_scale, int dtype, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (d_k < 8 || d_k > 128 || d_k % 8 != 0) return BP_ERR_HEAD_DIM;
    if (batch <= 0 || nsenses <= 0 || seqlen <= 0 || t0 < 0 || t0 >= seqlen || t0 % 128 != 0) return BP_ERR_SHAPE;
    if (!qk || !dpt || !lse || !dsum_ws || !dqk || !dk_acc) return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;
    const uint16_t *qp = static_cast<const uint16_t *>(qk);
    if (!qk_vec16(d_k, qp, qk_two_stride, qk_batch_stride, qk_row_stride, qk_sense_stride) ||
        !aligned16({dpt, dqk, dk_acc}) || !strides8({dpt_batch_stride, dqk_batch_stride, dqk_row_stride, dqk_sense_stride}))
        return BP_ERR_SHAPE;
    if ((dka_batch_stride | dka_row_stride | dka_sense_stride) & 3) return BP_ERR_SHAPE;
    bp::SenseGradParams p{};
    p.q = qp; p.k = qp + qk_two_stride; p.dpt = dpt; p.lse = lse; p.dsum = dsum_ws; p.dq = dqk; p.dk_acc = dk_acc;
    p.qk_bs = qk_batch_stride; p.qk_rs = qk_row_stride; p.qk_ss = qk_sense_stride;
    p.dpt_bs = dpt_batch_stride;
    p.dq_bs = dqk_batch_stride; p.dq_rs = dqk_row_stride; p.dq_ss = dqk_sense_stride;
    p.dka_bs = dka_batch_stride; p.dka_rs = dka_row_stride; p.dka_ss = dka_sense_stride;
    p.lse_stride = round_up(seqlen, 16);
    p.b = batch; p.s = seqlen; p.nsenses = nsenses; p.dk = d_k; p.t0 = t0;
    p.scale = softmax_scale;
    return launch_status(bp::launch_sense_dq_dk(p, dtype, static_cast<hipStream_t>(stream)));
}

int64_t bp_flash_bwd_ws_floats(int batch, int nheads, int64_t lse_stride) {
    if (batch <= 0 || nheads <= 0 || lse_stride <= 0) return 0;
    return (int64_t)batch * nheads * 2 * lse_stride;
}

int bp_flash_bwd(const void *dout, const void *q, const void *k, const void *v, const void *out,
                 const float *softmax_lse, float *dsum_ws, int64_t dsum_ws_floats, void *dq, void *dk, void *dv,
                 const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k,
                 int batch, int nheads, int head_dim, int max_seqlen_q, int max_seqlen_k,
                 int64_t do_row_stride, int64_t do_head_stride,
                 int64_t q_row_stride, int64_t q_head_stride,
                 int64_t k_row_stride, int64_t k_head_stride,
                 int64_t v_row_stride, int64_t v_head_stride,
                 int64_t o_row_stride, int64_t o_head_stride,
                 int64_t dq_row_stride, int64_t dq_head_stride,
                 int64_t dk_row_stride, int64_t dk_head_stride,
                 int64_t dv_row_stride, int64_t dv_head_stride,
                 int64_t lse_stride, float softmax_scale, int is_causal, int dtype,
                 bp_stream_t stream) {
    return bp_flash_bwd_dropout(dout, q, k, v, out, softmax_lse, dsum_ws, dsum_ws_floats, dq, dk, dv, cu_seqlens_q, cu_seqlens_k, batch,
                                nheads, head_dim, max_seqlen_q, max_seqlen_k, do_row_stride, do_head_stride,
                                q_row_stride, q_head_stride, k_row_stride, k_head_stride, v_row_stride,
                                v_head_stride, o_row_stride, o_head_stride, dq_row_stride, dq_head_stride,
                                dk_row_stride, dk_head_stride, dv_row_stride, dv_head_stride, lse_stride,
                                softmax_scale, is_causal, dtype, 0.f, nullptr, stream);
}

int bp_flash_bwd_dropout(const void *dout, const void *q, const void *k, const void *v, const void *out,
                 const float *softmax_lse, float *dsum_ws, int64_t dsum_ws_floats, void *dq, void *dk, void *dv,
                 const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k,
                 int batch, int nheads, int head_dim, int max_seqlen_q, int max_seqlen_k,
                 int64_t do_row_stride, int64_t do_head_stride,
                 int64_t q_row_stride, int64_t q_head_stride,
                 int64_t k_row_stride, int64_t k_head_stride,
                 int64_t v_row_stride, int64_t v_head_stride,
                 int64_t o_row_stride, int64_t o_head_stride,
                 int64_t dq_row_stride, int64_t dq_head_stride,
                 int64_t dk_row_stride, int64_t dk_head_stride,
                 int64_t dv_row_stride, int64_t dv_head_stride,
                 int64_t lse_stride, float softmax_scale, int is_causal, int dtype,
                 float p_dropout, const uint64_t *rng_state, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (head_dim < 8 || head_dim > 128 || head_dim % 8 != 0) return BP_ERR_HEAD_DIM;
    if (batch <= 0 || nheads <= 0 || max_seqlen_q <= 0 || max_seqlen_k <= 0) return BP_ERR_SHAPE;
    if (!dout || !q || !k || !v || !out || !softmax_lse || !dsum_ws || !dq || !dk || !dv) return BP_ERR_SHAPE;
    if ((cu_seqlens_q == nullptr) != (cu_seqlens_k == nullptr)) return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;
    if (!aligned16({dout, q, k, v, out, dq, dk, dv, softmax_lse, dsum_ws}) ||
        !strides8({do_row_stride, do_head_stride, q_row_stride, q_head_stride, k_row_stride, k_head_stride, v_row_stride,
                   v_head_stride, o_row_stride, o_head_stride, dq_row_stride, dq_head_stride, dk_row_stride,
                   dk_head_stride, dv_row_stride, dv_head_stride}))
        return BP_ERR_SHAPE;
    if (lse_stride % 16 != 0) return BP_ERR_SHAPE;
    // the dQ kernel writes both statistics rows of every (batch, head): an ABI-2-sized buffer would be overrun
    if (dsum_ws_floats < bp_flash_bwd_ws_floats(batch, nheads, lse_stride)) return BP_ERR_WORKSPACE;

    bp::FlashBwdParams p{};
    p.q = q; p.k = k; p.v = v; p.dout = dout; p.out = out; p.lse = softmax_lse; p.dsum = dsum_ws;
    p.dq = dq; p.dk = dk; p.dv = dv; p.cu_q = cu_seqlens_q; p.cu_k = cu_seqlens_k;
    p.q_rs = q_row_stride; p.q_hs = q_head_stride; p.k_rs = k_row_stride; p.k_hs = k_head_stride;
    p.v_rs = v_row_stride; p.v_hs = v_head_stride; p.do_rs = do_row_stride; p.do_hs = do_head_stride;
    p.o_rs = o_row_stride; p.o_hs = o_head_stride;
    p.dq_rs = dq_row_stride; p.dq_hs = dq_head_stride; p.dk_rs = dk_row_stride; p.dk_hs = dk_head_stride;
    p.dv_rs = dv_row_stride; p.dv_hs = dv_head_stride;
    p.lse_stride = lse_stride;
    p.b = batch; p.h = nheads; p.d = head_dim; p.max_sq = max_seqlen_q; p.max_sk = max_seqlen_k;
    p.causal = is_causal ? 1 : 0;
    p.scale = softmax_scale;
    p.rng_state = rng_state;
    if (!dropout_args(p_dropout, rng_state, p.drop_thr, p.drop_scale)) return BP_ERR_DROPOUT;
    hipError_t e = bp::launch_flash_bwd(p, dtype, static_cast<hipStream_t>(stream));
    if (e == hipErrorNotSupported) return BP_ERR_HEAD_DIM;
    return launch_status(e);
}

int bp_add_layer_norm(const void *x0, const void *x1, const void *gamma, const void *beta, void *z,
                      void *x_out, int64_t rows, int cols, float epsilon, int dtype, int x1_is_f32,
                      int xout_is_f32, int w_is_f32, bp_stream_t stream) {
    return bp_dropout_add_layer_norm(x0, x1, gamma, beta, z, x_out, nullptr, rows, cols, epsilon, dtype, 0,
                                     x1_is_f32, xout_is_f32, w_is_f32, 0.f, nullptr, stream);
}

int bp_dropout_add_layer_norm(const void *x0, const void *x1, const void *gamma, const void *beta, void *z,
                              void *x_out, uint8_t *dmask, int64_t rows, int cols, float epsilon, int dtype,
                              int x0_is_f32, int x1_is_f32, int xout_is_f32, int w_is_f32,
                              float p_dropout, const uint64_t *rng_state, bp_stream_t stream) {
    return bp_dropout_add_layer_norm_scaled(x0, x1, gamma, beta, nullptr, nullptr, z, x_out, dmask, rows, cols, epsilon,
                                            dtype, x0_is_f32, x1_is_f32, xout_is_f32, w_is_f32, p_dropout, rng_state, stream);
}

int bp_dropout_add_layer_norm_scaled(const void *x0, const void *x1, const void *gamma, const void *beta,
                                     const void *rowscale, const void *colscale, void *z, void *x_out, uint8_t *dmask,
                                     int64_t rows, int cols, float epsilon, int dtype, int x0_is_f32, int x1_is_f32,
                                     int xout_is_f32, int w_is_f32, float p_dropout, const uint64_t *rng_state,
                                     bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (rows <= 0 || rows > 0xffffffffLL || cols <= 0 || cols % 4 != 0 || cols > 8192) return BP_ERR_SHAPE;
    if (x0 == nullptr || gamma == nullptr || beta == nullptr || z == nullptr) return BP_ERR_SHAPE;
    if (!aligned16({x0, gamma, beta, z}) || !aligned16_or_null({x1, x_out, colscale}) ||
        (rowscale != nullptr && (reinterpret_cast<uintptr_t>(rowscale) & (x0_is_f32 ? 3u : 1u)) != 0) ||
        (dmask != nullptr && (reinterpret_cast<uintptr_t>(dmask) & 3u) != 0))
        return BP_ERR_SHAPE;
    if (!(isfinite(epsilon) && epsilon >= 0.f)) return BP_ERR_SCALE;
    // one residual dtype: when both x1 and x_out exist they must agree (reference ln_api.cpp:99-102);
    // an fp32 x0 implies an fp32 residual stream
    if (x1 != nullptr && x_out != nullptr && (x1_is_f32 != 0) != (xout_is_f32 != 0)) return BP_ERR_DTYPE;
    if (x0_is_f32 && ((x1 != nullptr && !x1_is_f32) || (x_out != nullptr && !xout_is_f32))) return BP_ERR_DTYPE;
    bp::LnParams p{};
    p.x0 = x0; p.x1 = x1; p.gamma = gamma; p.beta = beta; p.z = z; p.x_out = x_out;
    p.rows = rows; p.cols = cols; p.eps = epsilon;
    p.x1_f32 = x1_is_f32 ? 1 : 0; p.xo_f32 = xout_is_f32 ? 1 : 0; p.w_f32 = w_is_f32 ? 1 : 0;
    p.x0_f32 = x0_is_f32 ? 1 : 0;
    p.dmask = dmask; p.rng_state = rng_state;
    p.rowscale = rowscale; p.colscale = colscale;
    if (!dropout_args(p_dropout, rng_state, p.drop_thr, p.drop_scale)) return BP_ERR_DROPOUT;
    return launch_status(bp::launch_add_layer_norm(p, dtype, static_cast<hipStream_t>(stream)));
}

int bp_add_layer_norm_chain(const void *x0a, const void *x0b, const void *x1, const int64_t *token_ids,
                            const int64_t *position_ids, const void *word_table, const void *position_table,
                            const void *gamma, const void *beta, void *z, void *x_out, int64_t rows, int cols,
                            int64_t table_rows, int64_t position_rows, int64_t position_len, float epsilon, int dtype,
                            int w_is_f32, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (rows <= 0 || rows > 0xffffffffLL || cols <= 0 || cols % 4 != 0 || cols > 2048) return BP_ERR_SHAPE;
    if (gamma == nullptr || beta == nullptr || z == nullptr) return BP_ERR_SHAPE;
    // exactly one source of x0a: the tensor, or the tables with their ids
    const bool emb = word_table != nullptr;
    if (emb == (x0a != nullptr)) return BP_ERR_SHAPE;
    if (emb) {
        if (token_ids == nullptr || table_rows <= 0 || x1 != nullptr) return BP_ERR_SHAPE;   // (the embedding IS the stream so far)
        if ((reinterpret_cast<uintptr_t>(token_ids) & 7u) != 0 || (reinterpret_cast<uintptr_t>(position_ids) & 7u) != 0)
            return BP_ERR_SHAPE;
        if (position_table != nullptr) {
            if (position_rows <= 0 || position_len <= 0 || position_len > rows || rows % position_len != 0) return BP_ERR_SHAPE;
        } else if (position_ids != nullptr) {
            return BP_ERR_SHAPE;
        }
    } else if (token_ids != nullptr || position_ids != nullptr || position_table != nullptr) {
        return BP_ERR_SHAPE;
    }
    // 8-byte chunks of the 16-bit operands, 16-byte chunks of the fp32 residual stream and of fp32 weights
    if (!aligned16({gamma, beta, z}) || !aligned16_or_null({x0a, x0b, x1, x_out, word_table, position_table})) return BP_ERR_SHAPE;
    if (!(isfinite(epsilon) && epsilon >= 0.f)) return BP_ERR_SCALE;
    bp::LnParams p{};
    p.x0 = x0a; p.x0b = x0b; p.x1 = x1; p.gamma = gamma; p.beta = beta; p.z = z; p.x_out = x_out;
    p.rows = rows; p.cols = cols; p.eps = epsilon;
    p.x1_f32 = 1; p.xo_f32 = 1; p.w_f32 = w_is_f32 ? 1 : 0; p.x0_f32 = 0;
    if (emb) {
        p.tok = token_ids; p.wte = word_table; p.last_tok = table_rows - 1;
        if (position_table != nullptr) {
            p.pos = position_ids; p.wpe = position_table; p.last_pos = position_rows - 1;
            p.pos_len = (uint32_t)position_len;
        }
    }
    return launch_status(bp::launch_add_layer_norm_chain(p, dtype, static_cast<hipStream_t>(stream)));
}

int bp_softmax_bwd_causal(const void *alpha, void *dalpha_inout, int64_t n_matrices, int seqlen,
                          float softmax_scale, int dtype, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (n_matrices <= 0 || seqlen <= 0 || seqlen % 8 != 0 || seqlen > 4096) return BP_ERR_SHAPE;
    if (alpha == nullptr || dalpha_inout == nullptr || !aligned16({alpha, dalpha_inout})) return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;
    bp::SoftmaxBwdParams p{};
    p.alpha = alpha; p.dp = dalpha_inout; p.rows = n_matrices * seqlen; p.s = seqlen; p.scale = softmax_scale;
    hipError_t e = bp::launch_softmax_bwd_causal(p, dtype, static_cast<hipStream_t>(stream));
    if (e == hipErrorNotSupported) return BP_ERR_SHAPE;
    return launch_status(e);
}

int bp_add_layer_norm_bwd(const void *dz, const void *dx_in, const void *x, const void *gamma,
                          void *dx0, void *dx1, void *dgamma, void *dbeta, float *ws,
                          int64_t rows, int cols, float epsilon, int dtype, int res_is_f32, int w_is_f32,
                          bp_stream_t stream) {
    return bp_dropout_add_layer_norm_bwd(dz, dx_in, x, gamma, dx0, dx1, dgamma, dbeta, ws, rows, cols, epsilon, dtype,
                                         0, res_is_f32, w_is_f32, 0.f, nullptr, stream);
}

int bp_dropout_add_layer_norm_bwd(const void *dz, const void *dx_in, const void *x, const void *gamma,
                                  void *dx0, void *dx1, void *dgamma, void *dbeta, float *ws,
                                  int64_t rows, int cols, float epsilon, int dtype, int x0_is_f32, int res_is_f32,
                                  int w_is_f32, float p_dropout, const uint64_t *rng_state, bp_stream_t stream) {
    // (the unscaled entry point keeps its documented workspace contract: 2 * BP_LN_BWD_WS_ROWS * cols floats)
    return bp_dropout_add_layer_norm_scaled_bwd(dz, dx_in, x, nullptr, gamma, nullptr, nullptr, dx0, dx1, dgamma, dbeta,
                                                nullptr, ws, bp_ln_bwd_ws_floats(cols, 0), rows, cols, epsilon, dtype,
                                                x0_is_f32, res_is_f32, w_is_f32, p_dropout, rng_state, stream);
}

int64_t bp_ln_bwd_ws_floats(int cols, int has_colscale) {
    if (cols <= 0) return 0;
    return (int64_t)(has_colscale ? 3 : 2) * bp::kLnBwdMaxWg * cols;
}

int bp_dropout_add_layer_norm_scaled_bwd(const void *dz, const void *dx_in, const void *x, const void *x0,
                                         const void *gamma, const void *rowscale, const void *colscale,
                                         void *dx0, void *dx1, void *dgamma, void *dbeta, void *dcolscale,
                                         float *ws, int64_t ws_floats, int64_t rows, int cols, float epsilon, int dtype,
                                         int x0_is_f32, int res_is_f32, int w_is_f32, float p_dropout,
                                         const uint64_t *rng_state, bp_stream_t stream) {
    static_assert(BP_LN_BWD_WS_ROWS == bp::kLnBwdMaxWg, "workspace rows");
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (rows <= 0 || rows > 0xffffffffLL || cols <= 0 || cols % 4 != 0 || cols > 2048) return BP_ERR_SHAPE;
    if (!dz || !x || !gamma || !dx0 || !dgamma || !dbeta || !ws) return BP_ERR_SHAPE;
    if (colscale != nullptr && (x0 == nullptr || dcolscale == nullptr)) return BP_ERR_SHAPE;   // (layer_norm.py:36-37)
    if (!aligned16_or_null({dz, dx_in, x, x0, gamma, colscale, dx0, dx1, dgamma, dbeta, dcolscale, ws})) return BP_ERR_SHAPE;
    if (rowscale != nullptr && (reinterpret_cast<uintptr_t>(rowscale) & (x0_is_f32 ? 3u : 1u)) != 0) return BP_ERR_SHAPE;
    if (!(isfinite(epsilon) && epsilon >= 0.f)) return BP_ERR_SCALE;
    if (x0_is_f32 && !res_is_f32) return BP_ERR_DTYPE;
    if (ws_floats < bp_ln_bwd_ws_floats(cols, colscale != nullptr)) return BP_ERR_WORKSPACE;
    bp::LnBwdParams p{};
    p.dz = dz; p.dx_in = dx_in; p.x = x; p.gamma = gamma; p.dx0 = dx0; p.dx1 = dx1;
    p.dgamma = dgamma; p.dbeta = dbeta; p.ws = ws;
    p.rows = rows; p.cols = cols; p.eps = epsilon;
    p.n_wg = (int)((rows + 3) / 4 < bp::kLnBwdMaxWg ? (rows + 3) / 4 : bp::kLnBwdMaxWg);
    p.res_f32 = res_is_f32 ? 1 : 0; p.w_f32 = w_is_f32 ? 1 : 0; p.x0_f32 = x0_is_f32 ? 1 : 0;
    p.rng_state = rng_state;
    p.rowscale = rowscale; p.colscale = colscale; p.x0 = x0; p.dcolscale = colscale != nullptr ? dcolscale : nullptr;
    if (!dropout_args(p_dropout, rng_state, p.drop_thr, p.drop_scale)) return BP_ERR_DROPOUT;
    hipError_t e = bp::launch_add_layer_norm_bwd(p, dtype, static_cast<hipStream_t>(stream));
    if (e == hipErrorNotSupported) return BP_ERR_SHAPE;
    return launch_status(e);
}

int64_t bp_bias_grad_ws_floats(int64_t rows, int cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return (int64_t)bp::bias_gelu_bwd_slices(rows, cols) * cols;
}

int bp_bias_gelu_fwd(const void *x, const void *bias, void *pre_out, void *y, int64_t rows, int cols, int dtype,
                     bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (rows <= 0 || cols <= 0 || cols % 8 != 0) return BP_ERR_SHAPE;
    if (x == nullptr || y == nullptr || !aligned16({x, y})) return BP_ERR_SHAPE;
    if (!aligned16_or_null({bias, pre_out})) return BP_ERR_SHAPE;
    if (pre_out != nullptr && bias == nullptr) return BP_ERR_SHAPE;   // without a bias the pre-activation IS x
    bp::BiasGeluParams p{};
    p.x = x; p.bias = bias; p.pre = pre_out; p.y = y; p.rows = rows; p.cols = cols;
    return launch_status(bp::launch_bias_gelu_fwd(p, dtype, static_cast<hipStream_t>(stream)));
}

static int bias_grad_common(const void *grad, void *dbias, float *ws, int64_t rows, int cols, int dtype) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (rows <= 0 || cols <= 0 || cols % 8 != 0) return BP_ERR_SHAPE;
    if (grad == nullptr || !aligned16(grad)) return BP_ERR_SHAPE;
    if (dbias != nullptr && (ws == nullptr || !aligned16(ws))) return BP_ERR_SHAPE;
    return BP_OK;
}

int bp_bias_gelu_bwd(const void *grad, const void *pre, void *dpre, void *dbias, float *ws, int64_t rows, int cols,
                     int dtype, int dbias_is_f32, bp_stream_t stream) {
    const int rc = bias_grad_common(grad, dbias, ws, rows, cols, dtype);
    if (rc != BP_OK) return rc;
    if (pre == nullptr || dpre == nullptr || !aligned16({pre, dpre})) return BP_ERR_SHAPE;
    bp::BiasGeluParams p{};
    p.x = grad; p.pre = const_cast<void *>(pre); p.y = dpre; p.dbias = dbias; p.ws = dbias != nullptr ? ws : nullptr;
    p.rows = rows; p.cols = cols; p.dbias_f32 = dbias_is_f32 ? 1 : 0;
    return launch_status(bp::launch_bias_gelu_bwd(p, dtype, true, static_cast<hipStream_t>(stream)));
}

int bp_column_sum(const void *grad, void *dbias, float *ws, int64_t rows, int cols, int dtype, int dbias_is_f32,
                  bp_stream_t stream) {
    const int rc = bias_grad_common(grad, dbias, ws, rows, cols, dtype);
    if (rc != BP_OK) return rc;
    if (dbias == nullptr) return BP_ERR_SHAPE;
    bp::BiasGeluParams p{};
    p.x = grad; p.dbias = dbias; p.ws = ws; p.rows = rows; p.cols = cols; p.dbias_f32 = dbias_is_f32 ? 1 : 0;
    return launch_status(bp::launch_bias_gelu_bwd(p, dtype, false, static_cast<hipStream_t>(stream)));
}

static int xent_common(int64_t rows, int cols, int64_t row_stride, float smoothing, int dtype) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16 && dtype != BP_DTYPE_F32) return BP_ERR_DTYPE;
    if (rows <= 0 || rows > 0x7fffffffLL || cols <= 0 || row_stride < cols) return BP_ERR_SHAPE;
    if (!(smoothing >= 0.f && smoothing < 1.f)) return BP_ERR_SCALE;
    return BP_OK;
}

int bp_xentropy_fwd(const void *logits, const int64_t *labels, float *losses, float *lse,
                    int64_t rows, int cols, int64_t row_stride, float smoothing, int total_classes,
                    int dtype, bp_stream_t stream) {
    const int rc = xent_common(rows, cols, row_stride, smoothing, dtype);
    if (rc != BP_OK) return rc;
    if (logits == nullptr || labels == nullptr || losses == nullptr || lse == nullptr) return BP_ERR_SHAPE;
    bp::XentParams p{};
    p.logits = logits; p.labels = labels; p.losses = losses; p.lse = lse;
    p.rows = rows; p.cols = cols; p.row_stride = row_stride;
    p.total_classes = total_classes > 0 ? total_classes : cols;
    p.smoothing = smoothing;
    return launch_status(bp::launch_xentropy_fwd(p, dtype, static_cast<hipStream_t>(stream)));
}

int bp_xentropy_bwd(const float *grad_losses, const void *logits, const float *lse, const int64_t *labels,
                    void *grad_logits, int64_t rows, int cols, int64_t row_stride, int64_t grad_row_stride,
                    float smoothing, int total_classes, int dtype, bp_stream_t stream) {
    const int rc = xent_common(rows, cols, row_stride, smoothing, dtype);
    if (rc != BP_OK) return rc;
    if (grad_row_stride < cols) return BP_ERR_SHAPE;
    if (grad_losses == nullptr || logits == nullptr || lse == nullptr || labels == nullptr ||
        grad_logits == nullptr)
        return BP_ERR_SHAPE;
    bp::XentParams p{};
    p.logits = logits; p.labels = labels; p.lse = const_cast<float *>(lse); p.grad_losses = grad_losses;
    p.grad_logits = grad_logits;
    p.rows = rows; p.cols = cols; p.row_stride = row_stride; p.grad_row_stride = grad_row_stride;
    p.total_classes = total_classes > 0 ? total_classes : cols;
    p.smoothing = smoothing;
    return launch_status(bp::launch_xentropy_bwd(p, dtype, static_cast<hipStream_t>(stream)));
}

// ---- KV-cached decoding (bp_flash_decode / bp_sense_decode{,_weighted} / bp_sense_rows_dot) ----

int64_t bp_flash_decode_ws_floats(int batch, int nheads, int head_dim, int max_seqlen) {
    if (batch <= 0 || nheads <= 0 || head_dim <= 0 || max_seqlen <= 0) return 0;
    return (int64_t)batch * nheads * bp::decode_nsplit(batch, nheads, max_seqlen) * (head_dim + 2);
}

int bp_flash_decode(const void *q, const void *k_new, const void *v_new, void *kv_cache, const int32_t *cache_seqlens,
                    void *out, float *softmax_lse, float *ws, int64_t ws_floats,
                    int batch, int nheads, int head_dim, int max_seqlen,
                    int64_t q_batch_stride, int64_t q_head_stride,
                    int64_t knew_batch_stride, int64_t knew_head_stride,
                    int64_t vnew_batch_stride, int64_t vnew_head_stride,
                    int64_t kv_batch_stride, int64_t kv_row_stride, int64_t kv_two_stride, int64_t kv_head_stride,
                    int64_t o_batch_stride, int64_t o_head_stride, int64_t lse_batch_stride,
                    float softmax_scale, int dtype, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (head_dim < 1 || head_dim > 128 || head_dim % 8 != 0) return BP_ERR_HEAD_DIM;
    if (batch <= 0 || batch > 65535 || nheads <= 0 || nheads > 65535 || max_seqlen <= 0) return BP_ERR_SHAPE;
    if (q == nullptr || k_new == nullptr || v_new == nullptr || kv_cache == nullptr || cache_seqlens == nullptr
        || out == nullptr || ws == nullptr)
        return BP_ERR_SHAPE;
    if (!aligned16({q, k_new, v_new, kv_cache, out, ws})) return BP_ERR_SHAPE;
    if (!strides8({q_batch_stride, q_head_stride, knew_batch_stride, knew_head_stride, vnew_batch_stride,
                   vnew_head_stride, kv_batch_stride, kv_row_stride, kv_two_stride, kv_head_stride, o_batch_stride,
                   o_head_stride}))
        return BP_ERR_SHAPE;
    if (softmax_lse != nullptr && lse_batch_stride < nheads) return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;
    if (ws_floats < bp_flash_decode_ws_floats(batch, nheads, head_dim, max_seqlen)) return BP_ERR_WORKSPACE;
    bp::DecodeParams p{};
    p.q = q; p.k_new = k_new; p.v_new = v_new;
    p.k_cache = kv_cache; p.v = static_cast<uint16_t *>(kv_cache) + kv_two_stride;
    p.q_bs = q_batch_stride; p.q_gs = q_head_stride;
    p.kn_bs = knew_batch_stride; p.kn_gs = knew_head_stride;
    p.vn_bs = vnew_batch_stride; p.vn_gs = vnew_head_stride;
    p.kc_bs = p.vc_bs = kv_batch_stride; p.kc_rs = p.vc_rs = kv_row_stride; p.kc_gs = p.vc_gs = kv_head_stride;
    p.seqlens = cache_seqlens;
    p.b = batch; p.groups = nheads; p.dk = p.dv = head_dim; p.max_seqlen = max_seqlen;
    p.nsplit = bp::decode_nsplit(batch, nheads, max_seqlen);
    p.ws_acc = ws;
    p.ws_ml = ws + (int64_t)batch * nheads * p.nsplit * head_dim;
    p.o = out; p.o_bs = o_batch_stride; p.o_gs = o_head_stride;
    p.lse = softmax_lse; p.lse_bs = lse_batch_stride;
    p.scale_log2e = softmax_scale * bp::kLog2e;
    return launch_status(bp::launch_flash_decode(p, dtype, static_cast<hipStream_t>(stream)));
}

int64_t bp_sense_decode_ws_floats(int batch, int nsenses, int d_out, int max_seqlen) {
    if (batch <= 0 || nsenses <= 0 || d_out <= 0 || max_seqlen <= 0) return 0;
    return (int64_t)batch * nsenses * bp::decode_nsplit(batch, nsenses, max_seqlen) * (d_out + 2);
}

int bp_sense_decode(const void *q, const void *k_new, void *k_cache, const void *table, int32_t *row_index,
                    const int32_t *new_row, const int32_t *cache_seqlens, void *out, float *ws, int64_t ws_floats,
                    int batch, int nsenses, int d_k, int d_out, int max_seqlen, int64_t table_rows,
                    int64_t q_batch_stride, int64_t q_sense_stride,
                    int64_t knew_batch_stride, int64_t knew_sense_stride,
                    int64_t kc_batch_stride, int64_t kc_row_stride, int64_t kc_sense_stride,
                    int64_t t_row_stride, int64_t t_sense_stride, int64_t idx_batch_stride,
                    int64_t o_batch_stride, float softmax_scale, int dtype, bp_stream_t stream) {
    return bp_sense_decode_weighted(q, k_new, k_cache, table, row_index, new_row, cache_seqlens, nullptr, out, ws,
                                    ws_floats, batch, nsenses, d_k, d_out, max_seqlen, table_rows, q_batch_stride,
                                    q_sense_stride, knew_batch_stride, knew_sense_stride, kc_batch_stride, kc_row_stride,
                                    kc_sense_stride, t_row_stride, t_sense_stride, idx_batch_stride, o_batch_stride, 0, 0,
                                    softmax_scale, dtype, stream);
}

int bp_sense_decode_weighted(const void *q, const void *k_new, void *k_cache, const void *table, int32_t *row_index,
                             const int32_t *new_row, const int32_t *cache_seqlens, const float *key_weight, void *out,
                             float *ws, int64_t ws_floats,
                             int batch, int nsenses, int d_k, int d_out, int max_seqlen, int64_t table_rows,
                             int64_t q_batch_stride, int64_t q_sense_stride,
                             int64_t knew_batch_stride, int64_t knew_sense_stride,
                             int64_t kc_batch_stride, int64_t kc_row_stride, int64_t kc_sense_stride,
                             int64_t t_row_stride, int64_t t_sense_stride, int64_t idx_batch_stride,
                             int64_t o_batch_stride, int64_t kw_batch_stride, int64_t kw_sense_stride,
                             float softmax_scale, int dtype, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (d_k < 1 || d_k > bp::kWideMaxDk || d_k % 8 != 0) return BP_ERR_HEAD_DIM;
    if (d_out < 1) return BP_ERR_DOUT;
    if (d_out % 8 != 0 || d_out > 2048) return BP_ERR_SHAPE;
    if (batch <= 0 || batch > 65535 || nsenses <= 0 || nsenses > 64 || max_seqlen <= 0 || table_rows <= 0
        || table_rows > 0x7fffffffLL)
        return BP_ERR_SHAPE;
    if (q == nullptr || k_new == nullptr || k_cache == nullptr || table == nullptr || row_index == nullptr
        || new_row == nullptr || cache_seqlens == nullptr || out == nullptr || ws == nullptr)
        return BP_ERR_SHAPE;
    if (!aligned16({q, k_new, k_cache, table, out, ws})) return BP_ERR_SHAPE;
    if (!strides8({q_batch_stride, q_sense_stride, knew_batch_stride, knew_sense_stride, kc_batch_stride, kc_row_stride,
                   kc_sense_stride, t_row_stride, t_sense_stride, o_batch_stride}))
        return BP_ERR_SHAPE;
    // a weight row holds max_seqlen entries; rows of different (sample, sense) pairs do not overlap
    if (key_weight != nullptr && (kw_sense_stride < max_seqlen || kw_batch_stride < max_seqlen)) return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;
    if (ws_floats < bp_sense_decode_ws_floats(batch, nsenses, d_out, max_seqlen)) return BP_ERR_WORKSPACE;
    bp::DecodeParams p{};
    p.q = q; p.k_new = k_new; p.k_cache = k_cache; p.v = const_cast<void *>(table);
    p.q_bs = q_batch_stride; p.q_gs = q_sense_stride;
    p.kn_bs = knew_batch_stride; p.kn_gs = knew_sense_stride;
    p.kc_bs = kc_batch_stride; p.kc_rs = kc_row_stride; p.kc_gs = kc_sense_stride;
    p.vc_rs = t_row_stride; p.vc_gs = t_sense_stride;
    p.row_index = row_index; p.ri_bs = idx_batch_stride; p.new_row = new_row; p.table_rows = table_rows;
    p.seqlens = cache_seqlens;
    p.b = batch; p.groups = nsenses; p.dk = d_k; p.dv = d_out; p.max_seqlen = max_seqlen;
    p.nsplit = bp::decode_nsplit(batch, nsenses, max_seqlen);
    p.ws_acc = ws;
    p.ws_ml = ws + (int64_t)batch * nsenses * p.nsplit * d_out;
    p.o = out; p.o_bs = o_batch_stride;
    p.scale_log2e = softmax_scale * bp::kLog2e;
    if (key_weight == nullptr) return launch_status(bp::launch_sense_decode(p, dtype, static_cast<hipStream_t>(stream)));
    p.key_weight = key_weight; p.kw_bs = kw_batch_stride; p.kw_gs = kw_sense_stride;
    return launch_status(bp::launch_sense_decode_weighted(p, dtype, static_cast<hipStream_t>(stream)));
}

int bp_sense_rows_dot(const void *table, const int32_t *row_index, const int32_t *new_row, const int32_t *cache_seqlens,
                      const void *vec, float *out,
                      int batch, int nsenses, int d_out, int max_seqlen, int64_t table_rows,
                      int64_t t_row_stride, int64_t t_sense_stride, int64_t idx_batch_stride, int64_t vec_batch_stride,
                      int64_t o_batch_stride, int64_t o_sense_stride, int dtype, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (d_out < 1) return BP_ERR_DOUT;
    if (d_out % 8 != 0 || d_out > 2048) return BP_ERR_SHAPE;
    if (batch <= 0 || batch > 65535 || nsenses <= 0 || nsenses > 64 || max_seqlen <= 0 || table_rows <= 0
        || table_rows > 0x7fffffffLL)
        return BP_ERR_SHAPE;
    if (table == nullptr || row_index == nullptr || new_row == nullptr || cache_seqlens == nullptr || vec == nullptr
        || out == nullptr)
        return BP_ERR_SHAPE;
    if (!aligned16({table, vec})) return BP_ERR_SHAPE;
    if (!strides8({t_row_stride, t_sense_stride, vec_batch_stride})) return BP_ERR_SHAPE;
    if (o_sense_stride < max_seqlen || o_batch_stride < max_seqlen) return BP_ERR_SHAPE;
    bp::RowsDotParams p{};
    p.table = table; p.vec = vec; p.row_index = row_index; p.new_row = new_row; p.seqlens = cache_seqlens; p.out = out;
    p.t_rs = t_row_stride; p.t_gs = t_sense_stride; p.ri_bs = idx_batch_stride; p.v_bs = vec_batch_stride;
    p.o_bs = o_batch_stride; p.o_gs = o_sense_stride; p.table_rows = table_rows;
    p.b = batch; p.groups = nsenses; p.dout = d_out; p.max_seqlen = max_seqlen;
    return launch_status(bp::launch_sense_rows_dot(p, dtype, static_cast<hipStream_t>(stream)));
}

// ---- token selection (bp_pick_token, bp_pick_token_ctl, bp_pick_token_lim, bp_pick_token_lim_rows) ----

// the argument checks of bp_pick_token and the parameters they admit; bp_pick_token_ctl adds its own behind them
static int pick_params(bp::PickParams &p, const void *logits, int64_t *tokens, int64_t *sequences, float *stats,
                       const uint64_t *rng_state, const int32_t *counters, int batch, int vocab, int64_t row_stride,
                       int64_t tokens_stride, int64_t seq_stride, int seq_cols, int do_sample, float temperature, int top_k,
                       float top_p, int dtype) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16 && dtype != BP_DTYPE_F32) return BP_ERR_DTYPE;
    if (batch <= 0 || vocab <= 0 || vocab > (1 << 23) || row_stride < vocab || tokens_stride < 1) return BP_ERR_SHAPE;
    if (logits == nullptr || tokens == nullptr) return BP_ERR_SHAPE;
    if (sequences != nullptr && (seq_cols < 1 || seq_stride < seq_cols)) return BP_ERR_SHAPE;
    const uintptr_t elem = dtype == BP_DTYPE_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(logits) % elem || reinterpret_cast<uintptr_t>(tokens) % 8
        || reinterpret_cast<uintptr_t>(sequences) % 8 || reinterpret_cast<uintptr_t>(stats) % 4
        || reinterpret_cast<uintptr_t>(rng_state) % 8 || reinterpret_cast<uintptr_t>(counters) % 4)
        return BP_ERR_SHAPE;
    if (!scale_ok(temperature) || !scale_ok(1.f / temperature)) return BP_ERR_SCALE;
    if (!(top_p > 0.f && top_p <= 1.f)) return BP_ERR_SAMPLING;
    if (do_sample && rng_state == nullptr) return BP_ERR_SAMPLING;
    p.logits = logits; p.tokens = tokens; p.sequences = sequences; p.stats = stats; p.rng_state = rng_state;
    p.counters = counters;
    p.row_stride = row_stride; p.tokens_stride = tokens_stride; p.seq_stride = seq_stride;
    p.batch = batch; p.vocab = vocab; p.seq_cols = seq_cols;
    p.do_sample = do_sample ? 1 : 0; p.top_k = top_k;
    p.inv_t = 1.f / temperature; p.top_p = top_p;
    p.finished = nullptr; p.theta = p.inv_theta = 1.f; p.eos = -1; p.pad = 0; p.min_length = 0;
    return BP_OK;
}

int bp_pick_token(const void *logits, int64_t *tokens, int64_t *sequences, float *stats, const uint64_t *rng_state,
                  const int32_t *counters, int batch, int vocab, int64_t row_stride, int64_t tokens_stride,
                  int64_t seq_stride, int seq_cols, int do_sample, float temperature, int top_k, float top_p, int dtype,
                  bp_stream_t stream) {
    bp::PickParams p{};
    const int e = pick_params(p, logits, tokens, sequences, stats, rng_state, counters, batch, vocab, row_stride,
                              tokens_stride, seq_stride, seq_cols, do_sample, temperature, top_k, top_p, dtype);
    if (e != BP_OK) return e;
    return launch_status(bp::launch_pick_token(p, dtype, static_cast<hipStream_t>(stream)));
}

// the checks bp_pick_token_ctl adds behind pick_params, and its parameters
static int pick_ctl_params(bp::PickParams &p, const int64_t *sequences, int32_t *finished, int vocab, float repetition_penalty,
                           int eos_token_id, int pad_token_id, int min_length) {
    if (!scale_ok(repetition_penalty) || !scale_ok(1.f / repetition_penalty)) return BP_ERR_SAMPLING;
    if (repetition_penalty != 1.f && sequences == nullptr) return BP_ERR_SAMPLING;
    if (eos_token_id >= 0 && finished == nullptr) return BP_ERR_SAMPLING;
    if (eos_token_id >= vocab || min_length < 0 || reinterpret_cast<uintptr_t>(finished) % 4) return BP_ERR_SHAPE;
    if (finished != nullptr && (pad_token_id < 0 || pad_token_id >= vocab)) return BP_ERR_SHAPE;
    if (repetition_penalty != 1.f && vocab > (1 << 19)) return BP_ERR_SHAPE;   // the history bitmap: 64 KB of LDS at most
    p.finished = finished;
    p.theta = repetition_penalty; p.inv_theta = 1.f / repetition_penalty;
    p.eos = eos_token_id < 0 ? -1 : eos_token_id; p.pad = pad_token_id; p.min_length = min_length;
    return BP_OK;
}

int bp_pick_token_ctl(const void *logits, int64_t *tokens, int64_t *sequences, float *stats, const uint64_t *rng_state,
                      const int32_t *counters, int32_t *finished,
                      int batch, int vocab, int64_t row_stride, int64_t tokens_stride, int64_t seq_stride, int seq_cols,
                      int do_sample, float temperature, int top_k, float top_p,
                      float repetition_penalty, int eos_token_id, int pad_token_id, int min_length,
                      int dtype, bp_stream_t stream) {
    bp::PickParams p{};
    int e = pick_params(p, logits, tokens, sequences, stats, rng_state, counters, batch, vocab, row_stride,
                        tokens_stride, seq_stride, seq_cols, do_sample, temperature, top_k, top_p, dtype);
    if (e != BP_OK) return e;
    e = pick_ctl_params(p, sequences, finished, vocab, repetition_penalty, eos_token_id, pad_token_id, min_length);
    if (e != BP_OK) return e;
    return launch_status(bp::launch_pick_token_ctl(p, dtype, static_cast<hipStream_t>(stream)));
}

// bp_pick_token_lim and bp_pick_token_lim_rows: every check and every parameter; the two arrays are NULL for the former, and a
// scalar is only read (and checked) where its array is NULL
static int pick_lim_params(bp::PickParams &p, const void *logits, int64_t *tokens, int64_t *sequences, float *stats,
                           const uint64_t *rng_state, const int32_t *counters, int32_t *finished,
                           int batch, int vocab, int64_t row_stride, int64_t tokens_stride, int64_t seq_stride, int seq_cols,
                           int do_sample, float temperature, int top_k, float top_p,
                           float repetition_penalty, int eos_token_id, int pad_token_id, int min_length,
                           int no_repeat_ngram_size, float frequency_penalty, float presence_penalty, int penalty_begin,
                           const int32_t *suppress_ids, int n_suppress, const int32_t *penalty_begins,
                           const int32_t *min_lengths, int dtype) {
    if (penalty_begins != nullptr) penalty_begin = 0;
    if (min_lengths != nullptr) min_length = 0;
    int e = pick_params(p, logits, tokens, sequences, stats, rng_state, counters, batch, vocab, row_stride,
                        tokens_stride, seq_stride, seq_cols, do_sample, temperature, top_k, top_p, dtype);
    if (e != BP_OK) return e;
    e = pick_ctl_params(p, sequences, finished, vocab, repetition_penalty, eos_token_id, pad_token_id, min_length);
    if (e != BP_OK) return e;
    if (!(fabsf(frequency_penalty) < INFINITY) || !(fabsf(presence_penalty) < INFINITY)) return BP_ERR_SAMPLING;
    const bool counted = frequency_penalty != 0.f || presence_penalty != 0.f;
    if ((no_repeat_ngram_size > 0 || counted) && sequences == nullptr) return BP_ERR_SAMPLING;
    if (n_suppress > 0 && (suppress_ids == nullptr || reinterpret_cast<uintptr_t>(suppress_ids) % 4)) return BP_ERR_SAMPLING;
    if (no_repeat_ngram_size < 0 || no_repeat_ngram_size > BP_PICK_MAX_NGRAM || n_suppress < 0 || penalty_begin < 0)
        return BP_ERR_SHAPE;
    if (reinterpret_cast<uintptr_t>(penalty_begins) % 4 || reinterpret_cast<uintptr_t>(min_lengths) % 4) return BP_ERR_SHAPE;
    const bool limited = no_repeat_ngram_size > 0 || counted || n_suppress > 0;
    if (limited && vocab > BP_PICK_MAX_LIMITED_VOCAB) return BP_ERR_SHAPE;   // 19 id bits of a table entry, 64 KB per bitmap
    if (counted && seq_cols > BP_PICK_MAX_COUNTED_COLS) return BP_ERR_SHAPE;  // 13 count bits of a table entry
    p.suppress = n_suppress > 0 ? suppress_ids : nullptr; p.n_suppress = n_suppress;
    p.ngram = no_repeat_ngram_size; p.penalty_begin = penalty_begin;
    p.freq_pen = frequency_penalty; p.pres_pen = presence_penalty;
    p.table_shift = counted ? bp::lim_table_shift(seq_cols) : 31;
    p.penalty_begins = penalty_begins; p.min_lengths = min_lengths;
    if (bp::pick_lim_lds_bytes(p) > BP_PICK_MAX_LDS_BYTES) return BP_ERR_SHAPE;
    return BP_OK;
}

int bp_pick_token_lim(const void *logits, int64_t *tokens, int64_t *sequences, float *stats, const uint64_t *rng_state,
                      const int32_t *counters, int32_t *finished,
                      int batch, int vocab, int64_t row_stride, int64_t tokens_stride, int64_t seq_stride, int seq_cols,
                      int do_sample, float temperature, int top_k, float top_p,
                      float repetition_penalty, int eos_token_id, int pad_token_id, int min_length,
                      int no_repeat_ngram_size, float frequency_penalty, float presence_penalty, int penalty_begin,
                      const int32_t *suppress_ids, int n_suppress, int dtype, bp_stream_t stream) {
    bp::PickParams p{};
    const int e = pick_lim_params(p, logits, tokens, sequences, stats, rng_state, counters, finished, batch, vocab, row_stride,
                                  tokens_stride, seq_stride, seq_cols, do_sample, temperature, top_k, top_p, repetition_penalty,
                                  eos_token_id, pad_token_id, min_length, no_repeat_ngram_size, frequency_penalty,
                                  presence_penalty, penalty_begin, suppress_ids, n_suppress, nullptr, nullptr, dtype);
    if (e != BP_OK) return e;
    return launch_status(bp::launch_pick_token_lim(p, dtype, static_cast<hipStream_t>(stream)));
}

int bp_pick_token_lim_rows(const void *logits, int64_t *tokens, int64_t *sequences, float *stats, const uint64_t *rng_state,
                           const int32_t *counters, int32_t *finished,
                           int batch, int vocab, int64_t row_stride, int64_t tokens_stride, int64_t seq_stride, int seq_cols,
                           int do_sample, float temperature, int top_k, float top_p,
                           float repetition_penalty, int eos_token_id, int pad_token_id, int min_length,
                           int no_repeat_ngram_size, float frequency_penalty, float presence_penalty, int penalty_begin,
                           const int32_t *suppress_ids, int n_suppress, const int32_t *penalty_begins,
                           const int32_t *min_lengths, int dtype, bp_stream_t stream) {
    bp::PickParams p{};
    const int e = pick_lim_params(p, logits, tokens, sequences, stats, rng_state, counters, finished, batch, vocab, row_stride,
                                  tokens_stride, seq_stride, seq_cols, do_sample, temperature, top_k, top_p, repetition_penalty,
                                  eos_token_id, pad_token_id, min_length, no_repeat_ngram_size, frequency_penalty,
                                  presence_penalty, penalty_begin, suppress_ids, n_suppress, penalty_begins, min_lengths, dtype);
    if (e != BP_OK) return e;
    return launch_status(bp::launch_pick_token_rows(p, dtype, static_cast<hipStream_t>(stream)));
}

// one phrase list of bp_pick_token_phrases: the checks the host can make (the contents stay on the device, unread)
static int pick_phrase_list(const int32_t *ids, const int32_t *offsets, int n, int total, const int64_t *sequences) {
    if (n < 0 || total < 0 || n > BP_PICK_MAX_PHRASES) return BP_ERR_SHAPE;
    if (reinterpret_cast<uintptr_t>(ids) % 4 || reinterpret_cast<uintptr_t>(offsets) % 4) return BP_ERR_SHAPE;
    if (n > 0 && (ids == nullptr || offsets == nullptr || sequences == nullptr)) return BP_ERR_SAMPLING;
    return BP_OK;
}

int bp_pick_token_phrases(const void *logits, int64_t *tokens, int64_t *sequences, float *stats, const uint64_t *rng_state,
                          const int32_t *counters, int32_t *finished,
                          int batch, int vocab, int64_t row_stride, int64_t tokens_stride, int64_t seq_stride, int seq_cols,
                          int do_sample, float temperature, int top_k, float top_p,
                          float repetition_penalty, int eos_token_id, int pad_token_id, int min_length,
                          int no_repeat_ngram_size, float frequency_penalty, float presence_penalty, int penalty_begin,
                          const int32_t *suppress_ids, int n_suppress, const int32_t *penalty_begins,
                          const int32_t *min_lengths,
                          const int32_t *ban_ids, const int32_t *ban_offsets, int n_ban, int ban_total,
                          const int32_t *stop_ids, const int32_t *stop_offsets, int n_stop, int stop_total,
                          int32_t *ends, int32_t *reasons, int dtype, bp_stream_t stream) {
    static_assert(BP_PICK_MAX_PHRASE_LEN == bp::kMaxPhraseLen && BP_PICK_MAX_PHRASES == bp::kMaxPhrases, "bp_hip.h and bp_kernels.h");
    bp::PickParams p{};
    int e = pick_lim_params(p, logits, tokens, sequences, stats, rng_state, counters, finished, batch, vocab, row_stride,
                            tokens_stride, seq_stride, seq_cols, do_sample, temperature, top_k, top_p, repetition_penalty,
                            eos_token_id, pad_token_id, min_length, no_repeat_ngram_size, frequency_penalty,
                            presence_penalty, penalty_begin, suppress_ids, n_suppress, penalty_begins, min_lengths, dtype);
    if (e != BP_OK) return e;
    e = pick_phrase_list(ban_ids, ban_offsets, n_ban, ban_total, sequences);
    if (e != BP_OK) return e;
    e = pick_phrase_list(stop_ids, stop_offsets, n_stop, stop_total, sequences);
    if (e != BP_OK) return e;
    if (n_stop > 0 && finished == nullptr) return BP_ERR_SAMPLING;
    if (reinterpret_cast<uintptr_t>(ends) % 4 || reinterpret_cast<uintptr_t>(reasons) % 4) return BP_ERR_SHAPE;
    if (n_ban > 0 && vocab > BP_PICK_MAX_LIMITED_VOCAB) return BP_ERR_SHAPE;   // the ban bitmap: 64 KB of LDS at most
    p.ban_ids = n_ban > 0 ? ban_ids : nullptr; p.ban_offsets = n_ban > 0 ? ban_offsets : nullptr;
    p.n_ban = n_ban; p.ban_total = ban_total;
    p.stop_ids = n_stop > 0 ? stop_ids : nullptr; p.stop_offsets = n_stop > 0 ? stop_offsets : nullptr;
    p.n_stop = n_stop; p.stop_total = stop_total;
    p.ends = ends; p.reasons = reasons;
    if (bp::pick_phrases_lds_bytes(p) > BP_PICK_MAX_LDS_BYTES) return BP_ERR_SHAPE;
    return launch_status(bp::launch_pick_token_phrases(p, dtype, static_cast<hipStream_t>(stream)));
}

// ---- beam search (bp_beam_pick, bp_beam_copy_rows) ----

int64_t bp_beam_pick_ws_floats(int groups, int beam_width) {
    if (groups < 1 || beam_width < 1 || beam_width > 8) return 0;
    return (int64_t)groups * beam_width * 16;   // eight 64-bit keys a row
}

int bp_beam_pick(const void *logits, float *beam_scores, int32_t *finished, int32_t *parent, int64_t *tokens,
                 int64_t *sequences, const int32_t *counters, float *ws, int64_t ws_floats,
                 int groups, int beam_width, int vocab, int64_t row_stride, int64_t tokens_stride, int64_t seq_stride,
                 int seq_cols, int eos_token_id, int pad_token_id, int dtype, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16 && dtype != BP_DTYPE_F32) return BP_ERR_DTYPE;
    if (groups < 1 || beam_width < 1 || beam_width > 8 || (int64_t)groups * beam_width > 0x7fffffffLL) return BP_ERR_SHAPE;
    if (vocab < beam_width || vocab > (1 << 23) || row_stride < vocab || tokens_stride < 1) return BP_ERR_SHAPE;
    if (logits == nullptr || beam_scores == nullptr || parent == nullptr || tokens == nullptr || ws == nullptr)
        return BP_ERR_SHAPE;
    if (sequences != nullptr && (seq_cols < 1 || seq_stride < seq_cols)) return BP_ERR_SHAPE;
    const uintptr_t elem = dtype == BP_DTYPE_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(logits) % elem || reinterpret_cast<uintptr_t>(beam_scores) % 4
        || reinterpret_cast<uintptr_t>(finished) % 4 || reinterpret_cast<uintptr_t>(parent) % 4
        || reinterpret_cast<uintptr_t>(tokens) % 8 || reinterpret_cast<uintptr_t>(sequences) % 8
        || reinterpret_cast<uintptr_t>(counters) % 4 || reinterpret_cast<uintptr_t>(ws) % 8)
        return BP_ERR_SHAPE;
    if (eos_token_id >= vocab) return BP_ERR_SHAPE;
    if (finished != nullptr && (pad_token_id < 0 || pad_token_id >= vocab)) return BP_ERR_SHAPE;
    if (eos_token_id >= 0 && finished == nullptr) return BP_ERR_SAMPLING;
    if (ws_floats < bp_beam_pick_ws_floats(groups, beam_width)) return BP_ERR_WORKSPACE;
    bp::BeamPickParams p{};
    p.logits = logits; p.beam_scores = beam_scores; p.finished = finished; p.parent = parent; p.tokens = tokens;
    p.sequences = sequences; p.counters = counters; p.ws = ws;
    p.row_stride = row_stride; p.tokens_stride = tokens_stride; p.seq_stride = seq_stride;
    p.groups = groups; p.beam_width = beam_width; p.vocab = vocab; p.seq_cols = seq_cols;
    p.eos = eos_token_id < 0 ? -1 : eos_token_id; p.pad = finished != nullptr ? pad_token_id : 0;
    return launch_status(bp::launch_beam_pick(p, dtype, static_cast<hipStream_t>(stream)));
}

int bp_beam_copy_rows(const void *const *bases, const int64_t *row_strides, const int64_t *pos_bytes, int nsets,
                      const int32_t *parent, const int32_t *lengths, int rows, int first_position, int max_positions,
                      bp_stream_t stream) {
    if (nsets < 1 || nsets > bp::kBeamCopyMaxSets || rows < 1 || rows > 65535) return BP_ERR_SHAPE;
    if (bases == nullptr || row_strides == nullptr || pos_bytes == nullptr || parent == nullptr || lengths == nullptr)
        return BP_ERR_SHAPE;
    if (reinterpret_cast<uintptr_t>(parent) % 4 || reinterpret_cast<uintptr_t>(lengths) % 4) return BP_ERR_SHAPE;
    if (first_position < 0 || max_positions < 0) return BP_ERR_SHAPE;
    bp::BeamCopyParams p{};
    for (int i = 0; i < nsets; ++i) {
        if (bases[i] == nullptr || !aligned16(bases[i])) return BP_ERR_SHAPE;
        if (pos_bytes[i] < 4 || pos_bytes[i] % 4 != 0 || row_strides[i] % 16 != 0) return BP_ERR_SHAPE;
        if (row_strides[i] < pos_bytes[i] * (int64_t)max_positions) return BP_ERR_SHAPE;   // a row holds its positions
        p.base[i] = const_cast<void *>(bases[i]); p.row_stride[i] = row_strides[i]; p.pos_bytes[i] = pos_bytes[i];
    }
    p.parent = parent; p.lengths = lengths;
    p.nsets = nsets; p.rows = rows; p.first_position = first_position; p.max_positions = max_positions;
    return launch_status(bp::launch_beam_copy_rows(p, static_cast<hipStream_t>(stream)));
}

// ---- packed rows into padded buffers (bp_scatter_packed_rows) ----

int bp_scatter_packed_rows(const void *const *src, const int64_t *src_row_strides, void *const *dst,
                           const int64_t *dst_batch_strides, const int64_t *dst_pos_strides, const int64_t *row_bytes,
                           int nsets, const int32_t *cu_seqlens, int batch, int64_t total_rows, int max_seqlen,
                           int max_positions, bp_stream_t stream) {
    if (nsets < 1 || nsets > bp::kScatterMaxSets || batch < 1 || batch > 65535) return BP_ERR_SHAPE;
    if (src == nullptr || src_row_strides == nullptr || dst == nullptr || dst_batch_strides == nullptr
        || dst_pos_strides == nullptr || row_bytes == nullptr || cu_seqlens == nullptr)
        return BP_ERR_SHAPE;
    if (reinterpret_cast<uintptr_t>(cu_seqlens) % 4) return BP_ERR_SHAPE;
    if (max_seqlen < 0 || max_positions < 0 || total_rows < 0) return BP_ERR_SHAPE;
    bp::ScatterRowsParams p{};
    for (int i = 0; i < nsets; ++i) {
        if (src[i] == nullptr || dst[i] == nullptr) return BP_ERR_SHAPE;
        const uintptr_t all = reinterpret_cast<uintptr_t>(src[i]) | reinterpret_cast<uintptr_t>(dst[i])
            | (uintptr_t)src_row_strides[i] | (uintptr_t)dst_batch_strides[i] | (uintptr_t)dst_pos_strides[i]
            | (uintptr_t)row_bytes[i];
        if (all % 4 != 0 || row_bytes[i] < 4 || dst_batch_strides[i] < 0) return BP_ERR_SHAPE;
        if (row_bytes[i] > src_row_strides[i] || row_bytes[i] > dst_pos_strides[i]) return BP_ERR_SHAPE;
        p.src[i] = src[i]; p.dst[i] = dst[i]; p.src_row_stride[i] = src_row_strides[i];
        p.dst_batch_stride[i] = dst_batch_strides[i]; p.dst_pos_stride[i] = dst_pos_strides[i]; p.row_bytes[i] = row_bytes[i];
        if (all % 16 == 0) p.wide |= 1u << i;
    }
    p.cu_seqlens = cu_seqlens; p.total_rows = total_rows;
    p.nsets = nsets; p.batch = batch; p.limit = max_seqlen < max_positions ? max_seqlen : max_positions;
    return launch_status(bp::launch_scatter_packed_rows(p, static_cast<hipStream_t>(stream)));
}

// ---- segmented row sums (bp_segment_sum_rows) ----

int bp_segment_sum_rows(const void *rows, const int32_t *order, const int32_t *seg_begin, float *acc, int64_t n_rows,
                        int64_t n_segments, int cols, int64_t rows_stride, int64_t acc_stride, int accumulate, int dtype,
                        bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (n_rows < 0 || n_rows > 0x7fffffffLL || n_segments < 0 || n_segments > BP_SEGMENT_SUM_MAX_SEGMENTS) return BP_ERR_SHAPE;
    if (cols < 8 || cols > BP_SEGMENT_SUM_MAX_COLS || !mult8(cols)) return BP_ERR_SHAPE;
    if (rows_stride < cols || !mult8(rows_stride) || acc_stride < cols || acc_stride % 4 != 0) return BP_ERR_SHAPE;
    if (accumulate != 0 && accumulate != 1) return BP_ERR_SHAPE;
    if (rows == nullptr || order == nullptr || seg_begin == nullptr || acc == nullptr) return BP_ERR_SHAPE;
    if (!aligned16({rows, acc}) || reinterpret_cast<uintptr_t>(order) % 4 || reinterpret_cast<uintptr_t>(seg_begin) % 4)
        return BP_ERR_SHAPE;
    bp::SegmentSumParams p{};
    p.rows = static_cast<const uint16_t *>(rows); p.order = order; p.seg_begin = seg_begin; p.acc = acc;
    p.rows_stride = rows_stride; p.acc_stride = acc_stride;
    p.n_rows = (int)n_rows; p.n_segments = (int)n_segments; p.cols = cols; p.accumulate = accumulate;
    return launch_status(bp::launch_segment_sum_rows(p, dtype, static_cast<hipStream_t>(stream)));
}

// ---- row extremes (bp_row_extremes) ----

int bp_row_extremes(const void *logits, float *top_val, int32_t *top_idx, float *bot_val, int32_t *bot_idx,
                    int rows, int cols, int64_t row_stride, int n, int dtype, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16 && dtype != BP_DTYPE_F32) return BP_ERR_DTYPE;
    // (the row reader rounds cols up by a 16-byte chunk at either end in 32-bit arithmetic: 16 columns of head room)
    if (rows < 0 || cols < 1 || cols > 0x7fffffff - 16 || row_stride < cols) return BP_ERR_SHAPE;
    if (n < 1 || n > BP_ROW_EXTREMES_MAX_N || n > cols) return BP_ERR_SHAPE;
    const uintptr_t elem = dtype == BP_DTYPE_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(logits) % elem || reinterpret_cast<uintptr_t>(top_val) % 4
        || reinterpret_cast<uintptr_t>(top_idx) % 4 || reinterpret_cast<uintptr_t>(bot_val) % 4
        || reinterpret_cast<uintptr_t>(bot_idx) % 4)
        return BP_ERR_SHAPE;
    if (rows == 0) return BP_OK;
    if (logits == nullptr) return BP_ERR_SHAPE;
    if (top_val == nullptr && top_idx == nullptr && bot_val == nullptr && bot_idx == nullptr) return BP_OK;   // nothing asked for
    bp::RowExtremesParams p{};
    p.logits = logits; p.top_val = top_val; p.top_idx = top_idx; p.bot_val = bot_val; p.bot_idx = bot_idx;
    p.row_stride = row_stride; p.rows = rows; p.cols = cols; p.n = n;
    return launch_status(bp::launch_row_extremes(p, dtype, static_cast<hipStream_t>(stream)));
}

// ---- sense attribution (bp_sense_attribute) ----

int64_t bp_sense_attribute_ws_floats(int nq, int nsenses) {
    if (nq <= 0 || nsenses <= 0) return 0;
    return (int64_t)nq * nsenses * 2;
}

int bp_sense_attribute(const void *qk, const void *table, const int32_t *row_index, const int32_t *query_sample,
                       const int32_t *query_pos, const float *vec, float *out, float *probs, float *ws, int64_t ws_floats,
                       int batch, int seqlen, int nsenses, int d_k, int d_out, int nq, int nvec, int64_t table_rows,
                       int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride, int64_t qk_sense_stride,
                       int64_t t_row_stride, int64_t t_sense_stride, int64_t idx_batch_stride,
                       int64_t v_query_stride, int64_t v_vec_stride,
                       int64_t o_query_stride, int64_t o_vec_stride, int64_t o_sense_stride,
                       int64_t p_query_stride, int64_t p_sense_stride,
                       float softmax_scale, int dtype, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (d_k < 1 || d_k > bp::kWideMaxDk || d_k % 8 != 0) return BP_ERR_HEAD_DIM;
    if (d_out < 1 || d_out % 8 != 0 || d_out > 2048) return BP_ERR_DOUT;
    if (nq < 1 || nq > 65535 || nvec < 1 || nvec > bp::kAttributeMaxVecs || nsenses < 1 || nsenses > 64 || batch < 1
        || seqlen < 1 || table_rows < 1 || table_rows > 0x7fffffffLL)
        return BP_ERR_SHAPE;
    if (qk == nullptr || table == nullptr || row_index == nullptr || query_sample == nullptr || query_pos == nullptr
        || vec == nullptr || out == nullptr || ws == nullptr)
        return BP_ERR_SHAPE;
    const uint16_t *qp = static_cast<const uint16_t *>(qk);
    if (!aligned16({qp, qp + qk_two_stride, table, vec})) return BP_ERR_SHAPE;
    if (!strides8({qk_batch_stride, qk_row_stride, qk_two_stride, qk_sense_stride, t_row_stride, t_sense_stride}))
        return BP_ERR_SHAPE;
    if ((v_query_stride & 3) != 0 || (v_vec_stride & 3) != 0) return BP_ERR_SHAPE;
    for (const void *p4 : {(const void *)row_index, (const void *)query_sample, (const void *)query_pos, (const void *)out,
                           (const void *)probs, (const void *)ws})
        if (reinterpret_cast<uintptr_t>(p4) % 4) return BP_ERR_SHAPE;
    // rows of different (query, vector, sense) triples do not overlap
    if (o_sense_stride < seqlen || (nvec > 1 && o_vec_stride < nsenses * o_sense_stride)
        || (nq > 1 && o_query_stride < nvec * o_vec_stride))
        return BP_ERR_SHAPE;
    if (probs != nullptr && (p_sense_stride < seqlen || (nq > 1 && p_query_stride < nsenses * p_sense_stride)))
        return BP_ERR_SHAPE;
    if (!scale_ok(softmax_scale)) return BP_ERR_SCALE;
    if (ws_floats < bp_sense_attribute_ws_floats(nq, nsenses)) return BP_ERR_WORKSPACE;
    bp::AttributeParams p{};
    p.q = qp; p.k = qp + qk_two_stride; p.table = table;
    p.row_index = row_index; p.query_sample = query_sample; p.query_pos = query_pos;
    p.vec = vec; p.out = out; p.probs = probs; p.ws = ws;
    p.qk_bs = qk_batch_stride; p.qk_rs = qk_row_stride; p.qk_ss = qk_sense_stride;
    p.t_rs = t_row_stride; p.t_gs = t_sense_stride; p.ri_bs = idx_batch_stride;
    p.v_qs = v_query_stride; p.v_vs = v_vec_stride;
    p.o_qs = o_query_stride; p.o_vs = o_vec_stride; p.o_gs = o_sense_stride;
    p.p_qs = p_query_stride; p.p_gs = p_sense_stride; p.table_rows = table_rows;
    p.b = batch; p.s = seqlen; p.groups = nsenses; p.dk = d_k; p.dout = d_out; p.nq = nq; p.nvec = nvec;
    p.scale = softmax_scale;
    return launch_status(bp::launch_sense_attribute(p, dtype, static_cast<hipStream_t>(stream)));
}

// ---- sense similarity (bp_sense_similarity) ----

int bp_sense_similarity(const void *table, const int32_t *cand_index, const void *query,
                        float *flat, float *min_pair, float *max_pair, float *min_all, float *max_all, float *per_sense,
                        int64_t ncand, int nsenses, int d, int nq, int64_t table_rows,
                        int64_t t_row_stride, int64_t t_sense_stride, int64_t q_query_stride, int64_t q_sense_stride,
                        int64_t o_query_stride, int64_t ps_query_stride, int64_t ps_sense_stride,
                        int dtype, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16) return BP_ERR_DTYPE;
    if (d < 1 || d % 8 != 0 || d > 2048) return BP_ERR_DOUT;
    if (nsenses < 1 || nsenses > 64 || (nsenses & (nsenses - 1)) != 0) return BP_ERR_SHAPE;   // 1, 2, 4, ..., 64
    if (nq < 1 || (int64_t)nq * nsenses > BP_SIMILARITY_MAX_QUERY_ROWS) return BP_ERR_SHAPE;
    if (ncand < 0 || ncand > 0x7fffffffLL || table_rows < 1 || table_rows > 0x7fffffffLL) return BP_ERR_SHAPE;
    if (flat == nullptr && min_pair == nullptr && max_pair == nullptr && min_all == nullptr && max_all == nullptr
        && per_sense == nullptr)
        return BP_ERR_SHAPE;
    if (cand_index == nullptr && ncand > table_rows) return BP_ERR_SHAPE;
    if (ncand == 0) return BP_OK;
    if (table == nullptr || query == nullptr) return BP_ERR_SHAPE;
    if (!aligned16({table, query})) return BP_ERR_SHAPE;
    if (!strides8({t_row_stride, t_sense_stride, q_query_stride, q_sense_stride})) return BP_ERR_SHAPE;
    for (const void *p4 : {(const void *)cand_index, (const void *)flat, (const void *)min_pair, (const void *)max_pair,
                           (const void *)min_all, (const void *)max_all, (const void *)per_sense})
        if (reinterpret_cast<uintptr_t>(p4) % 4) return BP_ERR_SHAPE;
    const bool any_pair = flat != nullptr || min_pair != nullptr || max_pair != nullptr || min_all != nullptr || max_all != nullptr;
    if (any_pair && o_query_stride < ncand) return BP_ERR_SHAPE;
    // rows of different (query, sense) pairs do not overlap
    if (per_sense != nullptr && (ps_sense_stride < ncand || (nq > 1 && ps_query_stride < nsenses * ps_sense_stride)))
        return BP_ERR_SHAPE;
    bp::SimilarityParams p{};
    p.table = table; p.query = query; p.cand_index = cand_index;
    p.flat = flat; p.min_pair = min_pair; p.max_pair = max_pair; p.min_all = min_all; p.max_all = max_all;
    p.per_sense = per_sense;
    p.t_rs = t_row_stride; p.t_gs = t_sense_stride; p.q_qs = q_query_stride; p.q_gs = q_sense_stride;
    p.o_qs = o_query_stride; p.ps_qs = ps_query_stride; p.ps_gs = ps_sense_stride; p.table_rows = table_rows;
    p.ncand = (int)ncand; p.groups = nsenses; p.d = d; p.nq = nq;
    p.logk = 0;
    while ((1 << p.logk) < nsenses) ++p.logk;
    return launch_status(bp::launch_sense_similarity(p, dtype, static_cast<hipStream_t>(stream)));
}

// ---- row scoring (bp_score_rows) ----

int bp_score_rows(const void *logits, const int64_t *targets, float *logprob, int32_t *rank, float *lse, int32_t *top1,
                  float *entropy, int64_t rows, int cols, int ntargets, int64_t row_stride, int64_t target_stride,
                  int64_t out_stride, int dtype, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16 && dtype != BP_DTYPE_F32) return BP_ERR_DTYPE;
    if (rows <= 0 || rows > 0x7fffffffLL || cols <= 0 || cols > 0x7fffffff - 16 || row_stride < cols) return BP_ERR_SHAPE;
    if (ntargets < 1 || ntargets > BP_SCORE_MAX_TARGETS || target_stride < ntargets) return BP_ERR_SHAPE;
    if (logits == nullptr || targets == nullptr) return BP_ERR_SHAPE;
    if (logprob == nullptr && rank == nullptr && lse == nullptr && top1 == nullptr && entropy == nullptr) return BP_ERR_SHAPE;
    if ((logprob != nullptr || rank != nullptr) && out_stride < ntargets) return BP_ERR_SHAPE;
    const uintptr_t elem = dtype == BP_DTYPE_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(logits) % elem || reinterpret_cast<uintptr_t>(targets) % 8) return BP_ERR_SHAPE;
    for (const void *p4 : {(const void *)logprob, (const void *)rank, (const void *)lse, (const void *)top1, (const void *)entropy})
        if (reinterpret_cast<uintptr_t>(p4) % 4) return BP_ERR_SHAPE;
    bp::ScoreParams p{};
    p.logits = logits; p.targets = targets; p.logprob = logprob; p.rank = rank; p.lse = lse; p.top1 = top1; p.entropy = entropy;
    p.rows = rows; p.row_stride = row_stride; p.target_stride = target_stride; p.out_stride = out_stride;
    p.cols = cols; p.ntargets = ntargets;
    return launch_status(bp::launch_score_rows(p, dtype, static_cast<hipStream_t>(stream)));
}

// ---- the record of a pick (bp_pick_report) ----

int bp_pick_report(const void *logits, const int64_t *tokens, const int32_t *counters, float *logprob, int32_t *rank,
                   float *entropy, int32_t *top_idx, float *top_logprob, int rows, int vocab, int64_t row_stride,
                   int64_t tokens_stride, int rec_cols, int64_t rec_stride, int n_top, int dtype, bp_stream_t stream) {
    if (dtype != BP_DTYPE_F16 && dtype != BP_DTYPE_BF16 && dtype != BP_DTYPE_F32) return BP_ERR_DTYPE;
    if (rows < 1 || vocab < 1 || vocab > 0x7fffffff - 16 || row_stride < vocab || tokens_stride < 1) return BP_ERR_SHAPE;
    if (rec_cols < 1 || rec_stride < rec_cols) return BP_ERR_SHAPE;
    if (n_top < 0 || n_top > BP_PICK_REPORT_MAX_TOP || n_top > vocab) return BP_ERR_SHAPE;
    if (logits == nullptr || tokens == nullptr || counters == nullptr) return BP_ERR_SHAPE;
    if (logprob == nullptr && rank == nullptr && entropy == nullptr && top_idx == nullptr && top_logprob == nullptr)
        return BP_ERR_SHAPE;
    if (n_top > 0 && top_idx == nullptr && top_logprob == nullptr) return BP_ERR_SHAPE;
    const uintptr_t elem = dtype == BP_DTYPE_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(logits) % elem || reinterpret_cast<uintptr_t>(tokens) % 8) return BP_ERR_SHAPE;
    for (const void *p4 : {(const void *)counters, (const void *)logprob, (const void *)rank, (const void *)entropy,
                           (const void *)top_idx, (const void *)top_logprob})
        if (reinterpret_cast<uintptr_t>(p4) % 4) return BP_ERR_SHAPE;
    bp::PickReportParams p{};
    p.logits = logits; p.tokens = tokens; p.counters = counters;
    p.logprob = logprob; p.rank = rank; p.entropy = entropy; p.top_idx = top_idx; p.top_logprob = top_logprob;
    p.row_stride = row_stride; p.tokens_stride = tokens_stride; p.rec_stride = rec_stride;
    p.rows = rows; p.vocab = vocab; p.rec_cols = rec_cols; p.n_top = n_top;
    return launch_status(bp::launch_pick_report(p, dtype, static_cast<hipStream_t>(stream)));
}

}  // extern "C"
