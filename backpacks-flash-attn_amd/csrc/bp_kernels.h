// Internal launch interface between the C ABI (bp_api.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/bp_hip.h"
#include "bp_common.h"

namespace bp {

// ---- launcher dispatch: a run-time value becomes a compile-time constant for a generic lambda --------------------------
// f receives BF16{} / F16{}, a std::integral_constant or a std::bool_constant; the constants convert to template
// arguments as they are (`kernel<decltype(et), kd, vec>`).  Only what a lambda body names is instantiated: a restriction
// of the instantiation set is an `if constexpr` in the body.
template <class F> hipError_t with_dtype(int dtype, F &&f) { return dtype == BP_DTYPE_BF16 ? f(BF16{}) : f(F16{}); }
// the kernels over rows of logits (vocab_row.h) also take fp32: f receives float{} then
template <class F> hipError_t with_row_dtype(int dtype, F &&f) { return dtype == BP_DTYPE_F32 ? f(float{}) : with_dtype(dtype, f); }

template <class F> hipError_t with_flag(bool b, F &&f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// 16-column steps of a head / sense width d <= 128: KD = ceil(d / 16), 8 for anything outside 1..7
template <int KD = 1, class F> hipError_t with_kd(int d, F &&f) {
    if constexpr (KD < 8)
        if ((d + 15) / 16 != KD) return with_kd<KD + 1>(d, f);
    return f(std::integral_constant<int, KD>{});
}
// 64-column V chunks of the trunk kernels (flash_fwd*.hip) for KD steps: 1, 1, 2, 2, 3, 3, 4, 4
constexpr int trunk_nv(int kd) { return (kd + 1) / 2; }

// the smallest N of the list with x <= N; `none` when x exceeds them all
template <int N, int... Ns, class F> hipError_t with_bound(int x, hipError_t none, F &&f) {
    if (x <= N) return f(std::integral_constant<int, N>{});
    if constexpr (sizeof...(Ns) > 0) return with_bound<Ns...>(x, none, f);
    else return none;
}

// workgroups of a persistent launch: one per CU of the current device (cached per thread; 256 when the query fails),
// fewer when there are fewer jobs
inline int persistent_grid(int njobs) {
    thread_local int cached_dev = -1, cus = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return njobs < 256 ? njobs : 256;
    if (dev != cached_dev) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        cached_dev = dev;
    }
    return njobs < cus ? njobs : cus;
}

// All strides are in ELEMENTS (16-bit elements for q/k/v/o/c, fp32 for lse).
struct FlashParams {
    const void *q, *k, *v;
    void *o;
    float *lse;
    const int *cu_q, *cu_k;   // NULL: fixed length, sequence b at rows [b*max_s, (b+1)*max_s)
    int64_t q_rs, q_hs, k_rs, k_hs, v_rs, v_hs, o_rs, o_hs;
    int64_t q_bs, k_bs, v_bs, o_bs;   // batch strides, used only when cu_q == NULL
    int64_t lse_stride;       // elements between consecutive (batch, head) rows of lse
    int b, h, d;
    int max_sq, max_sk;
    int n_qtiles;             // ceil(max_sq / 128)
    int causal;
    int pair;                 // flash_fwd_dma: one workgroup takes query tiles t and n-1-t (causal load balance)
    float scale_log2e;        // softmax_scale * log2(e)
    // dropout (training): see bp_philox.h.  drop_thr == 0: no dropout.
    const uint64_t *rng_state;   // device {seed, offset}
    uint32_t drop_thr;           // keep iff u16 < drop_thr  (round((1-p) * 65536))
    float drop_scale;            // 1 / (1 - p)
};

struct FlashBwdParams {
    const void *q, *k, *v, *dout, *out;
    const float *lse;         // (b, h, lse_stride) from the forward
    float *dsum;              // (b, h, lse_stride) workspace: D_i = sum_d dO_i[d] * O_i[d], written by the dQ kernel
    void *dq, *dk, *dv;
    const int *cu_q, *cu_k;   // NULL: fixed length
    int64_t q_rs, q_hs, k_rs, k_hs, v_rs, v_hs, do_rs, do_hs, o_rs, o_hs;
    int64_t dq_rs, dq_hs, dk_rs, dk_hs, dv_rs, dv_hs;
    int64_t lse_stride;
    int b, h, d, max_sq, max_sk, causal;
    float scale;
    const uint64_t *rng_state;   // dropout, as in FlashParams (must be the forward's state)
    uint32_t drop_thr;
    float drop_scale;
};

hipError_t launch_flash_bwd(const FlashBwdParams &p, int dtype, hipStream_t stream);

struct ProbsParams {
    const void *q, *k;
    const float *lse;
    void *p;
    int64_t q_bs, q_rs, q_hs, k_bs, k_rs, k_hs;
    int64_t lse_stride;
    int64_t p_bs, p_hs, p_rs;
    int b, h, d, sq, sk;
    int causal;
    int p_vec;                // 1: 8-byte stores into P are aligned
    int p_vec16;              // 1: 16-byte stores at multiples of 8 keys are aligned (full-line path)
    float scale_log2e;
    const uint64_t *rng_state;   // dropout: dropped entries are stored NEGATED (sign bit), see bp_attn_probs_dropout
    uint32_t drop_thr;
};

// job queues of the persistent sense-mix launches (mix_ring.h; sense_mix_dma.hip, sense_mix_bwd.hip): one ticket per XCD.
// 64 bytes, zeroed in front of every launch (arm_mix_queues)
struct MixQueues {
    unsigned int ticket[8];
    unsigned int pad[8];
};
hipError_t arm_mix_queues(MixQueues *&queues, hipStream_t stream);   // NULL -> a record of the library's ring
// a job is numbered group * kMixMaxTiles + tile: at most this many 256-row tiles per sequence (bp_api.hip, sense_route)
constexpr int kMixMaxTiles = 256;

struct MixParams {
    const void *q, *k;        // q_l[t] = q + b*qk_bs + t*qk_rs + l*qk_ss ; k likewise
    const void *c;            // content[b, s, l, :] = c + b*c_bs + s*c_rs + l*c_ss
    void *o;                  // out[b, t, :] = o + b*o_bs + t*o_rs
    const float *lse;         // (b, k, lse_stride) natural-log LSE of every (sense, query)
    union {
        const float *kw;      // optional key weights w[b, l, s] (fp32, unit stride along s): alpha[b,l,:,s] *= w
        // launch_sense_mix_varlen only (packed batches; there is no weighted packed form, so the two never meet): sample b
        // owns rows [cu[b], cu[b + 1]) of the operands; (b + 1) device ints, non-decreasing, every length in 0 .. s, not
        // validated.  It shares the key weights' slot because a field of its own moves the arguments that kernels take
        // BEHIND their MixParams (sense_lse_wide_dma_kernel's lse: other offsets in its text).
        const int32_t *cu;
    };
    int64_t kw_bs, kw_ss;
    const int32_t *row_index; // optional (bp_sense_mix_gather): content[b, s, l, :] = c + row_index[b*idx_bs + s]*c_rs + l*c_ss
    int64_t idx_bs;
    uint32_t last_table_row;  // table_rows - 1: indices are clamped to it (unsigned, so a negative index also lands there)
    int64_t qk_bs, qk_rs, qk_ss;
    int64_t c_bs, c_rs, c_ss;
    int64_t o_bs, o_rs;
    int64_t lse_stride;
    int b, s, nsenses, dk, dout;
    int n_qtiles;             // ceil(s / 256)
    int n_chunks;             // ceil(dout / 256)
    float scale_log2e;
    MixQueues *queues;        // caller's record (queue_ws) or NULL; armed by launch_sense_mix_dma
};

// Packed batches (bp_sense_mix_varlen / bp_sense_mix_gather_varlen; sense_mix_varlen.hip): MixParams with `cu` set.  The
// operands are (total, ...) tensors, s = max_seqlen (n_qtiles counts its tiles), the batch strides and idx_bs are not
// read, lse is (b, nsenses, lse_stride) as in the fixed form.
hipError_t launch_sense_mix_varlen(const MixParams &p, int dtype, hipStream_t stream);

// limits of the gathering sense mix: a job's row indices share the LDS with the ring as u16 (sense_mix_dma.hip)
constexpr int kMixGatherMaxKeys = 4096;
constexpr int64_t kMixGatherMaxRows = 65536;

// backward of the sense combination (sense_mix_bwd.hip)
struct MixBwdParams {
    const void *q, *k;        // as MixParams
    const void *dout;         // dout[b, t, :] = dout + b*do_bs + t*do_rs
    void *dc;                 // dC[b, s, l, :] = dc + b*c_bs + s*c_rs + l*c_ss
    const float *lse;         // (b, k, lse_stride)
    int64_t qk_bs, qk_rs, qk_ss;
    int64_t do_bs, do_rs;
    int64_t c_bs, c_rs, c_ss;
    int64_t lse_stride;
    int b, s, nsenses, dk, dout_cols;
    int n_ktiles;             // ceil(s / 256)
    int n_chunks;             // ceil(dout_cols / 256)
    float scale_log2e;
    MixQueues *queues;        // caller's record (queue_ws) or NULL; armed by launch_sense_mix_dc
};
hipError_t launch_sense_mix_dc(const MixBwdParams &p, int dtype, hipStream_t stream);

struct SenseGradParams {
    const void *q, *k;        // as MixParams
    const void *dpt;          // (b, N, 128) 16-bit: dP^T slab, row s*k + l, column = query t0 + j
    const float *lse;         // (b, k, lse_stride)
    float *dsum;              // (b, k, lse_stride): D, written by the dq kernel, read by the dk kernel
    void *dq;                 // dq_l[t] = dq + b*dq_bs + t*dq_rs + l*dq_ss   (16-bit)
    float *dk_acc;            // dk_l[s] += at dk_acc + b*dka_bs + s*dka_rs + l*dka_ss   (fp32)
    int64_t qk_bs, qk_rs, qk_ss;
    int64_t dpt_bs;
    int64_t dq_bs, dq_rs, dq_ss;
    int64_t dka_bs, dka_rs, dka_ss;
    int64_t lse_stride;
    int b, s, nsenses, dk;
    int t0;                   // first query of the slab (multiple of 128)
    float scale;
};
hipError_t launch_sense_dq_dk(const SenseGradParams &p, int dtype, hipStream_t stream);

struct SoftmaxBwdParams {
    const void *alpha;   // (n, s, s) 16-bit causal softmax output (zeros above the diagonal)
    void *dp;            // (n, s, s) 16-bit: gradient w.r.t. alpha in, gradient w.r.t. the scores out
    int64_t rows;        // n * s
    int s;
    float scale;
};
hipError_t launch_softmax_bwd_causal(const SoftmaxBwdParams &p, int dtype, hipStream_t stream);

struct XentParams {
    const void *logits;        // (rows, cols), row stride in elements, last stride 1
    const int64_t *labels;     // (rows)
    float *losses, *lse;       // (rows) fp32                                   [forward out / backward in: lse]
    const float *grad_losses;  // (rows) fp32                                   [backward]
    void *grad_logits;         // (rows, cols) logits' dtype, may alias logits   [backward]
    int64_t rows, row_stride, grad_row_stride;
    int cols, total_classes;
    float smoothing;
};

hipError_t launch_xentropy_fwd(const XentParams &p, int dtype, hipStream_t stream);
hipError_t launch_xentropy_bwd(const XentParams &p, int dtype, hipStream_t stream);

struct LnParams {
    const void *x0;           // (rows, cols) 16-bit, or fp32 when x0_f32 (then z is fp32 too)
    const void *x1;           // (rows, cols) residual in, 16-bit or fp32, may be NULL
    const void *gamma, *beta; // (cols) 16-bit or fp32
    void *z;                  // (rows, cols) in x0's dtype
    void *x_out;              // (rows, cols) residual out (x0 + x1), 16-bit or fp32, may be NULL
    int64_t rows;
    int cols;
    int x1_f32, xo_f32, w_f32;
    float eps;
    int x0_f32;
    uint8_t *dmask;              // optional (rows, cols) keep mask out (1 = kept), only written with dropout
    const uint64_t *rng_state;   // dropout on x0 (bp_philox.h); drop_thr == 0: none
    uint32_t drop_thr;
    float drop_scale;
    const void *rowscale;        // optional (rows) in x0's dtype: x0 row r is multiplied by rowscale[r] (DropPath)
    const void *colscale;        // optional (cols) in gamma's dtype: column c by colscale[c] (LayerScale)
    // launch_add_layer_norm_chain only (the inference forms; NULL / 0 otherwise)
    const void *x0b;             // optional (rows, cols) 16-bit second branch output: x = (x0 + x1) + x0b
    const int64_t *tok;          // (rows) token ids: x0 = wte[tok] (+ wpe[position]) instead of the x0 pointer
    const int64_t *pos;          // optional (pos_len) position ids; NULL: the position of row r is r % pos_len
    const void *wte, *wpe;       // (last_tok + 1, cols) / optional (last_pos + 1, cols) 16-bit tables
    uint32_t pos_len;            // row r takes position entry r % pos_len (rows for per-row ids, seqlen for shared ones)
    int64_t last_tok, last_pos;  // ids are clamped to [0, last] as unsigned values
};

hipError_t launch_add_layer_norm(const LnParams &p, int dtype, hipStream_t stream);
hipError_t launch_add_layer_norm_chain(const LnParams &p, int dtype, hipStream_t stream);

constexpr int kLnBwdMaxWg = 1024;   // row-parallel workgroups of the backward = rows of its partial-sum workspace
struct LnBwdParams {
    const void *dz;           // (rows, cols) 16-bit: gradient of the normalised output
    const void *dx_in;        // (rows, cols) residual dtype: gradient of the residual output (prenorm), may be NULL
    const void *x;            // (rows, cols) residual dtype: the summed stream x0 + x1 the forward normalised
    const void *gamma;        // (cols) 16-bit or fp32
    void *dx0;                // (rows, cols) 16-bit
    void *dx1;                // (rows, cols) residual dtype, may be NULL (same values as dx0)
    void *dgamma, *dbeta;     // (cols) gamma's dtype
    float *ws;                // (2, kLnBwdMaxWg, cols) fp32 partial sums; (3, ...) with a colscale
    int64_t rows;
    int cols, n_wg;
    int res_f32, w_f32;
    float eps;
    int x0_f32;                  // dz and dx0 are fp32 (the forward's x0 / z dtype)
    const uint64_t *rng_state;   // the forward's dropout state: dx0 = dropout-masked, rescaled dx
    uint32_t drop_thr;
    float drop_scale;
    const void *rowscale, *colscale;   // the forward's (optional)
    const void *x0;              // the forward's x0 (dz's dtype): needed for dcolscale only
    void *dcolscale;             // (cols) gamma's dtype, with colscale
};
hipError_t launch_add_layer_norm_bwd(const LnBwdParams &p, int dtype, hipStream_t stream);
// bias + tanh-GELU forward / backward and bias-gradient column sums (bias_gelu.hip)
constexpr int kBiasGeluMaxSlices = 1024;
struct BiasGeluParams {
    const void *x;       // fwd: (rows, cols) GEMM output;  bwd / column sum: the incoming gradient g
    const void *bias;    // fwd: (cols) 16-bit or NULL
    void *pre;           // fwd: optional (rows, cols) out = x + bias;  bwd: (rows, cols) in = saved pre-activation
    void *y;             // fwd: gelu out;  bwd: dpre out (may alias x)
    void *dbias;         // bwd: (cols) out, fp32 or 16-bit, may be NULL
    float *ws;           // bwd: (slices, cols) fp32 partial sums (required when dbias != NULL)
    int64_t rows;
    int cols;
    int dbias_f32;
};
hipError_t launch_bias_gelu_fwd(const BiasGeluParams &p, int dtype, hipStream_t stream);
hipError_t launch_bias_gelu_bwd(const BiasGeluParams &p, int dtype, bool gelu, hipStream_t stream);
int bias_gelu_bwd_slices(int64_t rows, int cols);
hipError_t launch_flash_fwd(const FlashParams &p, int dtype, hipStream_t stream);
// LDS-DMA ring version; needs 16-byte friendly shapes (vec)
hipError_t launch_flash_fwd_dma(const FlashParams &p, int dtype, hipStream_t stream);
hipError_t launch_attn_probs(const ProbsParams &p, int dtype, bool vec, hipStream_t stream);
hipError_t launch_sense_mix(const MixParams &p, int dtype, bool vec_qk, bool vec_c, hipStream_t stream);
// LDS-DMA ring version; needs 16-byte friendly shapes (vec_qk && vec_c)
hipError_t launch_sense_mix_dma(const MixParams &p, int dtype, hipStream_t stream);
// wide senses, 128 < d_k <= kWideMaxDk (sense_wide.hip): the reference's few-sense ablations (vecs-4: 160, vecs-1: 640)
constexpr int kWideMaxDk = 640;
// the LSE pre-pass and alpha take the mix operands without content (d_out = 0): `lse` is written, alpha reads p.lse
hipError_t launch_sense_lse_wide(const MixParams &p, float *lse, int dtype, bool vec, hipStream_t stream);
hipError_t launch_sense_alpha_wide(const MixParams &p, void *alpha, int dtype, bool vec, hipStream_t stream);
hipError_t launch_sense_mix_wide(const MixParams &p, int dtype, bool vec_qk, bool vec_c, hipStream_t stream);
// LDS-DMA ring versions for the reference's two few-sense configurations exactly (d_k = 160 / 640, 16-byte friendly
// operands, s % 32 == 0): sense_wide_dma.hip
bool sense_wide_dma_takes(int s, int dk, int dout, bool vec_qk, bool vec_c, bool weighted);
hipError_t launch_sense_mix_wide_dma(const MixParams &p, int dtype, hipStream_t stream);
hipError_t launch_sense_lse_wide_dma(const MixParams &p, float *lse, int dtype, hipStream_t stream);

// Single-query decode against a cache (decode_core.h): bp_flash_decode (groups = heads; value rows from the V half of the
// cache) and bp_sense_decode (groups = senses; value rows from a table through a row index).  Element strides.
struct DecodeParams {
    const void *q, *k_new, *v_new;
    void *k_cache, *v;                // v: V half of the KV cache (trunk) / the content table (senses)
    int64_t q_bs, q_gs, kn_bs, kn_gs, vn_bs, vn_gs;
    int64_t kc_bs, kc_rs, kc_gs;      // key of (b, j, g): k_cache + b*kc_bs + j*kc_rs + g*kc_gs
    int64_t vc_bs, vc_rs, vc_gs;      // trunk: value of (b, j, g); senses: table row r, sense g at r*vc_rs + g*vc_gs
    int32_t *row_index;               // senses: (b, max_seqlen) table row of every cached position, stride ri_bs
    int64_t ri_bs;
    const int32_t *new_row;           // senses: (b) table row of the new position
    int64_t table_rows;
    const int32_t *seqlens;           // (b) cached positions before the new one
    float *ws_acc, *ws_ml;            // (b, groups, nsplit, dv) and (b, groups, nsplit, 2) fp32 partials
    void *o;
    int64_t o_bs, o_gs;
    float *lse;                       // trunk only, optional: (b, lse_bs) natural-log LSE of every head's row
    int64_t lse_bs;
    int b, groups, dk, dv, max_seqlen, nsplit;
    float scale_log2e;
    // bp_sense_decode_weighted only (last, so the kernels without them keep their argument offsets): fp32 weight of
    // (b, g, j) at key_weight + b*kw_bs + g*kw_gs + j
    const float *key_weight;
    int64_t kw_bs, kw_gs;
};
int decode_nsplit(int batch, int groups, int max_seqlen);
hipError_t launch_flash_decode(const DecodeParams &p, int dtype, hipStream_t stream);
hipError_t launch_sense_decode(const DecodeParams &p, int dtype, hipStream_t stream);
// the senses' combine alone: second launch of the weighted decode, whose split kernels are a code object of their own
hipError_t launch_sense_decode_combine(const DecodeParams &p, int dtype, hipStream_t stream);
hipError_t launch_sense_decode_weighted(const DecodeParams &p, int dtype, hipStream_t stream);

// bp_sense_rows_dot (sense_rows_dot.hip): out[b, l, j] = table[row(b, j), l, :] . vec[b, :] for j = 0 .. seqlens[b]
struct RowsDotParams {
    const void *table, *vec;
    const int32_t *row_index, *new_row, *seqlens;
    float *out;
    int64_t t_rs, t_gs, ri_bs, v_bs, o_bs, o_gs, table_rows;
    int b, groups, dout, max_seqlen;
};
hipError_t launch_sense_rows_dot(const RowsDotParams &p, int dtype, hipStream_t stream);

// bp_pick_token (pick_token.hip): one token per row of logits -- argmax, or a draw after temperature / top-k / top-p
struct PickParams {
    const void *logits;          // (batch, vocab) 16-bit or fp32, element stride row_stride, last stride 1; only read
    int64_t *tokens;             // token of row b at tokens[b * tokens_stride]
    int64_t *sequences;          // optional: row b, column counters[b] receives the token when 0 <= column < seq_cols
    float *stats;                // optional (batch, 4): lowest kept z, log-sum-exp of the kept z, kept count, u
    const uint64_t *rng_state;   // device {seed, offset} (bp_philox.h); read when do_sample
    const int32_t *counters;     // optional (batch): Philox counter of every row = column of `sequences`; NULL: 0
    int64_t row_stride, tokens_stride, seq_stride;
    int batch, vocab, seq_cols;
    int do_sample, top_k;
    float inv_t, top_p;          // 1 / temperature
    // bp_pick_token_ctl only (pick_token_ctl.hip); the plain kernels never read past top_p
    int32_t *finished;           // optional (batch): a set flag turns the row's pick into `pad`; set when the pick is `eos`
    float theta, inv_theta;      // repetition penalty and its reciprocal
    int eos, pad, min_length;    // eos < 0: none; the EOS entry counts as -inf while counters[b] < min_length
    // bp_pick_token_lim only (pick_token_lim.hip); the plain and the controlled kernels never read past min_length
    const int32_t *suppress;     // n_suppress ids that count as -inf; ids outside [0, vocab) are ignored
    int n_suppress, ngram;       // ngram: no_repeat_ngram_size, 0 = off
    int penalty_begin;           // history positions at or behind it are counted
    int table_shift;             // 32 - log2(slots of the count table)
    float freq_pen, pres_pen;
    // bp_pick_token_lim_rows only (pick_token_rows.hip); no other kernel reads past pres_pen
    const int32_t *penalty_begins;   // optional (batch): replaces penalty_begin for row b; negative entries count as 0
    const int32_t *min_lengths;      // optional (batch): replaces min_length for row b; negative entries count as 0
    // bp_pick_token_phrases only (pick_token_phrases.hip); no other kernel reads past min_lengths.  Phrase j of a list is
    // ids[offsets[j] : offsets[j + 1]]; the kernel checks every offset against `total` and every length against kMaxPhraseLen
    const int32_t *ban_ids, *ban_offsets;     // n_ban phrases: the last id is banned behind the others
    const int32_t *stop_ids, *stop_offsets;   // n_stop phrases: generated text that ends with one finishes the row
    int32_t *ends, *reasons;                  // optional (batch) each: written when this call sets finished[b]
    int n_ban, ban_total, n_stop, stop_total;
};
constexpr int kMaxPhraseLen = 64;    // BP_PICK_MAX_PHRASE_LEN
constexpr int kMaxPhrases = 1024;    // BP_PICK_MAX_PHRASES: one phrase per thread of the pick's workgroup
hipError_t launch_pick_token(const PickParams &p, int dtype, hipStream_t stream);
hipError_t launch_pick_token_ctl(const PickParams &p, int dtype, hipStream_t stream);
hipError_t launch_pick_token_lim(const PickParams &p, int dtype, hipStream_t stream);
hipError_t launch_pick_token_rows(const PickParams &p, int dtype, hipStream_t stream);
hipError_t launch_pick_token_phrases(const PickParams &p, int dtype, hipStream_t stream);
// 32 - log2(slots), slots = the power of two >= 2 seq_cols (at least 2)
inline int lim_table_shift(int seq_cols) {
    int log2 = 1;
    while ((1 << log2) < 2 * seq_cols) ++log2;
    return 32 - log2;
}
size_t pick_lim_lds_bytes(const PickParams &p);   // static + dynamic LDS of a bp_pick_token_lim / _lim_rows launch
size_t pick_phrases_lds_bytes(const PickParams &p);   // of a bp_pick_token_phrases launch: the ban bitmap is on for a ban list too

// bp_beam_pick (beam_pick.hip): one beam-search step, rows r = g * beam_width + w
struct BeamPickParams {
    const void *logits;          // (groups * beam_width, vocab) 16-bit or fp32, element stride row_stride; only read
    float *beam_scores;          // (rows) read and written
    int32_t *finished;           // (rows) read and written; NULL only without an EOS id
    int32_t *parent;             // (rows) written: the global row every slot continues
    int64_t *tokens;             // token of slot r at tokens[r * tokens_stride]
    int64_t *sequences;          // optional: row r, column counters[r] receives the token when 0 <= column < seq_cols
    const int32_t *counters;     // optional (rows); NULL: 0
    float *ws;                   // bp_beam_pick_ws_floats(groups, beam_width) floats, 8-byte aligned
    int64_t row_stride, tokens_stride, seq_stride;
    int groups, beam_width, vocab, seq_cols;
    int eos, pad;                // eos < 0: none
};
hipError_t launch_beam_pick(const BeamPickParams &p, int dtype, hipStream_t stream);

// bp_beam_copy_rows (beam_copy.hip): rows r with parent[r] != r take positions [first_position, lengths[r]) of row parent[r]
constexpr int kBeamCopyMaxSets = 32;
struct BeamCopyParams {
    void *base[kBeamCopyMaxSets];
    int64_t row_stride[kBeamCopyMaxSets];   // bytes
    int64_t pos_bytes[kBeamCopyMaxSets];    // bytes per position, positions contiguous in a row
    const int32_t *parent, *lengths;        // (rows)
    int nsets, rows, first_position, max_positions;
};
hipError_t launch_beam_copy_rows(const BeamCopyParams &p, hipStream_t stream);

// bp_scatter_packed_rows (scatter_rows.hip): row cu_seqlens[b] + j of a packed source lands at [b][j] of a padded destination
constexpr int kScatterMaxSets = 32;
constexpr int kScatterPositions = 32;       // positions a workgroup owns
struct ScatterRowsParams {
    const void *src[kScatterMaxSets];
    void *dst[kScatterMaxSets];
    int64_t src_row_stride[kScatterMaxSets];                                   // bytes
    int64_t dst_batch_stride[kScatterMaxSets], dst_pos_stride[kScatterMaxSets];
    int64_t row_bytes[kScatterMaxSets];
    const int32_t *cu_seqlens;              // (batch + 1), on the device; not trusted
    int64_t total_rows;
    uint32_t wide;                          // bit i: set i moves 16-byte words (everything of it a multiple of 16)
    int nsets, batch, limit;                // limit = min(max_seqlen, max_positions)
};
hipError_t launch_scatter_packed_rows(const ScatterRowsParams &p, hipStream_t stream);

// bp_segment_sum_rows (segment_sum_rows.hip): acc[u] (= or +=) the fp32 sum of rows order[seg_begin[u]] .. order[seg_begin[u + 1] - 1]
constexpr int kSegLongRows = 32;            // segments of at least this many rows are cut into column slabs, 16 row lanes each
constexpr int kSegSlabCols = 128;           // columns of a slab
struct SegmentSumParams {
    const uint16_t *rows;                   // (n_rows, cols) 16-bit, element stride rows_stride
    const int32_t *order, *seg_begin;       // (n_rows), (n_segments + 1); on the device, not trusted
    float *acc;                             // (n_segments, cols), element stride acc_stride
    int64_t rows_stride, acc_stride;
    int n_rows, n_segments, cols, accumulate;
    int n_slabs;                            // set by the launcher
};
hipError_t launch_segment_sum_rows(SegmentSumParams p, int dtype, hipStream_t stream);

// bp_row_extremes (row_extremes.hip): the n largest / n smallest elements of every row, values and columns, in order
constexpr int kRowExtremesMaxN = BP_ROW_EXTREMES_MAX_N;
struct RowExtremesParams {
    const void *logits;          // (rows, cols) 16-bit or fp32, element stride row_stride, last stride 1; only read
    float *top_val, *bot_val;    // (rows, n) dense each; an end with both pointers NULL is skipped
    int32_t *top_idx, *bot_idx;
    int64_t row_stride;
    int rows, cols, n;
};
hipError_t launch_row_extremes(const RowExtremesParams &p, int dtype, hipStream_t stream);

// bp_sense_attribute (sense_attribute.hip): out[n, v, l, j] = p_j * table[row(b_n, j), l, :] . vec[n, v, :], p the causal
// softmax row of query n = (query_sample[n], query_pos[n]) over keys 0 .. i_n; zeros behind i_n
constexpr int kAttributeMaxVecs = BP_ATTRIBUTE_MAX_VECS;
struct AttributeParams {
    const void *q, *k, *table;   // q / k: the two halves of qk (B, S, 2, k, d_k); table (table_rows, k, d_out); 16-bit
    const int32_t *row_index, *query_sample, *query_pos;
    const float *vec;            // (nq, nvec, d_out)
    float *out, *probs, *ws;     // probs optional; ws: (nq, k, 2) = (m, Z)
    int64_t qk_bs, qk_rs, qk_ss, t_rs, t_gs, ri_bs, v_qs, v_vs, o_qs, o_vs, o_gs, p_qs, p_gs, table_rows;
    int b, s, groups, dk, dout, nq, nvec;
    float scale;
};
hipError_t launch_sense_attribute(const AttributeParams &p, int dtype, hipStream_t stream);

// bp_sense_similarity (sense_similarity.hip): the cosine measures of nq query words' sense vectors against ncand candidate
// words of the sense table -- cosines of matched senses, their min / max, min / max over all sense pairs, the flat cosine
constexpr int kSimilarityMaxQueryRows = BP_SIMILARITY_MAX_QUERY_ROWS;
struct SimilarityParams {
    const void *table, *query;   // (table_rows, k, d) and (nq, k, d) 16-bit
    const int32_t *cand_index;   // (ncand) or NULL: candidate c is row c
    float *flat, *min_pair, *max_pair, *min_all, *max_all;   // (nq, ncand), query stride o_qs; any may be NULL
    float *per_sense;            // (nq, k, ncand), strides ps_qs / ps_gs; may be NULL
    int64_t t_rs, t_gs, q_qs, q_gs, o_qs, ps_qs, ps_gs, table_rows;
    int ncand, groups, logk, d, nq;   // groups = k = 1 << logk
};
hipError_t launch_sense_similarity(const SimilarityParams &p, int dtype, hipStream_t stream);

// bp_score_rows (score_rows.hip): per row of logits, the log-sum-exp, the entropy, the greedy token, and the log-probability and
// rank of up to kScoreMaxTargets target columns, in one pass over the row
constexpr int kScoreMaxTargets = BP_SCORE_MAX_TARGETS;
struct ScoreParams {
    const void *logits;          // (rows, cols) 16-bit or fp32, element stride row_stride, last stride 1; only read
    const int64_t *targets;      // (rows, ntargets), element stride target_stride between rows
    float *logprob;              // (rows, ntargets), element stride out_stride between rows; any output may be NULL
    int32_t *rank;               // (rows, ntargets), the same stride
    float *lse, *entropy;        // (rows) dense
    int32_t *top1;               // (rows) dense
    int64_t rows, row_stride, target_stride, out_stride;
    int cols, ntargets;
};
hipError_t launch_score_rows(const ScoreParams &p, int dtype, hipStream_t stream);

// bp_pick_report (pick_report.hip): per row of logits and the token just picked from it, the token's log-probability and rank,
// the row's entropy and its n_top most likely tokens, written into column counters[b] of the record buffers
constexpr int kPickReportMaxTop = BP_PICK_REPORT_MAX_TOP;
struct PickReportParams {
    const void *logits;          // (rows, vocab) 16-bit or fp32, element stride row_stride, last stride 1; only read
    const int64_t *tokens;       // (rows), element stride tokens_stride
    const int32_t *counters;     // (rows): the column of the records; outside [0, rec_cols) nothing is written for the row
    float *logprob, *entropy;    // (rows, rec_cols), element stride rec_stride between rows; any record may be NULL
    int32_t *rank;               // the same
    int32_t *top_idx;            // (rows, rec_stride, n_top), dense in the last axis
    float *top_logprob;          // the same
    int64_t row_stride, tokens_stride, rec_stride;
    int rows, vocab, rec_cols, n_top;
};
hipError_t launch_pick_report(const PickReportParams &p, int dtype, hipStream_t stream);

}  // namespace bp
