/*
 * bp_hip.h -- C ABI of libbackpack_hip.so: the MI355X (gfx950) implementation of the
 * Backpack forward hot path.
 *
 * The reference (john-hewitt/backpacks-flash-attn) has no C ABI: its native boundary is the
 * pybind11 module `flash_attn_cuda` (csrc/flash_attn/fmha_api.cpp:776-782) taking at::Tensor,
 * and its Backpack-specific ops are eager ATen calls (training/src/models/backpack.py:107-122,313).
 * Every entry point below names the reference interface it replaces.  All of them
 *   - take raw DEVICE pointers, explicit sizes and int64 ELEMENT strides (no torch types),
 *   - allocate nothing and keep no caller-visible state (re-entrant; scratch is passed in by the caller).
 *     bp_sense_mix* / bp_sense_mix_dc launch persistent workgroups that pull jobs from ticket queues in a 64-byte
 *     record of device memory, `queue_ws` (BP_QUEUE_WS_BYTES, 16-byte aligned, contents undefined on entry: a
 *     memset node in front of the kernel zeroes it on the stream; it must belong to this launch alone until the
 *     launch has completed -- so a captured HIP graph owns the record it replays).  queue_ws == NULL takes the next
 *     record of a 64-entry ring owned by the library: fine for eager launches with fewer than 64 of them in flight;
 *     a NULL queue_ws on a stream that is being captured returns BP_ERR_QUEUE_WS (a replayed graph would share the
 *     library's record with every other launch),
 *   - enqueue on the given hipStream_t and return without synchronising,
 *   - return 0 on success or a negative BP_ERR_* (the Python layer raises RuntimeError, which
 *     is what TORCH_CHECK failures surface as in the reference: fmha_api.cpp:206-250).
 */
#ifndef BP_HIP_H
#define BP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BP_ABI_VERSION 11  /* 2: *_dropout entry points added; 3: bias/GELU + column-sum entry points added, the
                              persistent sense-mix launches take a caller-owned `queue_ws`; 4: bp_flash_bwd* take the
                              size of `dsum_ws` (bp_flash_bwd_ws_floats) and check it, queue_ws == NULL is refused
                              while the stream is capturing (BP_ERR_QUEUE_WS); 5: bp_dropout_add_layer_norm_scaled{,_bwd}
                              (rowscale / colscale of the reference's dropout_add_ln) added; 6: bp_sense_mix_gather added;
                              7: bp_sense_mix_gather clamps row_index to the table and takes tables of at most 65 536 rows;
                              8: bp_sense_lse / _alpha / _mix / _mix_weighted take sense widths d_k up to 640 (wide senses:
                              the reference's vecs-4 / vecs-1 ablations), bp_build_flags() added;
                              9: bp_sense_mix_gather takes the two few-sense widths d_k = 160 / 640 (seqlen % 32 == 0; any
                              number of table rows);
                              10: bp_flash_decode / bp_sense_decode (KV-cached single-token decoding) and their
                              *_ws_floats queries added;
                              11: bp_sense_decode_weighted (per-key weights on the decode step's probabilities) and
                              bp_sense_rows_dot (dot products of the cached positions' sense vectors with one vector)
                              added: KV-cached decoding of the intervened Backpacks;
                              (still 11, a purely additive entry point: bp_pick_token, token selection on the device --
                              argmax, temperature, top-k, top-p -- and BP_ERR_SAMPLING;
                              and another: bp_pick_token_ctl, the same pick with a repetition penalty, an EOS mask below
                              a minimal length and finished flags;
                              and two more: bp_beam_pick / bp_beam_copy_rows, a beam-search step and the cache reorder;
                              and one more: bp_pick_token_lim, the controlled pick with n-gram blocking, frequency /
                              presence penalties and a list of suppressed ids;
                              and one more: bp_row_extremes, the n largest / n smallest elements of every row of a
                              matrix, for the vocabulary projections of sense vectors;
                              and one more: bp_sense_attribute, the shares of every (position, sense) pair in a logit;
                              and one more: bp_add_layer_norm_chain, the inference-only forms of the fused add + LayerNorm
                              -- a second branch input, x0 rebuilt from the embedding tables, residual written in place;
                              and one more: bp_sense_similarity, the cosine measures of sense vectors (lexical similarity,
                              nearest words in sense space) in one pass over the sense table;
                              and one more: bp_score_rows, what an evaluation keeps of a row of logits -- log-probability and
                              rank of the gold token, log-sum-exp, greedy token, entropy -- in one pass over the row;
                              and three more: bp_sense_lse_varlen / bp_sense_mix_varlen / bp_sense_mix_gather_varlen, the sense
                              kernels on packed batches described by cu_seqlens;
                              and one more: bp_pick_report, the record of a decode step's pick -- log-probability and rank of
                              the token, entropy, the n most likely tokens -- in the record column the counter names);
                              and four more: bp_gemm_bf16 / bp_gemm_f16, a dense layer by a pinned hipBLASLt solution, with
                              bp_gemm_library / bp_gemm_heuristic, BP_ERR_GEMM and the BP_GEMM_* statuses;
                              and one more: bp_scatter_packed_rows, the rows of a packed batch into (batch, positions, ...)
                              buffers -- the prefill of the KV caches from packed prompts;
                              and one more: bp_pick_token_phrases, the row-limited pick with banned phrases and stop phrases
                              of several tokens, matched against the row's history on the device;
                              and one more: bp_segment_sum_rows, fp32 sums of 16-bit rows over the segments of a sorted index --
                              the gradient of the rows of a sense table that several positions read) */

/* element type of q/k/v/out/content tensors */
#define BP_DTYPE_F16 0
#define BP_DTYPE_BF16 1
#define BP_DTYPE_F32 2   /* accepted by the cross-entropy entry points and bp_pick_token only */

#define BP_OK 0
#define BP_ERR_DTYPE -1       /* dtype is not BP_DTYPE_F16 / BP_DTYPE_BF16         (fmha_api.cpp:215-219) */
#define BP_ERR_HEAD_DIM -2    /* head_dim < 1 or > 128 (sense width d_k > 640)      (fmha_api.cpp:245)     */
#define BP_ERR_SHAPE -3       /* batch/nheads/seqlen <= 0, or a required pointer is NULL (fmha_api.cpp:244-252) */
#define BP_ERR_SCALE -4       /* softmax_scale is not finite or not > 0                                     */
#define BP_ERR_LAUNCH -5      /* hipLaunchKernel failed (FMHA_CHECK_CUDA, src/fmha_utils.h:39)              */
#define BP_ERR_DOUT -6        /* sense mix: d_out < 1                                                       */
#define BP_ERR_DROPOUT -7     /* p_dropout outside [0,1), rng_state NULL with p > 0, or a shape the dropout path lacks */
#define BP_ERR_QUEUE_WS -8    /* persistent launch with queue_ws == NULL on a stream that is being captured            */
#define BP_ERR_WORKSPACE -9   /* a caller-provided workspace is smaller than the entry point's *_ws_floats() query     */
#define BP_ERR_SAMPLING -10   /* bp_pick_token: top_p outside (0, 1], or do_sample without an rng_state; bp_pick_token_ctl:
                                 also a repetition_penalty not finite and > 0 or without sequences, an EOS id without flags;
                                 bp_pick_token_lim: also a non-finite frequency / presence penalty, n-gram blocking or a
                                 penalty without sequences, n_suppress > 0 with a NULL or misaligned list;
                                 bp_pick_token_phrases: also a phrase list with a NULL array or without sequences, stop
                                 phrases without flags */
#define BP_ERR_GEMM -11       /* bp_gemm_*: a call into hipBLASLt or the HIP runtime failed                          */

/* bounds of bp_pick_token_lim (BP_ERR_SHAPE beyond them) */
#define BP_PICK_MAX_NGRAM 64                  /* no_repeat_ngram_size */
#define BP_PICK_MAX_LIMITED_VOCAB (1 << 19)   /* vocab with any of its controls on: 19 id bits of a count entry, 64 KB a bitmap */
#define BP_PICK_MAX_COUNTED_COLS 8191         /* seq_cols under a frequency / presence penalty: 13 count bits of an entry */
#define BP_PICK_MAX_LDS_BYTES (160 * 1024)    /* static + dynamic LDS of one launch: the LDS of a CU */
/* bounds of bp_pick_token_phrases */
#define BP_PICK_MAX_PHRASE_LEN 64             /* ids of one phrase (= BP_PICK_MAX_NGRAM); longer ones are ignored on the device */
#define BP_PICK_MAX_PHRASES 1024              /* phrases of one list: one per thread of the pick's workgroup */

#define BP_ROW_EXTREMES_MAX_N 64              /* bp_row_extremes: elements kept per end of a row */

#define BP_ATTRIBUTE_MAX_VECS 4                /* bp_sense_attribute: fp32 vectors per query */

#define BP_SIMILARITY_MAX_QUERY_ROWS 64        /* bp_sense_similarity: nq * nsenses, the query rows of one call */

#define BP_SCORE_MAX_TARGETS 8                 /* bp_score_rows: target columns per row */
#define BP_PICK_REPORT_MAX_TOP 16              /* bp_pick_report: most likely tokens recorded per pick */

#define BP_QUEUE_WS_BYTES 64  /* `queue_ws` of the persistent sense-mix launches */

typedef void *bp_stream_t; /* a hipStream_t */

/* Human-readable text for a BP_ERR_* code (static storage). */
const char *bp_strerror(int code);
int bp_abi_version(void);
/* 0 for a product build.  Bit 0: -DBP_FWD_WHATIF, bit 1: -DBP_BWD_WHATIF (timing builds that delete work on purpose:
 * results are garbage); no other bit is defined.  A binding should refuse to load a library with bit 0 or 1 set as its
 * default one. */
int bp_build_flags(void);

/*
 * bp_flash_fwd -- fused attention forward  O = softmax(scale * Q K^T [+ causal mask]) V  and the
 * row log-sum-exp.  Replaces flash_attn_cuda.fwd / mha_fwd (csrc/flash_attn/fmha_api.cpp:189-325),
 * no-dropout path; called by _flash_attn_forward (flash_attn/flash_attn_interface.py:13-28).
 *
 *   q            (total_q, nheads, head_dim) 16-bit, last stride 1; row/head strides free
 *   k, v         (total_k, nheads, head_dim) likewise.  v == NULL and out == NULL: LSE only.
 *   out          (total_q, nheads, head_dim), caller-allocated, written in place
 *   softmax_lse  (batch, nheads, lse_stride) fp32, natural log; -inf for a row with no key;
 *                entries >= that sequence's length are left untouched (fmha_api.cpp:276)
 *   cu_seqlens_* int32 (batch+1) device arrays of row offsets; NULL means fixed length:
 *                sequence b occupies rows [b*max_seqlen, (b+1)*max_seqlen)
 *   is_causal    mask is top-left aligned: key j visible to query i iff j <= i
 *                (csrc/flash_attn/src/fmha/mask.h:57-70)
 * Any head_dim in [1,128] is accepted; the 16-byte vector path needs head_dim % 8 == 0 with
 * 16-byte aligned rows (the reference's only mode), other shapes take an element-wise loader.
 */
int bp_flash_fwd(const void *q, const void *k, const void *v, void *out, float *softmax_lse,
                 const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k,
                 int batch, int nheads, int head_dim, int max_seqlen_q, int max_seqlen_k,
                 int64_t q_row_stride, int64_t q_head_stride,
                 int64_t k_row_stride, int64_t k_head_stride,
                 int64_t v_row_stride, int64_t v_head_stride,
                 int64_t o_row_stride, int64_t o_head_stride,
                 int64_t lse_stride, float softmax_scale, int is_causal, int dtype,
                 bp_stream_t stream);

/*
 * bp_flash_fwd_dropout -- bp_flash_fwd with in-kernel attention dropout (training): replaces the p_dropout > 0
 * path of flash_attn_cuda.fwd (csrc/flash_attn/fmha_api.cpp:199,306-320; kernel
 * src/fmha_fprop_kernel_1xN.h:494-506).  O = (dropout(P) / (1 - p)) V; the row log-sum-exp is that of the
 * UNdropped probabilities, as upstream.
 *   p_dropout  in [0, 1); 0 = identical to bp_flash_fwd (rng_state may then be NULL)
 *   rng_state  DEVICE pointer to two uint64 {seed, offset} (the role of the at::Generator's philox state,
 *              fmha_api.cpp:314-320).  Read by the kernel, never written; hand the SAME two words to
 *              bp_flash_bwd_dropout / bp_attn_probs_dropout to regenerate the same mask.  The mask is a pure
 *              function of (seed, offset, batch*nheads index, query index, key index): Philox2x32-10 keyed per
 *              (batch, head), one call per run of 4 keys, 16-bit uniforms against round((1-p) * 65536)
 *              (csrc/bp_philox.h; tests/philox_ref.py restates it on the host).
 * Dropout needs the 16-byte vector path (head_dim % 8 == 0, aligned rows); BP_ERR_DROPOUT otherwise.
 */
int bp_flash_fwd_dropout(const void *q, const void *k, const void *v, void *out, float *softmax_lse,
                         const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k,
                         int batch, int nheads, int head_dim, int max_seqlen_q, int max_seqlen_k,
                         int64_t q_row_stride, int64_t q_head_stride,
                         int64_t k_row_stride, int64_t k_head_stride,
                         int64_t v_row_stride, int64_t v_head_stride,
                         int64_t o_row_stride, int64_t o_head_stride,
                         int64_t lse_stride, float softmax_scale, int is_causal, int dtype,
                         float p_dropout, const uint64_t *rng_state, bp_stream_t stream);

/*
 * bp_attn_probs -- materialise normalised attention probabilities
 *   P[b,h,i,j] = exp(scale * q_i.k_j - lse[b,h,i])  for visible (i,j), exactly 0 elsewhere.
 * Serves `return_attn_probs=True` of the flash interface (flash_attn_interface.py:242-267; the
 * reference returns S_dmask from the same launch, fmha_api.cpp:279,322-324) and is the second pass
 * of bp_sense_alpha.  Fixed-length batches only.
 *   probs (batch, nheads, seqlen_q, seqlen_k) 16-bit, strides p_batch/p_head/p_row, last stride 1.
 */
int bp_attn_probs(const void *q, const void *k, const float *softmax_lse, void *probs,
                  int batch, int nheads, int head_dim, int seqlen_q, int seqlen_k,
                  int64_t q_batch_stride, int64_t q_row_stride, int64_t q_head_stride,
                  int64_t k_batch_stride, int64_t k_row_stride, int64_t k_head_stride,
                  int64_t lse_stride,
                  int64_t p_batch_stride, int64_t p_head_stride, int64_t p_row_stride,
                  float softmax_scale, int is_causal, int dtype, bp_stream_t stream);

/*
 * bp_attn_probs_dropout -- bp_attn_probs that also reports the dropout mask of bp_flash_fwd_dropout called with
 * the same (p_dropout, rng_state): a DROPPED entry is stored with its sign bit set (-P, or -0.0), a kept one
 * as +P.  Same encoding idea as the reference's S_dmask (fmha_api.cpp:279; tests/test_flash_attn.py:181-236
 * decode it with `S >= 0`); here P is already normalised, so decode with the sign BIT, not with `< 0`.
 */
int bp_attn_probs_dropout(const void *q, const void *k, const float *softmax_lse, void *probs,
                          int batch, int nheads, int head_dim, int seqlen_q, int seqlen_k,
                          int64_t q_batch_stride, int64_t q_row_stride, int64_t q_head_stride,
                          int64_t k_batch_stride, int64_t k_row_stride, int64_t k_head_stride,
                          int64_t lse_stride,
                          int64_t p_batch_stride, int64_t p_head_stride, int64_t p_row_stride,
                          float softmax_scale, int is_causal, int dtype,
                          float p_dropout, const uint64_t *rng_state, bp_stream_t stream);

/*
 * bp_sense_lse -- log-sum-exp of every (sense, query) row of the causal sense attention:
 *   lse[b,l,t] = log sum_{s<=t} exp(scale * q_l[t].k_l[s])
 * First pass of bp_sense_alpha / bp_sense_mix, exported so callers can share one LSE between them
 * (and time the passes separately).  The reference computes this inside torch.softmax
 * (training/src/models/backpack.py:122).
 *   lse (batch, nsenses, roundup(seqlen,16)) fp32, natural log.
 * Sense widths (this entry point, bp_sense_alpha, bp_sense_mix, bp_sense_mix_weighted): 1 <= d_k <= 640.  Up to 128 the
 * attention-class kernels run (LDS-DMA path for 16-byte friendly layouts); 129 ... 640 -- the reference's few-sense
 * ablations, training/configs/experiment/owt/backpack-mini-flash-vecs-4.yaml (d_k = 160) and ...-vecs-1.yaml (640) --
 * the wide kernels of csrc/sense_wide.hip (any alignment; d_k % 8 == 0 with 16-byte aligned rows takes 16-byte loads).
 * At d_k = 160 / 640 exactly, on 16-byte friendly operands with seqlen % 32 == 0, the LDS-DMA ring kernels of
 * csrc/sense_wide_dma.hip run instead (bp_sense_lse, bp_sense_mix; bp_sense_mix_gather takes only these two widths beyond 128).
 * The backward entry points stay at d_k <= 128.
 */
int bp_sense_lse(const void *qk, float *lse, int batch, int seqlen, int nsenses, int d_k,
                 int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride,
                 int64_t qk_sense_stride, float softmax_scale, int dtype, bp_stream_t stream);

/*
 * bp_sense_alpha -- Backpack contextualisation weights
 *   alpha[b,l,t,s] = softmax_s( q_l[t].k_l[s] * scale ) over s <= t, 0 for s > t.
 * Replaces the eager body of ContextSelfAttn.forward after its Wqkv projection
 * (training/src/models/backpack.py:112-122).
 *   qk     (batch, seqlen, 2, nsenses, d_k) 16-bit: the Wqkv output viewed as in backpack.py:111;
 *          element strides qk_batch/qk_row/qk_two/qk_sense, last stride 1
 *   alpha  (batch, nsenses, seqlen, seqlen) 16-bit contiguous, caller-allocated
 *   lse_ws fp32 scratch, batch * nsenses * roundup(seqlen,16) elements
 *   lse_ready  0: compute the LSE into lse_ws first;  1: lse_ws already holds bp_sense_lse's result
 */
int bp_sense_alpha(const void *qk, void *alpha, float *lse_ws, int lse_ready,
                   int batch, int seqlen, int nsenses, int d_k,
                   int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride,
                   int64_t qk_sense_stride, float softmax_scale, int dtype, bp_stream_t stream);

/*
 * bp_sense_mix -- fused sense-weighted combination, alpha never materialised:
 *   out[b,t,:] = sum_l sum_{s<=t} alpha[b,l,t,s] * content[b,s,l,:]
 * Replaces `torch.sum(contextualization @ content, dim=1)` together with the softmax that
 * produced `contextualization` (training/src/models/backpack.py:305,313).
 *   qk       as in bp_sense_alpha
 *   content  (batch, seqlen, nsenses, d_out) 16-bit -- the (B,S,k*d) output of the content
 *            model's final MLP before its reshape/transpose (backpack.py:274-276); element strides
 *            c_batch/c_row/c_sense, last stride 1.  d_out is free (vocab-sized content works).
 *   out      (batch, seqlen, d_out) 16-bit, strides o_batch/o_row
 *   lse_ws   fp32 scratch, batch * nsenses * roundup(seqlen,16) elements
 *   lse_ready  as in bp_sense_alpha
 *   queue_ws   BP_QUEUE_WS_BYTES of device memory for the persistent launch, or NULL (see the top of this file)
 */
int bp_sense_mix(const void *qk, const void *content, void *out, float *lse_ws, int lse_ready,
                 int batch, int seqlen, int nsenses, int d_k, int d_out,
                 int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride,
                 int64_t qk_sense_stride,
                 int64_t c_batch_stride, int64_t c_row_stride, int64_t c_sense_stride,
                 int64_t o_batch_stride, int64_t o_row_stride,
                 float softmax_scale, int dtype, void *queue_ws, bp_stream_t stream);

/*
 * bp_sense_mix_weighted -- bp_sense_mix with the intervention hook fused in:
 *   out[b,t,:] = sum_l sum_{s<=t} alpha[b,l,t,s] * key_weight[b,l,s] * content[b,s,l,:]
 * i.e. column s of sense l's contextualisation (equivalently: row s of that sense's content) is
 * scaled before the contraction.  Covers, without materialising alpha or a re-weighted copy of the
 * content, the reference's control experiments:
 *   - `contextualization[0, vector_index, :, index] *= percent` then `sum(contextualization @ content)`
 *     (training/src/test_genderbias.py:71-78),
 *   - `content * content_weights.transpose(1,2).unsqueeze(3)` then the same contraction
 *     (training/src/models/intervened_models.py:97-101).
 *   key_weight  (batch, nsenses, seqlen) fp32, unit stride along seqlen, element strides
 *               kw_batch/kw_sense; NULL = no weighting (then identical to bp_sense_mix)
 * All other arguments as bp_sense_mix.
 */
int bp_sense_mix_weighted(const void *qk, const void *content, const float *key_weight, void *out,
                          float *lse_ws, int lse_ready,
                          int batch, int seqlen, int nsenses, int d_k, int d_out,
                          int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride,
                          int64_t qk_sense_stride,
                          int64_t c_batch_stride, int64_t c_row_stride, int64_t c_sense_stride,
                          int64_t kw_batch_stride, int64_t kw_sense_stride,
                          int64_t o_batch_stride, int64_t o_row_stride,
                          float softmax_scale, int dtype, void *queue_ws, bp_stream_t stream);

/*
 * bp_sense_mix_gather -- bp_sense_mix with the content rows taken from a TABLE through a row index:
 *   out[b,t,:] = sum_l sum_{s<=t} alpha[b,l,t,s] * table[row_index[b,s], l, :]
 * The sense vectors C_l(x_s) of the reference depend on the token x_s alone (training/src/models/backpack.py:251-276: word
 * embedding without positions, an Identity mixer, per-token MLPs), so inference can run the content network once per
 * DISTINCT token of a batch (table = its output for the sorted distinct ids, row_index = torch.unique's inverse) and never
 * materialise the (batch, seqlen, nsenses * d_out) content tensor the reference builds (:276, :313).
 *   table      (table_rows, nsenses, d_out), element strides t_row_stride / t_sense_stride, last dim contiguous
 *   row_index  (batch, seqlen) int32, unit stride along seqlen, element stride idx_batch_stride; 0 <= value < table_rows.
 *              NOT validated: the kernel clamps every index as an unsigned value to table_rows - 1, so a negative or too
 *              large index silently reads the table's LAST row (never memory outside the table); callers that need an
 *              error for bad ids check them before the call (the reference's nn.Embedding asserts on the device)
 * Restrictions (BP_ERR_SHAPE otherwise; callers gather the rows themselves and call bp_sense_mix): the 16-byte vector
 * path (d_k % 8 == 0, d_out % 8 == 0, aligned bases, strides multiples of 8), seqlen <= 4096 and table_rows <= 65536 (a
 * job's row indices are kept in 8 KB of LDS as u16; ABI 6 took any row count at seqlen <= 4096 / 2048), and
 * table_rows * t_row_stride * 2 bytes < 4 GiB (row offsets are 32-bit in the DMA instruction).  Senses wider than 128:
 * d_k = 160 or 640 with seqlen % 32 == 0 only (ABI 9; row indices are kept as u32, any table_rows); BP_ERR_HEAD_DIM otherwise.
 * All other arguments as bp_sense_mix.
 */
int bp_sense_mix_gather(const void *qk, const void *table, const int32_t *row_index, void *out,
                        float *lse_ws, int lse_ready,
                        int batch, int seqlen, int nsenses, int d_k, int d_out, int64_t table_rows,
                        int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride,
                        int64_t qk_sense_stride,
                        int64_t t_row_stride, int64_t t_sense_stride, int64_t idx_batch_stride,
                        int64_t o_batch_stride, int64_t o_row_stride,
                        float softmax_scale, int dtype, void *queue_ws, bp_stream_t stream);

/*
 * bp_sense_lse_varlen, bp_sense_mix_varlen, bp_sense_mix_gather_varlen -- bp_sense_lse, bp_sense_mix and bp_sense_mix_gather on
 * PACKED batches (added within ABI 11: additive).  The sequences of a batch lie behind one another without padding, as in
 * the ragged calls of bp_flash_fwd: sample b owns rows [cu_seqlens[b], cu_seqlens[b + 1]) of every (total, ...) operand, and
 * attends causally within them.  A sample's output rows carry the bits bp_sense_mix returns for that sample alone.
 *   qk          (total, 2, nsenses, d_k) 16-bit, element strides qk_row/qk_two/qk_sense, last stride 1
 *   content     (total, nsenses, d_out), strides c_row/c_sense;  table / row_index (total) int32 as in bp_sense_mix_gather
 *   out         (total, d_out), stride o_row
 *   lse, lse_ws (batch, nsenses, roundup(max_seqlen,16)) fp32 -- the layout of the trunk's ragged calls; entries at or
 *               behind a sample's length are not written
 *   cu_seqlens  batch + 1 device ints, non-decreasing, cu_seqlens[0] >= 0, every length in 0 .. max_seqlen (a zero-length
 *               sample is legal and owns no rows).  NOT validated -- the host never reads the array (the contract of
 *               bp_flash_fwd's arrays): a length beyond max_seqlen loses its last rows, a decreasing array reads and
 *               writes rows of other samples.  NULL is BP_ERR_SHAPE.
 *   max_seqlen  takes the place of seqlen: it sizes the launch and the lse rows, and may exceed the longest length
 *   lse_ready, queue_ws (required on a capturing stream: BP_ERR_QUEUE_WS) and the error codes as in the fixed-length forms
 * There are no batch strides, and no idx_batch_stride.
 * Restrictions: narrow senses on the 16-byte vector path only, i.e. what bp_sense_mix_gather states -- d_k % 8 == 0 and
 * d_k <= 128 (BP_ERR_HEAD_DIM otherwise), d_out % 8 == 0 (BP_ERR_DOUT), aligned bases and strides that are multiples of 8,
 * max_seqlen <= 65536 (BP_ERR_SHAPE); the gathering form max_seqlen <= 4096, table_rows <= 65536 and a table below 4 GiB.
 * No key-weighted, wide or element-wise-loader form and no backward exist: callers pad such batches.
 */
int bp_sense_lse_varlen(const void *qk, float *lse, const int32_t *cu_seqlens, int batch, int max_seqlen, int nsenses,
                        int d_k, int64_t qk_row_stride, int64_t qk_two_stride, int64_t qk_sense_stride,
                        float softmax_scale, int dtype, bp_stream_t stream);
int bp_sense_mix_varlen(const void *qk, const void *content, void *out, float *lse_ws, int lse_ready,
                        const int32_t *cu_seqlens, int batch, int max_seqlen, int nsenses, int d_k, int d_out,
                        int64_t qk_row_stride, int64_t qk_two_stride, int64_t qk_sense_stride,
                        int64_t c_row_stride, int64_t c_sense_stride, int64_t o_row_stride,
                        float softmax_scale, int dtype, void *queue_ws, bp_stream_t stream);
int bp_sense_mix_gather_varlen(const void *qk, const void *table, const int32_t *row_index, void *out,
                               float *lse_ws, int lse_ready,
                               const int32_t *cu_seqlens, int batch, int max_seqlen, int nsenses, int d_k, int d_out,
                               int64_t table_rows,
                               int64_t qk_row_stride, int64_t qk_two_stride, int64_t qk_sense_stride,
                               int64_t t_row_stride, int64_t t_sense_stride, int64_t o_row_stride,
                               float softmax_scale, int dtype, void *queue_ws, bp_stream_t stream);

/*
 * bp_sense_mix_dc -- backward of bp_sense_mix with respect to the content:
 *   dcontent[b,s,l,:] = sum_{t>=s} alpha[b,l,t,s] * dout[b,t,:]
 * alpha is recomputed from qk and the saved log-sum-exp; no (batch, nsenses, seqlen, seqlen) tensor exists.  The
 * reference leaves this product to autograd through `torch.sum(contextualization @ content, dim=1)`
 * (training/src/models/backpack.py:313).
 *   qk        as in bp_sense_alpha, d_k % 8 == 0 (pad the projection, see ContextSelfAttn.project)
 *   dout      (batch, seqlen, d_out) 16-bit, strides do_batch/do_row, last stride 1, d_out % 8 == 0
 *   lse       (batch, nsenses, roundup(seqlen,16)) fp32: bp_sense_lse's result for this qk
 *   dcontent  (batch, seqlen, nsenses, d_out) 16-bit, strides c_batch/c_row/c_sense (the content's own layout)
 */
int bp_sense_mix_dc(const void *qk, const void *dout, const float *lse, void *dcontent,
                    int batch, int seqlen, int nsenses, int d_k, int d_out,
                    int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride, int64_t qk_sense_stride,
                    int64_t do_batch_stride, int64_t do_row_stride,
                    int64_t c_batch_stride, int64_t c_row_stride, int64_t c_sense_stride,
                    float softmax_scale, int dtype, void *queue_ws, bp_stream_t stream);

/*
 * bp_sense_dq_dk -- backward of the sense weights with respect to qk, for ONE slab of 128 queries [t0, t0 + 128):
 *   D_l[t]  = sum_s alpha_l[t,s] dP_l[t,s]        dS_l[t,s] = alpha_l[t,s] (dP_l[t,s] - D_l[t])
 *   dq_l[t] = scale sum_s dS_l[t,s] k_l[s]   -> written to dqk[b, t, 0, l, :]   (rows of the slab)
 *   dk_l[s] += scale sum_{t in slab} dS_l[t,s] q_l[t]   -> ADDED to dk_acc[b, s, l, :] (fp32; zero it before the
 *              first slab, run the slabs one after the other on one stream: the sum is then deterministic)
 * where dP_l[t,s] = dout[b,t,:] . content[b,s,l,:] comes precomputed, TRANSPOSED, from the caller:
 *   dpt  (batch, N, 128) 16-bit, row index s * nsenses + l, column = query t0 + j, N = min(seqlen, t0 + 128) *
 *        nsenses: the plain GEMM  content.view(batch, seqlen*nsenses, d)[:, :N] @ dout[:, t0:t0+128].T  (columns of
 *        queries past the sequence: anything finite).  A (B, S*k, 128) buffer, 1/(S/128) of the alpha-sized ones.
 *   dsum_ws  (batch, nsenses, roundup(seqlen,16)) fp32 scratch (D of the slab's rows is put there)
 *   dqk      16-bit, laid out like qk (strides dqk_batch/dqk_row/dqk_sense, the q half at offset 0)
 * Replaces what autograd does for ContextSelfAttn.forward (training/src/models/backpack.py:116-122).
 */
int bp_sense_dq_dk(const void *qk, const void *dpt, const float *lse, float *dsum_ws, void *dqk, float *dk_acc,
                   int batch, int seqlen, int nsenses, int d_k, int t0,
                   int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride, int64_t qk_sense_stride,
                   int64_t dpt_batch_stride,
                   int64_t dqk_batch_stride, int64_t dqk_row_stride, int64_t dqk_sense_stride,
                   int64_t dka_batch_stride, int64_t dka_row_stride, int64_t dka_sense_stride,
                   float softmax_scale, int dtype, bp_stream_t stream);

/*
 * bp_flash_bwd -- attention backward: dq, dk, dv from q, k, v, dout and the forward's out and softmax_lse.
 * Replaces flash_attn_cuda.bwd / mha_bwd (csrc/flash_attn/fmha_api.cpp:337-504) called by
 * _flash_attn_backward (flash_attn/flash_attn_interface.py:31-47), no-dropout path.  P is recomputed
 * from the LSE as upstream; the result is deterministic (no atomics).
 *   q, dout, out, dq  (total_q, nheads, head_dim); k, v, dk, dv (total_k, nheads, head_dim): 16-bit, last
 *                stride 1, 16-byte aligned rows, head_dim % 8 == 0 and <= 128
 *   softmax_lse  (batch, nheads, lse_stride) fp32
 *   dsum_ws      (batch, nheads, 2, lse_stride) fp32 workspace, contents undefined on entry: the kernels put the row
 *                statistics there, -D[b,h,i] = -sum_d dout_i[d] * out_i[d] (upstream's dsoftmax_sum,
 *                fmha_api.cpp:421) and -softmax_lse[b,h,i] / softmax_scale
 *   dsum_ws_floats  number of floats `dsum_ws` holds; must be >= bp_flash_bwd_ws_floats(batch, nheads, lse_stride)
 *                (BP_ERR_WORKSPACE otherwise: the workspace doubled between ABI 2 and 3, so its size is now an
 *                argument instead of a sentence in this comment)
 *   cu_seqlens_*       as in bp_flash_fwd (NULL = fixed length)
 */
int64_t bp_flash_bwd_ws_floats(int batch, int nheads, int64_t lse_stride);
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
                 bp_stream_t stream);

/*
 * bp_flash_bwd_dropout -- bp_flash_bwd for a forward that ran bp_flash_fwd_dropout: the p_dropout > 0 path of
 * flash_attn_cuda.bwd (fmha_api.cpp:337-504), which upstream feeds with the generator state saved by the
 * forward (flash_attn_interface.py:53-68: `rng_state`).  `out` must be the dropped-out forward output and
 * (p_dropout, rng_state) the forward's; the kernels regenerate the mask.
 */
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
                         float p_dropout, const uint64_t *rng_state, bp_stream_t stream);

/*
 * bp_add_layer_norm -- fused residual add + LayerNorm forward (eval path):
 *   x = x0 + x1 ;  z = (x - mean) * rsqrt(var + eps) * gamma + beta     (fp32 math)
 * Replaces dropout_layer_norm.dropout_add_ln_fwd with dropout_p = 0 and no rowscale / colscale /
 * subset (reference csrc/layer_norm/ln_api.cpp:83-254, called from
 * flash_attn/ops/layer_norm.py:9-25 by Block.forward, flash_attn/modules/block.py:83-104, and by
 * GPTModel.forward, flash_attn/models/gpt.py:236-240).
 *   x0       (rows, cols) contiguous, dtype `dtype` (fp16 / bf16)
 *   x1       residual in, (rows, cols) contiguous, fp32 if x1_is_f32 else `dtype`; may be NULL
 *   gamma, beta  (cols), fp32 if w_is_f32 else `dtype`
 *   z        (rows, cols) in `dtype` (the reference's otype = itype, ln_api.cpp:104)
 *   x_out    residual out = x0 + x1 rounded to its dtype (fp32 if xout_is_f32 else `dtype`); may be
 *            NULL.  z is computed from the unrounded fp32 sum (ln_fwd_kernels.cuh:131-133).
 * cols must be a multiple of 4 and <= 8192; all pointers 16-byte aligned.
 */
int bp_add_layer_norm(const void *x0, const void *x1, const void *gamma, const void *beta, void *z,
                      void *x_out, int64_t rows, int cols, float epsilon, int dtype, int x1_is_f32,
                      int xout_is_f32, int w_is_f32, bp_stream_t stream);

/*
 * bp_dropout_add_layer_norm -- the full forward of the reference's dropout_add_ln_fwd minus rowscale / colscale /
 * subset (csrc/layer_norm/ln_api.cpp:83-254; kernel ln_fwd_kernels.cuh:76,112-134):
 *   x = dropout(x0) / (1 - p) + x1 ;  z = LayerNorm(x)
 * Arguments as bp_add_layer_norm, plus
 *   x0_is_f32  x0 (and therefore z: otype = itype, ln_api.cpp:104) is fp32 instead of `dtype` -- the AMP case,
 *              where the fp32 embedding output enters the first LayerNorm; requires an fp32 residual stream
 *   dmask      optional (rows, cols) uint8 keep mask out (1 = kept; 4-byte aligned), written only when p_dropout > 0
 *              -- what `return_dropout_mask=True` hands back (flash_attn/ops/layer_norm.py:207-217)
 *   p_dropout, rng_state   as in bp_flash_fwd_dropout; here ONE stream per call with counter (row, column / 4)
 * rows must be < 2^32.
 */
int bp_dropout_add_layer_norm(const void *x0, const void *x1, const void *gamma, const void *beta, void *z,
                              void *x_out, uint8_t *dmask, int64_t rows, int cols, float epsilon, int dtype,
                              int x0_is_f32, int x1_is_f32, int xout_is_f32, int w_is_f32,
                              float p_dropout, const uint64_t *rng_state, bp_stream_t stream);

/*
 * bp_softmax_bwd_causal -- backward of the causal softmax behind the sense weights (training path of
 * ContextSelfAttn.forward, training/src/models/backpack.py:112-122, which the reference leaves to autograd):
 *   dscores[n,t,s] = scale * alpha[n,t,s] * (dalpha[n,t,s] - sum_{s'<=t} alpha[n,t,s'] dalpha[n,t,s'])  for s <= t,
 *   0 above the diagonal.  In place: `dalpha_inout` holds dalpha on entry and dscores on return.
 *   alpha, dalpha_inout  (n_matrices, seqlen, seqlen) 16-bit contiguous, 16-byte aligned;
 *   seqlen % 8 == 0 and <= 4096 (BP_ERR_SHAPE otherwise)
 */
int bp_softmax_bwd_causal(const void *alpha, void *dalpha_inout, int64_t n_matrices, int seqlen,
                          float softmax_scale, int dtype, bp_stream_t stream);

/*
 * bp_add_layer_norm_bwd -- backward of bp_add_layer_norm (eval-path subset of the reference's
 * dropout_add_ln_bwd, csrc/layer_norm/ln_api.cpp:256-408; Python side flash_attn/ops/layer_norm.py:131-152):
 *   dx = rs (dz*gamma - mean(dz*gamma) - xhat mean(dz*gamma*xhat)) + dx_in ;  dgamma = sum dz*xhat ; dbeta = sum dz
 * with mean / rstd recomputed from `x`, the summed stream the forward normalised (its x_out; x0 itself when
 * the forward had no residual).  dx0 and dx1 receive the same values in their own dtypes.
 *   dz, dx0      (rows, cols) 16-bit           dx_in, x, dx1  (rows, cols) residual dtype (dx_in / dx1 may be NULL)
 *   gamma, dgamma, dbeta  (cols) fp32 or 16-bit (w_is_f32)
 *   ws           fp32 workspace, 2 * BP_LN_BWD_WS_ROWS * cols elements
 * cols % 4 == 0 and <= 2048 (BP_ERR_SHAPE otherwise: callers differentiate the eager expression instead).
 */
#define BP_LN_BWD_WS_ROWS 1024
int bp_add_layer_norm_bwd(const void *dz, const void *dx_in, const void *x, const void *gamma,
                          void *dx0, void *dx1, void *dgamma, void *dbeta, float *ws,
                          int64_t rows, int cols, float epsilon, int dtype, int res_is_f32, int w_is_f32,
                          bp_stream_t stream);

/*
 * bp_dropout_add_layer_norm_bwd -- backward of bp_dropout_add_layer_norm (dropout_add_ln_bwd,
 * ln_api.cpp:256-408): as bp_add_layer_norm_bwd, with dx0 = dropout-masked dx / (1 - p) (dx1 stays dx).  The
 * mask is regenerated from the forward's (p_dropout, rng_state); the reference reads its saved dmask instead.
 *   x0_is_f32  dz and dx0 are fp32 (the forward's x0 / z dtype)
 */
int bp_dropout_add_layer_norm_bwd(const void *dz, const void *dx_in, const void *x, const void *gamma,
                                  void *dx0, void *dx1, void *dgamma, void *dbeta, float *ws,
                                  int64_t rows, int cols, float epsilon, int dtype, int x0_is_f32, int res_is_f32,
                                  int w_is_f32, float p_dropout, const uint64_t *rng_state, bp_stream_t stream);

/*
 * bp_dropout_add_layer_norm_scaled / _scaled_bwd -- bp_dropout_add_layer_norm{,_bwd} with the two scale vectors of the
 * reference's dropout_add_ln_fwd / _bwd (csrc/layer_norm/ln_api.cpp:83-254,256-408; kernels ln_fwd_kernels.cuh:99,123-125,
 * ln_bwd_kernels.cuh:183-195; Python side flash_attn/ops/layer_norm.py:207-217 `rowscale`, `layerscale`):
 *   x = dropout(x0 * rowscale[row]) / (1 - p) * colscale[col] + x1 ;  z = LayerNorm(x)
 *   dx0 = dx * rowscale[row] * mask / (1 - p) * colscale[col] ;  dcolscale[col] = sum_rows dx * rowscale[row] * mask / (1 - p) * x0
 *   rowscale  (rows) in x0's dtype (fp32 when x0_is_f32), or NULL      -- DropPath: Bernoulli(survival) / survival per row
 *   colscale  (cols) in gamma's dtype, or NULL                        -- LayerScale
 *   x0        backward only, the forward's x0 (needed for dcolscale; may be NULL without a colscale)
 *   dcolscale (cols) in gamma's dtype; required with a colscale
 *   ws        fp32 workspace of `ws_floats` elements >= bp_ln_bwd_ws_floats(cols, colscale != NULL) (BP_ERR_WORKSPACE otherwise)
 * With both vectors NULL these are the unscaled entry points (which forward to them).  The `subset` arguments of the
 * reference (x0_subset / out_subset / rowscale_const, a ViT token-dropping feature) are not part of this ABI.
 */
int64_t bp_ln_bwd_ws_floats(int cols, int has_colscale);
int bp_dropout_add_layer_norm_scaled(const void *x0, const void *x1, const void *gamma, const void *beta,
                                     const void *rowscale, const void *colscale, void *z, void *x_out, uint8_t *dmask,
                                     int64_t rows, int cols, float epsilon, int dtype, int x0_is_f32, int x1_is_f32,
                                     int xout_is_f32, int w_is_f32, float p_dropout, const uint64_t *rng_state,
                                     bp_stream_t stream);
int bp_dropout_add_layer_norm_scaled_bwd(const void *dz, const void *dx_in, const void *x, const void *x0,
                                         const void *gamma, const void *rowscale, const void *colscale,
                                         void *dx0, void *dx1, void *dgamma, void *dbeta, void *dcolscale,
                                         float *ws, int64_t ws_floats, int64_t rows, int cols, float epsilon, int dtype,
                                         int x0_is_f32, int res_is_f32, int w_is_f32, float p_dropout,
                                         const uint64_t *rng_state, bp_stream_t stream);

/*
 * bp_add_layer_norm_chain -- inference-only forms of bp_add_layer_norm for a chain of pre-norm blocks: no dropout, no
 * scales, no mask; 16-bit x0a / x0b / z, fp32 residual stream (x1, x_out).
 *   x = (x0a + x1) + x0b   in fp32, in exactly this order ;  z = LayerNorm(x) ;  x_out = x
 * which is, bit for bit, what two bp_add_layer_norm launches give when the first stores x0a + x1 in fp32 and the second
 * adds x0b to it -- without writing and re-reading that fp32 sum.
 *   x0a       (rows, cols) 16-bit, or NULL when the embedding source below is given (exactly one of the two)
 *   x0b, x1   (rows, cols) 16-bit / fp32, either may be NULL (no such term); x1 must be NULL with the embedding source
 *   token_ids, word_table       the embedding source: x0a[r] = word_table[token_ids[r]]; (rows) int64 and
 *                               (table_rows, cols) 16-bit
 *   position_table, position_ids  optional (position_rows, cols) 16-bit: x0a[r] = word row + position row, added in fp32 and
 *                               rounded once to the 16-bit type (a 16-bit add).  Row r takes entry r % position_len of
 *                               position_ids ((position_len) int64), or the position r % position_len itself when
 *                               position_ids is NULL; rows % position_len == 0.
 *                               Ids are clamped, as unsigned values, to the last row of their table.
 *   x_out     fp32 or NULL (z alone); may be x1 itself: every element is read before it is written, by the same lane
 * cols % 4 == 0 and <= 2048, rows < 2^32, pointers 16-byte aligned (ids 8-byte).
 */
int bp_add_layer_norm_chain(const void *x0a, const void *x0b, const void *x1, const int64_t *token_ids,
                            const int64_t *position_ids, const void *word_table, const void *position_table,
                            const void *gamma, const void *beta, void *z, void *x_out, int64_t rows, int cols,
                            int64_t table_rows, int64_t position_rows, int64_t position_len, float epsilon, int dtype,
                            int w_is_f32, bp_stream_t stream);

/*
 * bp_xentropy_fwd / bp_xentropy_bwd -- fused softmax cross-entropy over vocabulary-sized rows.
 * Replace xentropy_cuda_lib.forward(logits, labels, smoothing[, total_classes]) -> (losses, lse) and
 * xentropy_cuda_lib.backward(grad_loss, logits, lse, labels, smoothing, inplace, total_classes)
 * (flash_attn/losses/cross_entropy.py:37,54,103-105):
 *   lse_i  = log sum_j exp(x_ij)
 *   loss_i = (1 - s)(lse_i - x_i[y_i]) + s (lse_i - sum_j x_ij / total_classes)
 *   dx_ij  = g_i (exp(x_ij - lse_i) - (1 - s)[j == y_i] - s / total_classes)
 * A label outside [0, cols) has no x_i[y_i] term (shifted labels of the vocabulary-parallel caller,
 * cross_entropy.py:41-63); rows with the ignore index are zeroed by the caller (:39,:101).
 *   logits       (rows, cols) fp16 / bf16 / fp32 (dtype 0 / 1 / 2), row stride in elements, last stride 1
 *   labels       (rows) int64
 *   losses, lse  (rows) fp32
 *   grad_logits  (rows, cols) in the logits' dtype; MAY BE the logits buffer itself (inplace_backward)
 *   total_classes  <= 0: cols
 */
int bp_xentropy_fwd(const void *logits, const int64_t *labels, float *losses, float *lse,
                    int64_t rows, int cols, int64_t row_stride, float smoothing, int total_classes,
                    int dtype, bp_stream_t stream);
int bp_xentropy_bwd(const float *grad_losses, const void *logits, const float *lse, const int64_t *labels,
                    void *grad_logits, int64_t rows, int cols, int64_t row_stride, int64_t grad_row_stride,
                    float smoothing, int total_classes, int dtype, bp_stream_t stream);

/*
 * bp_bias_gelu_fwd / bp_bias_gelu_bwd / bp_column_sum -- the elementwise halves of the reference's fused dense
 * layers (flash_attn/ops/fused_dense.py:175-330 `FusedDenseGeluDenseFunc`, :27-108 `FusedDenseFunc`), i.e. what the
 * cuBLASLt epilogues of csrc/fused_dense_lib do around the GEMMs (fused_dense.cpp:195-197: `linear_gelu_forward`,
 * `bias_gelu_linear_dgrad_bgrad`, `linear_bias_wgrad`).  The GEMMs stay on the BLAS library.
 *   forward   y = gelu_tanh(x + bias);  pre_out (optional) = x + bias rounded to 16 bit -- y is then the GELU of that
 *             rounded value, so bp_bias_gelu_bwd differentiates exactly what the forward evaluated
 *   backward  dpre = grad * gelu_tanh'(pre);   dbias[c] = sum_r dpre[r,c]   (one pass; deterministic two-stage sum)
 *   column sum  dbias[c] = sum_r grad[r,c]     (bias gradient of a dense layer without activation)
 * gelu_tanh(x) = 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))  (GPT-2 `gelu_new`, F.gelu(approximate='tanh')).
 *   x, grad, pre, pre_out, y, dpre   (rows, cols) 16-bit contiguous, cols % 8 == 0, 16-byte aligned;
 *                                    y may alias x, dpre may alias grad
 *   bias    (cols) 16-bit or NULL (pre_out then must be NULL too: the pre-activation is x itself)
 *   dbias   (cols) fp32 (dbias_is_f32) or 16-bit; NULL in bp_bias_gelu_bwd = no bias gradient wanted
 *   ws      fp32 workspace of bp_bias_grad_ws_floats(rows, cols) elements (contents undefined on entry)
 */
int64_t bp_bias_grad_ws_floats(int64_t rows, int cols);
int bp_bias_gelu_fwd(const void *x, const void *bias, void *pre_out, void *y, int64_t rows, int cols, int dtype,
                     bp_stream_t stream);
int bp_bias_gelu_bwd(const void *grad, const void *pre, void *dpre, void *dbias, float *ws, int64_t rows, int cols,
                     int dtype, int dbias_is_f32, bp_stream_t stream);
int bp_column_sum(const void *grad, void *dbias, float *ws, int64_t rows, int cols, int dtype, int dbias_is_f32,
                  bp_stream_t stream);

/*
 * bp_flash_decode -- trunk attention of ONE new query row per (sample, head) against a KV cache, appending the new
 * token's key and value.  Serves the decode step of the reference's generation contract (flash_attn/modules/mha.py
 * _update_kv_cache + inner_cross_attn with causal=False, flash_attn/utils/generation.py greedy_decode), whose cache is
 *   kv_cache     (batch, max_seqlen, 2, nheads, head_dim) 16-bit, element strides kv_batch / kv_row / kv_two / kv_head,
 *                last stride 1 (the caller offsets the base by batch_size_offset rows)
 *   cache_seqlens  (batch) int32 DEVICE array: cached positions of sample b BEFORE this token, L_b.  The kernel writes
 *                k_new / v_new into cache row L_b and the query attends to rows [0, L_b], the new one included; lengths
 *                may differ between samples.  The host never reads them (one captured graph serves every step); a
 *                length outside [0, max_seqlen - 1] is clamped into it.  The lengths are not advanced here.
 *   q, k_new, v_new  (batch, nheads, head_dim) 16-bit, strides *_batch / *_head, last stride 1
 *   out          (batch, nheads, head_dim) 16-bit, strides o_batch / o_head, last stride 1
 *   softmax_lse  (batch, lse_batch_stride) fp32 or NULL: natural-log LSE of every head's row
 *   ws           fp32 workspace of ws_floats >= bp_flash_decode_ws_floats(batch, nheads, head_dim, max_seqlen)
 *                elements (BP_ERR_WORKSPACE otherwise), contents undefined on entry; it belongs to the call until the
 *                stream has run it
 * Softmax and accumulation in fp32; split over the keys with a fixed-order combine in a second launch: the result is
 * bit-identical across calls (no atomics).  head_dim % 8 == 0 and <= 128 (BP_ERR_HEAD_DIM otherwise); 16-byte aligned
 * bases, strides multiples of 8 (BP_ERR_SHAPE otherwise).
 */
int64_t bp_flash_decode_ws_floats(int batch, int nheads, int head_dim, int max_seqlen);
int bp_flash_decode(const void *q, const void *k_new, const void *v_new, void *kv_cache, const int32_t *cache_seqlens,
                    void *out, float *softmax_lse, float *ws, int64_t ws_floats,
                    int batch, int nheads, int head_dim, int max_seqlen,
                    int64_t q_batch_stride, int64_t q_head_stride,
                    int64_t knew_batch_stride, int64_t knew_head_stride,
                    int64_t vnew_batch_stride, int64_t vnew_head_stride,
                    int64_t kv_batch_stride, int64_t kv_row_stride, int64_t kv_two_stride, int64_t kv_head_stride,
                    int64_t o_batch_stride, int64_t o_head_stride, int64_t lse_batch_stride,
                    float softmax_scale, int dtype, bp_stream_t stream);

/*
 * bp_sense_decode -- the Backpack sense contraction for ONE new position t per sample (training/src/models/backpack.py
 * :297-314 restricted to the last row), appending the new position's sense key and row index:
 *   out[b,:] = sum_l sum_{j<=t} softmax_j(scale q[b,l,:].k_l(j)) table[row(b,j), l, :],   t = L_b = cache_seqlens[b]
 *   q, k_new     (batch, nsenses, d_k) 16-bit: the q / k halves of ContextSelfAttn.project for the new token, strides
 *                *_batch / *_sense, last stride 1
 *   k_cache      (batch, max_seqlen, nsenses, d_k) 16-bit sense keys of the cached positions, strides kc_batch / kc_row /
 *                kc_sense, last stride 1; row L_b is written with k_new
 *   table        (table_rows, nsenses, d_out) 16-bit sense vectors, strides t_row / t_sense, last stride 1: the whole-
 *                vocabulary sense table (row = token id) or a per-position content cache (row = b * max_seqlen + j)
 *   row_index    (batch, max_seqlen) int32, stride idx_batch: table row of every cached position; entry L_b is written
 *                with new_row[b].  Rows are clamped as unsigned values to table_rows - 1 (as bp_sense_mix_gather)
 *   new_row      (batch) int32 table row of the new position
 *   cache_seqlens  as in bp_flash_decode
 *   out          (batch, d_out) 16-bit, batch stride o_batch, last stride 1
 *   ws           fp32 workspace of ws_floats >= bp_sense_decode_ws_floats(batch, nsenses, d_out, max_seqlen) elements
 * A separate softmax per sense, fp32 accumulation, split over the keys with a fixed-order combine (no (batch, nsenses, t)
 * weight tensor in memory, bit-identical across calls).  1 <= nsenses <= 64, d_k % 8 == 0 and <= 640 (BP_ERR_HEAD_DIM),
 * d_out >= 1 (BP_ERR_DOUT), d_out % 8 == 0 and <= 2048, 16-byte aligned bases, strides multiples of 8 (BP_ERR_SHAPE).
 */
int64_t bp_sense_decode_ws_floats(int batch, int nsenses, int d_out, int max_seqlen);
int bp_sense_decode(const void *q, const void *k_new, void *k_cache, const void *table, int32_t *row_index,
                    const int32_t *new_row, const int32_t *cache_seqlens, void *out, float *ws, int64_t ws_floats,
                    int batch, int nsenses, int d_k, int d_out, int max_seqlen, int64_t table_rows,
                    int64_t q_batch_stride, int64_t q_sense_stride,
                    int64_t knew_batch_stride, int64_t knew_sense_stride,
                    int64_t kc_batch_stride, int64_t kc_row_stride, int64_t kc_sense_stride,
                    int64_t t_row_stride, int64_t t_sense_stride, int64_t idx_batch_stride,
                    int64_t o_batch_stride, float softmax_scale, int dtype, bp_stream_t stream);

/*
 * bp_sense_decode_weighted -- bp_sense_decode with the intervention hook of bp_sense_mix_weighted, restricted to the
 * last row (training/src/models/intervened_models.py:78-101, test_genderbias.py:71-78 on a KV cache):
 *   out[b,:] = sum_l sum_{j<=t} softmax_j(scale q[b,l,:].k_l(j)) key_weight[b,l,j] table[row(b,j), l, :]
 *   key_weight   (batch, nsenses, max_seqlen) fp32, element strides kw_batch / kw_sense (each >= max_seqlen), unit stride
 *                along the positions.  Entries [0, L_b] are read, entry L_b (the new position's) included: the caller
 *                fills it before the call.  Never written.  The weight multiplies the normalised probability and does
 *                not enter the softmax.  NULL: bp_sense_decode exactly (the strides are then ignored)
 * Every other operand, the append of key and row index, the clamps, the split and its fixed-order combine, the limits and
 * the error codes are bp_sense_decode's; the workspace is sized by bp_sense_decode_ws_floats.
 */
int bp_sense_decode_weighted(const void *q, const void *k_new, void *k_cache, const void *table, int32_t *row_index,
                             const int32_t *new_row, const int32_t *cache_seqlens, const float *key_weight, void *out,
                             float *ws, int64_t ws_floats,
                             int batch, int nsenses, int d_k, int d_out, int max_seqlen, int64_t table_rows,
                             int64_t q_batch_stride, int64_t q_sense_stride,
                             int64_t knew_batch_stride, int64_t knew_sense_stride,
                             int64_t kc_batch_stride, int64_t kc_row_stride, int64_t kc_sense_stride,
                             int64_t t_row_stride, int64_t t_sense_stride, int64_t idx_batch_stride,
                             int64_t o_batch_stride, int64_t kw_batch_stride, int64_t kw_sense_stride,
                             float softmax_scale, int dtype, bp_stream_t stream);

/*
 * bp_sense_rows_dot -- dot products of the sense vectors of every cached position, and of the new one, with one vector
 * per sample: the update of the running similarity sums of mask_annealing (intervened_models.py:29-53) in a decode step,
 *   out[b,l,j] = sum_c table[row(b,j), l, c] * vec[b,c],   j = 0 .. L_b,   row(b, L_b) = new_row[b]
 *   table, row_index, new_row, cache_seqlens, table_rows   as in bp_sense_decode, clamps included; nothing but `out` is
 *                written (row_index in particular is only read, entry L_b not at all)
 *   vec          (batch, d_out) 16-bit, batch stride vec_batch, last stride 1
 *   out          (batch, nsenses, max_seqlen) fp32, element strides o_batch / o_sense (each >= max_seqlen), unit stride
 *                along the positions; entries j > L_b are left untouched
 * fp32 accumulation in a fixed order (bit-identical across calls); the lengths are read on the device only.
 * 1 <= nsenses <= 64, d_out >= 1 (BP_ERR_DOUT), d_out % 8 == 0 and <= 2048, table and vec 16-byte aligned, their strides
 * multiples of 8 (BP_ERR_SHAPE).
 */
int bp_sense_rows_dot(const void *table, const int32_t *row_index, const int32_t *new_row, const int32_t *cache_seqlens,
                      const void *vec, float *out,
                      int batch, int nsenses, int d_out, int max_seqlen, int64_t table_rows,
                      int64_t t_row_stride, int64_t t_sense_stride, int64_t idx_batch_stride, int64_t vec_batch_stride,
                      int64_t o_batch_stride, int64_t o_sense_stride, int dtype, bp_stream_t stream);

/*
 * bp_pick_token -- the next token of every row of logits, chosen on the device: the pick of a decode step (the
 * reference's greedy_decode / sample, flash_attn/utils/generation.py, pick on the host with torch.argmax /
 * torch.multinomial; its control baseline samples with temperature and top_k, training/run_pplm.py:80,347-348,569-581).
 * No host value enters the pick, so one captured launch serves every step of a replayed decode graph.
 *   logits     (batch, vocab) fp16 / bf16 / fp32 (dtype 0 / 1 / 2), element stride row_stride >= vocab, last stride 1, any
 *              element-aligned base (16-byte loads start at the first 16-byte boundary).  Only read.
 *   tokens     int64, the pick of row b at tokens[b * tokens_stride]
 *   sequences  optional int64 (batch, seq_stride): row b, column counters[b] also receives the pick; the write is skipped
 *              when that column is outside [0, seq_cols)
 *   stats      optional fp32 (batch, 4) contiguous: {lowest kept z, natural-log sum-exp of the kept z, kept count, u}; greedy and
 *              degenerate rows report the maximum twice and a count of 1
 *   rng_state  DEVICE {seed, offset} as in bp_flash_fwd_dropout; read when do_sample, never written
 *   counters   optional int32 (batch) on the device; NULL means 0 for every row
 * do_sample == 0: the lowest index of the maximal logit; a NaN counts as larger than every number (torch.argmax).
 * do_sample != 0, with z_i = float(x_i) * (1 / temperature) (the reciprocal rounded to fp32 first):
 *   top_k   0 < top_k < vocab: tau = the top_k-th largest z counted with multiplicity, keep z_i >= tau (ties at the threshold
 *           are all kept); top_k <= 0 or >= vocab: off
 *   top_p   < 1: on the probabilities renormalised over what top_k kept, keep i iff the total probability of kept tokens
 *           with z_j > z_i is < top_p (equal logits share a fate; without ties the smallest prefix whose mass reaches top_p)
 *   u       ((r0 >> 8) + 0.5) * 2^-24 as a real number in (0, 1) (stats holds its fp32 rounding), (r0, _) =
 *           philox2x32(counters[b], salt, key) with (key, salt) the stream of index b of rng_state (csrc/bp_philox.h;
 *           tests/philox_ref.py: stream, philox2x32)
 *   token   the lowest index t, in vocabulary order, whose cumulative kept probability through t exceeds u
 *   a row whose kept mass is not positive and finite (a NaN or +inf among the z, or no finite z) takes the do_sample == 0 answer
 * Probabilities are exp(z_i - max z) in 40-bit fixed point, so every sum is an integer sum: the result is a pure function of
 * the arguments, bit for bit, whatever the order of the additions.
 * Errors, before any launch: BP_ERR_DTYPE; BP_ERR_SHAPE (batch or vocab < 1, vocab > 2^23, row_stride < vocab, tokens_stride
 * < 1, sequences with seq_cols < 1 or seq_stride < seq_cols, a NULL logits / tokens, a misaligned pointer); BP_ERR_SCALE
 * (temperature not finite or not > 0, checked for greedy calls too); BP_ERR_SAMPLING (top_p outside (0, 1]; do_sample with a
 * NULL rng_state).
 */
int bp_pick_token(const void *logits, int64_t *tokens, int64_t *sequences, float *stats, const uint64_t *rng_state,
                  const int32_t *counters, int batch, int vocab, int64_t row_stride, int64_t tokens_stride,
                  int64_t seq_stride, int seq_cols, int do_sample, float temperature, int top_k, float top_p, int dtype,
                  bp_stream_t stream);

/*
 * bp_pick_token_ctl -- bp_pick_token with the controls a generation loop needs to stop and not to loop: a repetition
 * penalty over the row's history (the reference's control baseline samples with temperature, top_k and
 * repetition_penalty, training/run_pplm.py:544-550, over set(output_so_far[0].tolist())), an EOS id that is masked below a
 * minimal length, and per-row finished flags.  Arguments as bp_pick_token's, and
 *   finished   optional int32 (batch) on the device, read and written
 * Per row b, with c = counters[b] (0 when counters is NULL):
 *   finished on entry (finished != NULL and finished[b] != 0): the token is pad_token_id, written to tokens and to column c
 *           of sequences as usual; no draw is made; stats = {0, 0, 0, u} (u = 0 when not do_sample); finished[b] stays set
 *   history H_b = the set of values of sequences[b, 0 : min(c, seq_cols)] inside [0, vocab): values outside are ignored,
 *           duplicates count once, sequences == NULL or c <= 0 give the empty set -- the prompt plus what was generated
 *   pen(z)  z for i not in H_b; for i in H_b: z * theta when z < 0, otherwise z * rtheta, theta = repetition_penalty,
 *           rtheta = 1 / theta rounded to fp32 (as 1 / temperature is): ONE fp32 multiplication either way; a NaN or an
 *           infinity passes through it.  theta == 1 skips the history altogether
 *   EOS     eos_token_id >= 0 and c < min_length: the EOS entry counts as -inf, in the greedy answer, in top_k, in top_p
 *           and in the draw.  min_length is the absolute sequence length, prompt included
 *   greedy  (do_sample == 0, and the answer of degenerate rows) the lowest index of the maximum of pen(float(x_i)) under
 *           the EOS mask, a NaN largest; temperature does not enter
 *   sampling  z_i = pen(float(x_i) * (1 / temperature)) under the EOS mask, then top_k, top_p, u and the vocabulary-order
 *           draw exactly as bp_pick_token states them, on 40-bit fixed-point masses; stats reports the lowest kept z, the
 *           log-sum-exp, the kept count and u in terms of these z
 *   after the pick: finished != NULL, eos_token_id >= 0 and token == eos_token_id set finished[b] = 1 (the EOS token
 *           itself is written, not the pad)
 * With every control off (repetition_penalty == 1, eos_token_id < 0, finished == NULL) tokens and stats are bp_pick_token's,
 * bit for bit.  The history is a bitmap in LDS, one bit per vocabulary entry, which bounds vocab by 2^19 under a penalty.
 * Errors, before any launch: everything bp_pick_token rejects, with its codes; BP_ERR_SAMPLING (repetition_penalty not
 * finite or not > 0; repetition_penalty != 1 with sequences == NULL; eos_token_id >= 0 with finished == NULL);
 * BP_ERR_SHAPE (eos_token_id >= vocab; pad_token_id outside [0, vocab) when finished != NULL; min_length < 0; a
 * misaligned finished; vocab > 2^19 with repetition_penalty != 1).
 */
int bp_pick_token_ctl(const void *logits, int64_t *tokens, int64_t *sequences, float *stats, const uint64_t *rng_state,
                      const int32_t *counters, int32_t *finished,
                      int batch, int vocab, int64_t row_stride, int64_t tokens_stride, int64_t seq_stride, int seq_cols,
                      int do_sample, float temperature, int top_k, float top_p,
                      float repetition_penalty, int eos_token_id, int pad_token_id, int min_length,
                      int dtype, bp_stream_t stream);

/*
 * bp_pick_token_lim -- bp_pick_token_ctl with limits on what a row may say: n-gram blocking, frequency and presence
 * penalties over the row's history, and a list of suppressed ids (the no_repeat_ngram_size, frequency_penalty /
 * presence_penalty and suppress_tokens of the common generation libraries).  (Additive, ABI still 11.)  Arguments as
 * bp_pick_token_ctl's, and
 *   no_repeat_ngram_size  n, 0 = off
 *   frequency_penalty, presence_penalty  fp32, any finite value (negative ones reward repetition); 0 and 0 = off
 *   penalty_begin  the first history position that is counted: the generation loops pass the prompt length, so the
 *                  penalties count generated tokens only; 0 counts the prompt too
 *   suppress_ids, n_suppress  device int32 list of ids that are never picked; ids outside [0, vocab) are ignored
 * Per row b, with c = counters[b], the history h = sequences[b, 0 : Lh], Lh = min(max(c, 0), seq_cols) (0 when sequences is
 * NULL; when c > seq_cols the history is the clamped one, as for bp_pick_token_ctl):
 *   finished on entry: the pad, exactly as bp_pick_token_ctl, before anything else
 *   an element's value is v = float(x), or float(x) * (1 / temperature) for sampling, and then in this order
 *   1  pen(v), bp_pick_token_ctl's repetition penalty over the set of h (prompt included), unchanged
 *   2  counts: n_v = the number of j in [min(penalty_begin, Lh), Lh) with h[j] == the element's id; when n_v > 0,
 *      v = v - fmaf(frequency_penalty, float(n_v), presence_penalty): one fp32 fma and one subtraction (the OpenAI / vLLM
 *      form); a NaN or an infinity passes through
 *   3  ban: v = -inf when the id is in suppress_ids, or in the n-gram set, or is the EOS id while c < min_length
 *   n-gram set (n >= 1): { h[i + n - 1] : 0 <= i <= Lh - n, h[i + t] == h[Lh - n + 1 + t] for all 0 <= t <= n - 2 } inside
 *      [0, vocab): the ids that would complete an n-gram the history already holds, prompt included.  The raw int64 values
 *      are compared, so ids outside the vocabulary match each other; n = 1 bans every id of h; Lh < n bans nothing
 *   the greedy answer, top_k, top_p, the draw and stats are bp_pick_token_ctl's on these values.  A row left without a
 *   finite value is degenerate and takes the greedy answer, which for a row of -inf is index 0 -- also when 0 is banned
 * With the controls off (n = 0, both penalties 0, n_suppress = 0) tokens and stats are bp_pick_token_ctl's, bit for bit.
 * Per-row state lives in LDS: the history bitmap, a ban bitmap of the same shape, and for the counts an open-addressing
 * table of 32-bit entries (id in the low 19 bits, count in the high 13) with the power of two >= 2 seq_cols slots.  No global
 * workspace, no global atomics.
 * Errors, before any launch: everything bp_pick_token_ctl rejects, with its codes; BP_ERR_SAMPLING (a non-finite penalty;
 * n > 0 or a non-zero penalty with sequences == NULL; n_suppress > 0 with a NULL or misaligned list); BP_ERR_SHAPE (n outside
 * 0..BP_PICK_MAX_NGRAM; n_suppress < 0; penalty_begin < 0; vocab > BP_PICK_MAX_LIMITED_VOCAB with any of these controls on;
 * seq_cols > BP_PICK_MAX_COUNTED_COLS with a non-zero penalty; static + dynamic LDS above BP_PICK_MAX_LDS_BYTES: 68 112 bytes
 * static, (vocab + 31) / 32 + 1 words per bitmap in use, 4 bytes per slot).
 */
int bp_pick_token_lim(const void *logits, int64_t *tokens, int64_t *sequences, float *stats, const uint64_t *rng_state,
                      const int32_t *counters, int32_t *finished,
                      int batch, int vocab, int64_t row_stride, int64_t tokens_stride, int64_t seq_stride, int seq_cols,
                      int do_sample, float temperature, int top_k, float top_p,
                      float repetition_penalty, int eos_token_id, int pad_token_id, int min_length,
                      int no_repeat_ngram_size, float frequency_penalty, float presence_penalty, int penalty_begin,
                      const int32_t *suppress_ids, int n_suppress, int dtype, bp_stream_t stream);

/*
 * bp_pick_token_lim_rows -- bp_pick_token_lim for a batch whose rows begin at different positions (right-padded prompts of
 * different lengths): the two values that bp_pick_token_lim takes as one scalar for the whole batch may come per row.
 * (Additive, ABI still 11.)  Arguments as bp_pick_token_lim's, and
 *   penalty_begins  optional int32 (batch) on the device: row b counts its history from penalty_begins[b] on; replaces
 *                   penalty_begin, which is then neither read nor checked
 *   min_lengths     optional int32 (batch) on the device: the EOS id of row b is masked while c < min_lengths[b]; replaces
 *                   min_length, which is then neither read nor checked
 * The host never reads the arrays (one captured launch serves every step): a negative entry counts as 0, on the device.
 * Everything else is bp_pick_token_lim's contract with the row's value in the scalar's place: the clamp min(begin, Lh), the
 * order pen -> counts -> ban, stats, degenerate rows, finished rows, the bounds.  With both arrays NULL, or with arrays that
 * hold the scalar in every row, tokens and stats are bp_pick_token_lim's, bit for bit.
 * Errors, before any launch: everything bp_pick_token_lim rejects, with its codes, where penalty_begin < 0 and
 * min_length < 0 are rejected only when the respective array is NULL; BP_ERR_SHAPE (a misaligned array).
 */
int bp_pick_token_lim_rows(const void *logits, int64_t *tokens, int64_t *sequences, float *stats, const uint64_t *rng_state,
                           const int32_t *counters, int32_t *finished,
                           int batch, int vocab, int64_t row_stride, int64_t tokens_stride, int64_t seq_stride, int seq_cols,
                           int do_sample, float temperature, int top_k, float top_p,
                           float repetition_penalty, int eos_token_id, int pad_token_id, int min_length,
                           int no_repeat_ngram_size, float frequency_penalty, float presence_penalty, int penalty_begin,
                           const int32_t *suppress_ids, int n_suppress, const int32_t *penalty_begins,
                           const int32_t *min_lengths, int dtype, bp_stream_t stream);

/*
 * bp_pick_token_phrases -- bp_pick_token_lim_rows with two lists of phrases of token ids: banned phrases (the bad_words_ids of
 * the common generation libraries: the LAST id of a phrase is banned while the row's text ends with the ids in front of it)
 * and stop phrases (a row whose generated text ends with one is finished, as by its EOS id).  (Additive, ABI still 11.)
 * Arguments as bp_pick_token_lim_rows's, and
 *   ban_ids, ban_offsets, n_ban, ban_total      int32 arrays on the device: phrase j is ban_ids[ban_offsets[j] :
 *                   ban_offsets[j + 1]], ban_offsets has n_ban + 1 entries, ban_ids has ban_total
 *   stop_ids, stop_offsets, n_stop, stop_total  the stop phrases, in the same form
 *   ends, reasons   optional int32 (batch) each, written for the rows this call finishes
 * The host never reads the arrays (one captured launch serves every step), so the device checks them: a phrase whose offsets
 * leave [0, total] or whose length lies outside 1..BP_PICK_MAX_PHRASE_LEN is ignored (decreasing offsets among them).
 * Per row b, with c, h, Lh as bp_pick_token_lim defines them, g_b = penalty_begins[b], else penalty_begin, clamped at 0, and
 * m_b = min_lengths[b], else min_length, clamped at 0:
 *   ban     a ban phrase w[0..L) matches when Lh >= L - 1 and h[Lh - L + 1 + t] == w[t] for all 0 <= t <= L - 2 (prompt
 *           included, as for the n-gram set; the int64 history against the sign-extended int32 id, so ids outside the
 *           vocabulary match by value).  A match adds w[L - 1] to the banned ids of step 3 of bp_pick_token_lim when it lies
 *           in [0, vocab); L = 1 always bans its id.  Everything behind the ban is the limited form's: the order pen ->
 *           counts -> ban, the degenerate row of -inf taking index 0, stats
 *   stop    after the token t of a row that was not finished on entry has been written, only when sequences != NULL and
 *           0 <= c < seq_cols (h is unclamped and the token has a column) and c >= m_b (the EOS id is no longer masked):
 *           with h' = h ++ [t], stop phrase j of length L matches when c + 1 - L >= g_b (the whole match is generated text: a
 *           prompt that ends with the phrase, or a match across the prompt's end, stops nothing) and h'[c + 1 - L + i] == w[i]
 *           for all 0 <= i < L.  Any match sets finished[b] = 1; the token stays, as the EOS token does, and later picks of
 *           the row write the pad
 *   ends, reasons   whenever this call sets finished[b], for the EOS id or a stop phrase: ends[b] = c + 1 and reasons[b] = 0
 *           for the EOS id, else 1 + j for the lowest matching j (the EOS id wins).  Neither is touched for a row that does
 *           not finish in this call or was finished on entry
 * With n_ban == n_stop == 0 and ends == reasons == NULL tokens, stats, the written column and the flags are
 * bp_pick_token_lim_rows's, bit for bit.  The stop phrases are matched by the whole workgroup, one phrase per thread, each
 * comparing backwards from the new token; the ban list is scanned the same way before the first pass over the row.
 * Errors, before any launch: everything bp_pick_token_lim_rows rejects, with its codes; BP_ERR_SAMPLING (a list with n > 0
 * whose ids or offsets are NULL, or with sequences == NULL; n_stop > 0 with finished == NULL); BP_ERR_SHAPE (n or total
 * negative; n > BP_PICK_MAX_PHRASES; a misaligned ids, offsets, ends or reasons; vocab > BP_PICK_MAX_LIMITED_VOCAB with
 * n_ban > 0; the LDS bound, where n_ban > 0 counts a ban bitmap).
 */
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
                          int32_t *ends, int32_t *reasons, int dtype, bp_stream_t stream);

/*
 * bp_beam_pick -- one decode step of beam search on the device for `groups` prompts x `beam_width` (W, 1..8) hypotheses,
 * rows r = g * W + w.  No host value enters, so one captured launch serves every step.  (Additive, ABI still 11.)
 *   logits       (groups * W, vocab) fp16 / bf16 / fp32, element stride row_stride >= vocab, last stride 1, any
 *                element-aligned base, as bp_pick_token's.  Only read.
 *   beam_scores  fp32 (groups * W), read and written: the sum of log-probabilities of every hypothesis
 *   finished     int32 (groups * W), read and written; NULL is allowed only with eos_token_id < 0
 *   parent       int32 (groups * W), written: the GLOBAL row index of the hypothesis every slot continues
 *   tokens       int64, the token of slot r at tokens[r * tokens_stride]
 *   sequences, seq_stride, seq_cols, counters   as bp_pick_token's: row r receives its token at column counters[r]; the
 *                write is skipped when that column is outside [0, seq_cols)
 *   ws, ws_floats  fp32 workspace of >= bp_beam_pick_ws_floats(groups, beam_width) elements, 8-byte aligned; contents
 *                undefined on entry, it belongs to the call until the call has completed on the stream
 * Per group g, with s_w = beam_scores[g W + w]:
 *   1 candidates  a live row w (finished NULL or 0): m = max_v float(x_v), lse = m + log sum_v exp(float(x_v) - m) in fp32
 *                 (the sum in 40-bit fixed point, as bp_pick_token's masses); candidate (w, v) has the score
 *                 s_w + (float(x_v) - lse), the two fp32 operations in that order.  A finished row contributes exactly one
 *                 candidate, (w, pad_token_id), with the score s_w unchanged: the frozen hypothesis.  A candidate whose score
 *                 is NaN ranks, and is written, as -inf (and -0 as +0).  A live row with a NaN or +inf logit, or without a
 *                 finite logit, has all its candidates at -inf.
 *   2 selection   candidates are ranked by (score descending, w ascending, v ascending); the first W win (vocab >= W, so
 *                 they exist).
 *   3 slots       a surviving hypothesis never moves: the winners are walked in rank order, and a winner takes slot w, its
 *                 parent's, if that slot is still free; then the rest, in rank order, each take the lowest free slot.
 *                 CONSEQUENCE: every slot that another slot names as parent also names itself,
 *                 parent[parent[r]] == parent[r] -- bp_beam_copy_rows relies on it.
 *   4 writes      slot t holding the winner (w, v, score): parent[g W + t] = g W + w; tokens and column counters[g W + t] of
 *                 sequences take v; beam_scores[g W + t] = score; finished[g W + t] = old finished[g W + w] | (w live and
 *                 v == eos_token_id).  All old scores and flags of the group are read before any is written.
 *   5 first step  needs no mode of its own: with beam_scores = {0, -inf, ..., -inf} all W winners come from beam 0.
 * Integer keys and integer sums: the result is bit-identical across calls.
 * Errors, before any launch: BP_ERR_DTYPE; BP_ERR_SHAPE (groups < 1, beam_width outside 1..8, vocab < beam_width or > 2^23,
 * row_stride < vocab, tokens_stride < 1, sequences with seq_cols < 1 or seq_stride < seq_cols, a NULL logits / beam_scores /
 * parent / tokens / ws, a misaligned pointer, eos_token_id >= vocab, pad_token_id outside [0, vocab) when finished != NULL);
 * BP_ERR_SAMPLING (eos_token_id >= 0 with finished == NULL); BP_ERR_WORKSPACE.
 */
int64_t bp_beam_pick_ws_floats(int groups, int beam_width);
int bp_beam_pick(const void *logits, float *beam_scores, int32_t *finished, int32_t *parent, int64_t *tokens,
                 int64_t *sequences, const int32_t *counters, float *ws, int64_t ws_floats,
                 int groups, int beam_width, int vocab, int64_t row_stride, int64_t tokens_stride, int64_t seq_stride,
                 int seq_cols, int eos_token_id, int pad_token_id, int dtype, bp_stream_t stream);

/*
 * bp_beam_copy_rows -- the caches follow the hypotheses, in one launch for all of them.  A "row set" is a buffer of `rows`
 * rows, row r at bases[i] + r * row_strides[i] bytes, holding max_positions positions of pos_bytes[i] contiguous bytes each
 * (a KV cache, a sequence buffer).  For every set and every row r with parent[r] != r, the bytes of positions
 * [first_position, lengths[r]) of row parent[r] are copied to row r.  Rows with parent[r] == r, and bytes outside the copied
 * range, are not touched.  A length outside [0, max_positions] is clamped; a parent outside [0, rows) leaves its row alone.
 *   bases, row_strides, pos_bytes   HOST arrays of nsets entries, read during the call and passed to the kernel by value
 *                (a captured graph keeps them: the buffers must not move)
 *   parent, lengths   int32 (rows) on the device; first_position, max_positions host values
 * THE CALLER GUARANTEES parent[parent[r]] == parent[r] (bp_beam_pick's slot rule does): sources are then never written, and
 * the plain copy is correct in place.
 * Errors, before any launch: BP_ERR_SHAPE (nsets outside 1..32, rows outside 1..65535, a NULL argument, a base that is not
 * 16-byte aligned, a row stride that is not a multiple of 16 or smaller than max_positions * pos_bytes, pos_bytes < 4 or not
 * a multiple of 4, a negative first_position or max_positions).
 */
int bp_beam_copy_rows(const void *const *bases, const int64_t *row_strides, const int64_t *pos_bytes, int nsets,
                      const int32_t *parent, const int32_t *lengths, int rows, int first_position, int max_positions,
                      bp_stream_t stream);

/*
 * bp_scatter_packed_rows -- the rows of a packed batch land in padded buffers, in one launch for all of them: the prefill of
 * the KV caches from packed prompts.  A "row set" is a source of total_rows rows, row t at src[i] + t * src_row_strides[i]
 * bytes, and a destination whose entry [b][j] lies at dst[i] + b * dst_batch_strides[i] + j * dst_pos_strides[i]; a row is
 * row_bytes[i] contiguous bytes at both ends.  For every set i, every sample b < batch and every position
 * j < min(len_b, max_seqlen, max_positions), len_b = cu_seqlens[b + 1] - cu_seqlens[b], row cu_seqlens[b] + j of the source
 * is copied to [b][j] of the destination.  No other byte of any destination is written.  (Additive, ABI still 11.)
 *   src, src_row_strides, dst, dst_batch_strides, dst_pos_strides, row_bytes   HOST arrays of nsets entries, read during
 *                the call and passed to the kernel by value (a captured graph keeps them: the buffers must not move)
 *   cu_seqlens   int32 (batch + 1) on the device, read on the device only: the call reads no host value that depends on
 *                it and is legal while a stream is capturing.  It is NOT trusted: a negative length counts as 0, a length
 *                is clamped as above, and a source row outside [0, total_rows) is skipped -- whatever cu_seqlens holds,
 *                nothing is read outside the sources and nothing is written outside [b][0, max_positions) of a destination.
 *   total_rows, max_seqlen, max_positions   host values; min(max_seqlen, max_positions) == 0 is a successful no-op
 * A set whose bases, strides and row_bytes are all multiples of 16 moves 16-byte words, any other set dwords.
 * Sources and destinations must not overlap.
 * Errors, before any launch: BP_ERR_SHAPE (nsets outside 1..32, batch outside 1..65535, a NULL argument or entry, a base, a
 * stride or a row_bytes that is not a multiple of 4, row_bytes < 4 or larger than the set's source row stride or destination
 * position stride, a negative destination batch stride, a negative max_seqlen, max_positions or total_rows).
 */
int bp_scatter_packed_rows(const void *const *src, const int64_t *src_row_strides, void *const *dst,
                           const int64_t *dst_batch_strides, const int64_t *dst_pos_strides, const int64_t *row_bytes,
                           int nsets, const int32_t *cu_seqlens, int batch, int64_t total_rows, int max_seqlen,
                           int max_positions, bp_stream_t stream);

/*
 * bp_segment_sum_rows -- deterministic fp32 sums of 16-bit rows over the segments of a sorted index:
 *     acc[u, c]  (= or +=)  sum over i in [seg_begin[u], seg_begin[u + 1])  of  rows[order[i], c]
 * The gradient of a table row that several positions read (an embedding-style backward): torch's index_add_ does this sum
 * with atomics, in the tensor's 16-bit dtype.  Here the sum is kept in fp32, no atomic is used, and every (segment, column)
 * has one owner: the bits of the result depend on the inputs only -- on a segment's rows and their order, not on the grid,
 * the schedule, the run, or where the segment stands among the others.  (Additive, ABI still 11.)
 *   rows         (n_rows, cols) fp16 / bf16, element stride rows_stride >= cols, last stride 1, 16-byte aligned base,
 *                cols and rows_stride multiples of 8, 8 <= cols <= BP_SEGMENT_SUM_MAX_COLS.  Only read.
 *   order        int32 (n_rows): the row numbers grouped by segment, ascending inside a segment (what a stable sort of the
 *                rows' segment numbers returns).  NOT validated: a value is clamped, unsigned, to n_rows - 1.
 *   seg_begin    int32 (n_segments + 1), non-decreasing.  NOT validated either: a value is clamped to [0, n_rows], a
 *                decreasing pair is an empty segment -- nothing is read outside rows / order.
 *   acc          fp32 (n_segments, cols), element stride acc_stride >= cols, a multiple of 4, 16-byte aligned base.  No
 *                element outside rows [0, n_segments), columns [0, cols) is written.
 *   accumulate   0: acc is overwritten, an empty segment writes zeros; 1: the sum is added to acc (one fp32 add per element),
 *                an empty segment leaves its row untouched
 *   n_rows >= 0, 0 <= n_segments <= BP_SEGMENT_SUM_MAX_SEGMENTS; n_segments == 0 is a successful no-op
 * A segment of fewer than 32 rows is summed row after row; a longer one by 16 lanes that take rows r, r + 16, ... each, whose
 * partial sums are added in ascending r.  One launch, no workspace, no host value read from the device.
 * Errors, before any launch: BP_ERR_DTYPE; BP_ERR_SHAPE (a NULL or misaligned pointer, cols outside its range or not a
 * multiple of 8, a stride below cols or not a multiple of 8 / 4, n_rows outside [0, 2^31 - 1], n_segments outside its range,
 * accumulate not 0 / 1).
 */
#define BP_SEGMENT_SUM_MAX_COLS (1 << 24)
#define BP_SEGMENT_SUM_MAX_SEGMENTS (0x7fffffff - 4096)
int bp_segment_sum_rows(const void *rows, const int32_t *order, const int32_t *seg_begin, float *acc, int64_t n_rows,
                        int64_t n_segments, int cols, int64_t rows_stride, int64_t acc_stride, int accumulate, int dtype,
                        bp_stream_t stream);

/*
 * bp_row_extremes -- the n largest and the n smallest elements of every row of a (rows, cols) matrix, with their columns,
 * in order: what a full sort of C_l(x) @ E^T is read for (the reference's training/src/visualize_vocab.py:74-81) and, with
 * n = 1, the row maximum of training/src/rank_vocab.py:84.  One launch that reads no host value.  (Additive, ABI still 11.)
 *   logits       (rows, cols) fp16 / bf16 / fp32, element stride row_stride >= cols, last stride 1, any element-aligned
 *                base.  Only read.
 *   n            1 <= n <= min(cols, BP_ROW_EXTREMES_MAX_N)
 *   top_val, top_idx   fp32 / int32 (rows, n) dense: the n largest elements of every row, largest first
 *   bot_val, bot_idx   fp32 / int32 (rows, n) dense: the n smallest, smallest first
 *                Any of the four may be NULL; an end whose two pointers are NULL is not computed.
 * The row is a total order on integers: an element's key is the order-preserving integer key of its RAW bits (sign bit set:
 * all bits flipped, else the sign bit flipped), so -0 < +0 and NaNs sit at the ends by their sign.  "Largest" ranks by (key
 * descending, column ascending), "smallest" by (key ascending, column ascending); *_val is float(element).  The answer is
 * unique and bit-identical across calls.
 * Errors, before any launch: BP_ERR_DTYPE; BP_ERR_SHAPE (n out of range, cols < 1 or > 2^31 - 1 - 16, rows < 0,
 * row_stride < cols, a NULL logits with rows > 0, a misaligned pointer).  rows == 0 is a successful no-op.
 */
int bp_row_extremes(const void *logits, float *top_val, int32_t *top_idx, float *bot_val, int32_t *bot_idx,
                    int rows, int cols, int64_t row_stride, int n, int dtype, bp_stream_t stream);

/*
 * bp_sense_attribute -- the share of every (context position, sense) pair in a logit.  The Backpack's logit of word w at
 * position i is sum_l sum_{j<=i} alpha^l_ij <C_l(x_j), E[w]> (no norm and no bias lie between the combination and the tied
 * LM head), and the summand is what the reference's training/src/localize_pred.py:25-65 reads off a (B, k, S, vocab)
 * product and a full (B, k, S, S) alpha.  Here, for nq queries, query n = position i_n = query_pos[n] of sample
 * b_n = query_sample[n], each with nvec fp32 vectors:
 *   s_j  = scale * sum_c q_l[b_n, i_n, c] * k_l[b_n, j, c]         fp32, one accumulator, ascending c;  j = 0 .. i_n
 *   m    = max_j s_j,  e_j = exp(s_j - m),  Z = sum_j e_j (fixed order),  p_j = e_j / Z
 *   out[n, v, l, j] = p_j * sum_c table[row(b_n, j), l, c] * vec[n, v, c]      j <= i_n
 *   out[n, v, l, j] = 0                                                        i_n < j < seqlen  (written: out may be
 *                                                                              uninitialised memory)
 *   probs[n, l, j]  = p_j, 0 behind i_n                                        when probs != NULL
 * The probability stays fp32 (the reference rounds alpha to 16 bits before it multiplies).  (Additive, ABI still 11.)
 *   qk           (batch, seqlen, 2, nsenses, d_k) 16-bit, the four element strides of bp_sense_alpha
 *   table, row_index, table_rows   (table_rows, nsenses, d_out) 16-bit and (batch, seqlen) int32 with the strides and the
 *                unsigned clamp of bp_sense_mix_gather: row(b, j) = min(unsigned(row_index[b, j]), table_rows - 1).  A
 *                per-position content tensor is the same call: a (batch * seqlen, nsenses, d_out) table, row = b * seqlen + j
 *   query_sample, query_pos   device int32 (nq), clamped on the device to [0, batch - 1] / [0, seqlen - 1]; the host never
 *                reads them, so one captured launch serves any queries
 *   vec          (nq, nvec, d_out) fp32 (E[w] exactly, or a sum of embedding rows that no 16-bit format holds), element
 *                strides v_query / v_vec (multiples of 4), 16-byte aligned base, last stride 1
 *   out          fp32, element strides o_query / o_vec / o_sense (o_sense >= seqlen, o_vec >= nsenses * o_sense when
 *                nvec > 1, o_query >= nvec * o_vec when nq > 1), unit stride along j
 *   probs        optional fp32, element strides p_query / p_sense (p_sense >= seqlen, p_query >= nsenses * p_sense)
 *   ws           fp32 workspace of `ws_floats` >= bp_sense_attribute_ws_floats(nq, nsenses) elements: the (m, Z) pair of
 *                every (query, sense); contents undefined on entry, it belongs to the call until the stream has run it
 * Two launches (the pairs; the shares), no atomics, every reduction in a fixed order: two calls agree bit for bit.  Keys
 * and table rows behind i_n, and other samples' rows, are never read.
 * Errors, before any launch: BP_ERR_DTYPE; BP_ERR_HEAD_DIM (d_k < 1, d_k % 8 != 0 or d_k > 640); BP_ERR_DOUT (d_out < 1,
 * d_out % 8 != 0 or d_out > 2048); BP_ERR_SHAPE (nq outside 1..65535, nvec outside 1..BP_ATTRIBUTE_MAX_VECS, nsenses outside
 * 1..64, batch, seqlen or table_rows < 1, table_rows > 2^31 - 1, a NULL required pointer, a base that is not 16-byte aligned
 * (qk, table, vec) or 4-byte aligned, a 16-bit stride that is no multiple of 8, an out / probs stride too small for its
 * nesting); BP_ERR_SCALE; BP_ERR_WORKSPACE.
 */
int64_t bp_sense_attribute_ws_floats(int nq, int nsenses);
int bp_sense_attribute(const void *qk, const void *table, const int32_t *row_index, const int32_t *query_sample,
                       const int32_t *query_pos, const float *vec, float *out, float *probs, float *ws, int64_t ws_floats,
                       int batch, int seqlen, int nsenses, int d_k, int d_out, int nq, int nvec, int64_t table_rows,
                       int64_t qk_batch_stride, int64_t qk_row_stride, int64_t qk_two_stride, int64_t qk_sense_stride,
                       int64_t t_row_stride, int64_t t_sense_stride, int64_t idx_batch_stride,
                       int64_t v_query_stride, int64_t v_vec_stride,
                       int64_t o_query_stride, int64_t o_vec_stride, int64_t o_sense_stride,
                       int64_t p_query_stride, int64_t p_sense_stride,
                       float softmax_scale, int dtype, bp_stream_t stream);

/*
 * bp_sense_similarity -- the cosine measures of sense vectors between nq query words and ncand candidate words of the
 * per-token sense table: the lexical-similarity measures of the reference's training/src/run_simlex.py:189-241 and the
 * neighbour scores of training/src/visualize_sim.py:197-222, in ONE pass over the candidates' rows (each is read once per
 * call, whatever nq is).  All arithmetic fp32.  For query n, candidate c, r = row(c):
 *   g[l', l]   = sum_e query[n, l', e] * table[r, l, e]     products of 16-bit elements are exact; fp32 sums in a fixed order
 *   A[l']      = sum_e query[n, l', e]^2,   B[l] = sum_e table[r, l, e]^2                          fixed order
 *   cos[l', l] = g[l', l] / (sqrtf(A[l']) * sqrtf(B[l]))        the order of run_simlex.py:202-208: dot over the outer
 *                                                               product of the norms; correctly rounded sqrtf and /
 *   per_sense[n, l, c] = cos[l, l]                                                  CosSense_l  (:226-229)
 *   min_pair / max_pair[n, c] = min / max over l of cos[l, l]                       MinPair / MaxPair  (:210-216)
 *   min_all / max_all[n, c]   = min / max over all (l', l) of cos[l', l]            MinAll / MaxAll  (:218-224)
 *   flat[n, c] = (sum_l g[l, l]) / (sqrtf(sum_l' A[l']) * sqrtf(sum_l B[l]))        Cos  (:194-200); sums ascending in l
 * A zero vector gives 0 / 0 = NaN as in the reference, and a min / max measure whose set of cosines holds a NaN is NaN (the
 * rule of torch.min / torch.max).  (Additive, ABI still 11.)
 *   table        (table_rows, nsenses, d) fp16 / bf16, element strides t_row / t_sense (multiples of 8), 16-byte aligned
 *                base, last stride 1: the rules of bp_sense_mix_gather.  Only read, and only the candidates' rows.
 *   cand_index   device int32 (ncand), or NULL.  NULL: candidate c is row c (ncand <= table_rows).  Otherwise
 *                row(c) = min(unsigned(cand_index[c]), table_rows - 1); the host never reads it, so one captured launch
 *                serves any candidate list
 *   query        (nq, nsenses, d) in the table's dtype, element strides q_query / q_sense (multiples of 8), 16-byte aligned
 *                base, last stride 1; nq * nsenses <= BP_SIMILARITY_MAX_QUERY_ROWS
 *   flat, min_pair, max_pair, min_all, max_all   fp32 (nq, ncand), ONE element stride o_query >= ncand between queries, unit
 *                stride along the candidates
 *   per_sense    fp32 (nq, nsenses, ncand), element strides ps_query / ps_sense (ps_sense >= ncand, ps_query >= nsenses *
 *                ps_sense when nq > 1), unit stride along the candidates
 *                Any of the six may be NULL (not written); all six NULL is BP_ERR_SHAPE.
 *   nsenses      a power of two, 1 .. 64 (the reference's configurations: 1, 4, 16, 64); any other count is BP_ERR_SHAPE
 * One launch, no workspace, no atomics, every reduction in a fixed order: two calls agree bit for bit.
 * Errors, before any launch: BP_ERR_DTYPE; BP_ERR_DOUT (d < 1, d % 8 != 0 or d > 2048); BP_ERR_SHAPE (nsenses outside 1..64
 * or no power of two, nq < 1, nq * nsenses > BP_SIMILARITY_MAX_QUERY_ROWS, ncand < 0 or > 2^31 - 1, table_rows < 1 or
 * > 2^31 - 1, every output NULL, cand_index NULL with ncand > table_rows, a NULL table / query, a base that is not 16-byte
 * aligned (table, query) or 4-byte aligned, a 16-bit stride that is no multiple of 8, an output stride too small).
 * ncand == 0 is a successful no-op.
 */
int bp_sense_similarity(const void *table, const int32_t *cand_index, const void *query,
                        float *flat, float *min_pair, float *max_pair, float *min_all, float *max_all, float *per_sense,
                        int64_t ncand, int nsenses, int d, int nq, int64_t table_rows,
                        int64_t t_row_stride, int64_t t_sense_stride, int64_t q_query_stride, int64_t q_sense_stride,
                        int64_t o_query_stride, int64_t ps_query_stride, int64_t ps_sense_stride,
                        int dtype, bp_stream_t stream);

/*
 * bp_score_rows -- what an evaluation keeps of a row of logits, in ONE pass over the row: the log-probability and the rank
 * of up to BP_SCORE_MAX_TARGETS target columns, the log-sum-exp, the greedy token and the predictive entropy.  Replaces the
 * torch composition behind the reference's evaluation (training/src/metrics/perplexity.py, accuracy.py, tasks/seq.py; the
 * p(' he') / p(' she') readout of training/src/test_genderbias.py:187-203): an fp32 log_softmax over (tokens, vocab) -- the
 * full-logits tensor at twice its size -- a gather, an argmax, a comparison count and an entropy pass.  bp_xentropy_fwd reads
 * the same bytes and keeps two floats of them.  (Additive, ABI still 11.)
 * Per row, with x_j = float(logits[row, j]), all arithmetic fp32:
 *   lse         = log sum_j exp(x_j), evaluated as m + log sum_j exp(x_j - m), m = max_j x_j
 *   logprob[i]  = x_t - lse                         t = targets[row, i] in [0, cols)
 *   rank[i]     = #{j : x_j > x_t} + #{j < t : x_j == x_t}    0-based, ties towards the lower id; comparisons of the converted
 *                 floats (-0 == +0), so an exact integer.  A NaN compares false both ways: a NaN entry precedes nothing, and
 *                 the rank of a NaN target is 0.
 *   t outside [0, cols) (an ignore_index, as bp_xentropy_fwd treats it): logprob[i] = 0, rank[i] = -1
 *   top1        = the greedy answer of bp_pick_token (do_sample == 0): the lowest index of the maximum, a NaN counting as
 *                 larger than every number (-0 == +0).  On a NaN-free row, rank[i] == 0 <=> top1 == t.
 *   entropy     = lse - (sum_j exp(x_j - m) x_j) / (sum_j exp(x_j - m)); a -inf entry contributes 0 to both sums, not a NaN
 * Degenerate rows follow the arithmetic of the definitions in the extended reals:
 *   a NaN anywhere      lse = entropy = NaN, every logprob NaN
 *   a +inf entry        lse = +inf, entropy = NaN (exp(inf - inf)); logprob = x_t - inf: -inf, or NaN for a +inf target
 *   no finite entry, all -inf   lse = -inf, entropy = NaN; logprob = -inf - -inf = NaN
 * ranks and top1 are defined by comparisons alone and hold on every row.
 *   logits   (rows, cols) fp16 / bf16 / fp32, element stride row_stride >= cols between rows, last stride 1; a row may start
 *            at any element (2- / 4-byte alignment): the elements in front of the first 16-byte boundary and behind the last are
 *            read one by one.  Only read.
 *   targets  int64 (rows, ntargets), element stride target_stride >= ntargets between rows; 1 <= ntargets <=
 *            BP_SCORE_MAX_TARGETS.  Repeated targets are fine.
 *   logprob  fp32 and  rank  int32, (rows, ntargets) with ONE element stride out_stride >= ntargets between rows
 *   lse, entropy  fp32 (rows);  top1  int32 (rows)
 *            Any of the five may be NULL (not written); all five NULL is BP_ERR_SHAPE.
 * One 256-thread workgroup per row, one launch, no workspace, no atomics, every reduction in a fixed order: two calls agree
 * bit for bit.  ntargets == 1 is a kernel of its own.
 * Errors, before any launch: BP_ERR_DTYPE; BP_ERR_SHAPE (rows <= 0 or > 2^31 - 1, cols <= 0 or > 2^31 - 17, row_stride < cols,
 * ntargets outside 1 .. BP_SCORE_MAX_TARGETS, target_stride < ntargets, a NULL logits / targets, every output NULL, out_stride <
 * ntargets with a logprob or rank, logits not aligned to its element, targets not 8-byte or an output not 4-byte aligned).
 */
int bp_score_rows(const void *logits, const int64_t *targets, float *logprob, int32_t *rank, float *lse, int32_t *top1,
                  float *entropy, int64_t rows, int cols, int ntargets, int64_t row_stride, int64_t target_stride,
                  int64_t out_stride, int dtype, bp_stream_t stream);

/*
 * bp_pick_report -- the record of a pick: what the model thought of the token a decode step just chose.  Per row b of logits,
 * with c = counters[b], t = tokens[b * tokens_stride] and x_j = float(logits[b, j]), in ONE launch that reads no host value
 * (legal inside a HIP-graph capture, right behind bp_pick_token* with the same logits, counters and tokens):
 *   c outside [0, rec_cols)   nothing is written for the row -- the pick's rule for `sequences`, so the record of the final,
 *                             dropped pick of a decode loop is dropped with it
 *   lse, logprob[b, c], rank[b, c], entropy[b, c]   exactly bp_score_rows' definitions with the one target t, fp32: logprob =
 *                             x_t - lse, rank = #{x_j > x_t} + #{j < t : x_j == x_t}; t outside [0, vocab) gives logprob 0 and
 *                             rank -1; rows with a NaN, a +inf or nothing but -inf follow the extended reals as described there
 *   top_idx[b, c, i]          the column of position i, 0 <= i < n_top, in the order (x descending as converted floats with
 *                             -0 == +0, a NaN above every number, column ascending): bp_pick_token's greedy order, so
 *                             top_idx[b, c, 0] is the greedy token on every row.  A total order on integers: the answer is
 *                             unique.  On a NaN-free row the element at position i has rank i.
 *   top_logprob[b, c, i]      float(x) - lse of that element: one fp32 subtraction against the lse of this call
 * (The log-probabilities are the model's: of the raw logits, before temperature, penalties and filters.)
 *   logits    (rows, vocab) fp16 / bf16 / fp32, element stride row_stride >= vocab, last stride 1; a row may start at any
 *             element.  Only read.
 *   tokens    int64, element stride tokens_stride >= 1;  counters  int32 (rows)
 *   logprob, entropy  fp32 and  rank  int32: (rows, rec_cols) with ONE element stride rec_stride >= rec_cols between rows
 *   top_idx   int32 and  top_logprob  fp32: (rows, rec_stride, n_top), dense in the last axis
 *             Any of the five may be NULL (not written); all five NULL is BP_ERR_SHAPE.
 *   n_top     0 <= n_top <= min(vocab, BP_PICK_REPORT_MAX_TOP)
 * One 1024-thread workgroup per row, max(1, n_top) passes over the row, no workspace, no atomics, every reduction in a fixed
 * order: two calls agree bit for bit.  (Additive, ABI still 11.)
 * Errors, before any launch: BP_ERR_DTYPE; BP_ERR_SHAPE (rows < 1, vocab < 1 or > 2^31 - 17, row_stride < vocab, tokens_stride
 * < 1, rec_cols < 1, rec_stride < rec_cols, n_top out of range, n_top > 0 with both top pointers NULL, a NULL logits / tokens /
 * counters, every record NULL, logits not aligned to its element, tokens not 8-byte, counters or a record not 4-byte aligned).
 */
int bp_pick_report(const void *logits, const int64_t *tokens, const int32_t *counters, float *logprob, int32_t *rank,
                   float *entropy, int32_t *top_idx, float *top_logprob, int rows, int vocab, int64_t row_stride,
                   int64_t tokens_stride, int rec_cols, int64_t rec_stride, int n_top, int dtype, bp_stream_t stream);

/* ---- dense layers by a pinned hipBLASLt solution (additive, ABI still 11; csrc/bp_gemm.hip, host code) ------------------------------
 *
 *   D[M,N] = A[M,K] . W[N,K]^T (+ bias[N]) (-> tanh-GELU),  row-major 16-bit operands, fp32 accumulation
 *
 * Which algorithm runs is a function of `table` alone.  The row used is the one with the call's dtype, epilogue, N and K and
 * the largest m_min <= M; its `solution` is a hipBLASLt solution index, valid for ONE library version (hipblasLtGetVersion)
 * on ONE architecture ("gfx950"), both stated in the row.  The index is turned into an algorithm, checked against the actual
 * problem and launched on `stream`.  Every other outcome is one of the BP_GEMM_* statuses below (> 0, not an error): NOTHING
 * was launched, D is untouched, and the caller runs the GEMM it would have run without this entry.  The library's heuristic
 * is never consulted by bp_gemm_*.
 *
 * The library is the libhipblaslt the process has already loaded (PyTorch's); this one is never the cause of a second copy
 * (BP_GEMM_NO_LIBRARY when none is loaded).  Handle and a 128 MiB workspace exist once per device from the first call on and
 * are never freed; launches on different streams that need the workspace are ordered by an event.
 *
 *   a, w, d      16-bit matrices with element strides lda >= K, ldw >= K, ldd >= N between rows (d: columns >= N of a wider
 *                buffer are not written)
 *   bias         (N,) in the operands' dtype; non-NULL exactly when epilogue != BP_GEMM_EPILOGUE_NONE
 *   table        n_rows rows, only read; n_rows == 0 is BP_GEMM_MISS
 *   solution_out optional: the index that ran, -1 otherwise
 * Errors: BP_ERR_SHAPE (a NULL operand, M / N / K < 1, a stride below its row, a bias without an epilogue or the reverse, an
 * epilogue out of range), BP_ERR_GEMM.
 */
#define BP_GEMM_EPILOGUE_NONE 0
#define BP_GEMM_EPILOGUE_BIAS 1
#define BP_GEMM_EPILOGUE_BIAS_GELU 2

#define BP_GEMM_MISS 1         /* no row for this (dtype, epilogue, N, K) with m_min <= M, or the row keeps the heuristic   */
#define BP_GEMM_VERSION 2      /* the row was measured with another library version or on another architecture           */
#define BP_GEMM_UNSUPPORTED 3  /* the library does not know the index, or the solution does not take this problem         */
#define BP_GEMM_CAPTURING 4    /* the stream is being captured into a graph                                               */
#define BP_GEMM_NO_LIBRARY 5   /* no libhipblaslt is loaded in this process                                               */

typedef struct {
    int32_t dtype;      /* BP_DTYPE_F16 / BP_DTYPE_BF16 */
    int32_t epilogue;   /* BP_GEMM_EPILOGUE_* */
    int32_t n, k;
    int64_t m_min;      /* the row applies to M >= m_min (>= 1) */
    int32_t version;    /* hipblasLtGetVersion of the library the index was measured with */
    int32_t solution;   /* solution index; < 0: keep the heuristic (BP_GEMM_MISS) */
    char arch[16];      /* "gfx950", NUL-terminated */
} bp_gemm_row;

int bp_gemm_bf16(const void *a, const void *w, const void *bias, void *d, int64_t M, int N, int K,
                 int64_t lda, int64_t ldw, int64_t ldd, int epilogue, const bp_gemm_row *table, int n_rows,
                 int *solution_out, bp_stream_t stream);
int bp_gemm_f16(const void *a, const void *w, const void *bias, void *d, int64_t M, int N, int K,
                int64_t lda, int64_t ldw, int64_t ldd, int epilogue, const bp_gemm_row *table, int n_rows,
                int *solution_out, bp_stream_t stream);
/* Version of the loaded library and the architecture of the current device as the table rows state them. */
int bp_gemm_library(int *version, char *arch, int arch_len);
/* For the tuning tool (scripts/tune_gemm.py) and tests: the solution indices of the heuristic's first `max_solutions`
 * candidates for a problem, best first; *count of them are written.  dtype: BP_DTYPE_F16 / BP_DTYPE_BF16. */
int bp_gemm_heuristic(int dtype, int epilogue, int64_t M, int N, int K, int64_t lda, int64_t ldw, int64_t ldd,
                      int *solutions, int max_solutions, int *count);

#ifdef __cplusplus
}
#endif
#endif /* BP_HIP_H */
