"""numpy restatement of the contracts behind src/utils/sense_vocab.py, shared by test_sense_vocab_host.py,
test_gpu_row_extremes.py and test_gpu_sense_vocab.py.  Written from the contract of bp_row_extremes (include/bp_hip.h) and
from the reference's lines, not from the code under test:

  row_extremes             the row order on RAW bits: a uint64 composite of (ordered key, column), then argsort
  non_contextual_localize  training/src/rank_vocab.py:69-100 in its own order, in float64: per token ld = C(v) @ E^T,
                           ld / ld.max(-1), then @ target; ids clamped to last_token_id and that id skipped (:74, :81-82)
  weights_from_scores      training/src/rank_vocab.py:37-67 with np.quantile
  localize_bound           the first-order error bound of a score, from the inputs alone

No golden file is recorded: the reference's rank_vocab.py cannot be imported where this repository is built (its plotting
imports, matplotlib / seaborn, and its task modules are absent), so the restatement below is what the tests hold on to."""
import numpy as np
import torch


# ---- raw bits ---------------------------------------------------------------------------------------------------------------------

def raw_bits(t):
    """(unsigned raw bits as uint64, key bits) of a torch tensor of fp32 / fp16 / bf16."""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32).astype(np.uint64), 32
    assert t.dtype in (torch.float16, torch.bfloat16), t.dtype
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).astype(np.uint64), 16


def ordered_key(raw, bits):
    """Order-preserving key of raw bits: sign set -> every bit flipped, else the sign bit flipped.  -0 < +0, NaNs at the ends."""
    sign = np.uint64(1 << (bits - 1))
    ones = np.uint64((1 << bits) - 1)
    return np.where(raw & sign != 0, raw ^ ones, raw ^ sign)


def value_of(raw, bits, dtype):
    """float(element) as fp32 from raw bits."""
    if bits == 32:
        return raw.astype(np.uint32).view(np.float32)
    if dtype == torch.bfloat16:
        return (raw.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return raw.astype(np.uint16).view(np.float16).astype(np.float32)


def row_extremes(t, n):
    """(top_val, top_idx, bot_val, bot_idx) of a (rows, cols) torch tensor: fp32 values and int32 columns, (rows, n) each.
    Largest: (key descending, column ascending); smallest: (key ascending, column ascending)."""
    raw, bits = raw_bits(t)
    key = ordered_key(raw, bits)
    col = np.arange(raw.shape[1], dtype=np.uint64)[None, :]
    ones = np.uint64((1 << bits) - 1)
    out = []
    for k in (ones - key, key):
        idx = np.argsort((k << np.uint64(32)) | col, axis=1, kind='stable')[:, :n]
        out += [value_of(np.take_along_axis(raw, idx, 1), bits, t.dtype), idx.astype(np.int32)]
    return tuple(out)


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- rank_vocab.py ----------------------------------------------------------------------------------------------------------------------

def non_contextual_localize(senses, emb, target, last_token_id=50256):
    """senses (V, k, d), emb (V, d), target (V,) float64 -> scores (V, k) float64, in the reference's order."""
    senses, emb, target = (np.asarray(a, dtype=np.float64) for a in (senses, emb, target))
    scores = np.zeros(senses.shape[:2])
    for v in range(senses.shape[0]):
        if v >= last_token_id:          # ids are clamped to last_token_id and that id is skipped
            continue
        ld = senses[v] @ emb.T          # (k, V)
        scores[v] = (ld / ld.max(axis=-1, keepdims=True)) @ target
    return scores


def weights_from_scores(scores, quantile_weights=(1.4, 1.2, 1.0, 0.8)):
    scores = np.asarray(scores, dtype=np.float64)
    q95, q80, q60 = (np.quantile(scores.reshape(-1), q) for q in (.95, .80, .60))
    mult = np.ones_like(scores)
    mult = np.where(q95 < scores, quantile_weights[0], mult)
    mult = np.where((q80 < scores) & (scores < q95), quantile_weights[1], mult)
    mult = np.where((q60 < scores) & (scores < q80), quantile_weights[2], mult)
    mult = np.where(scores < q60, quantile_weights[3], mult)
    return mult


EPS_OUT = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12, torch.float32: 0.0}   # half an ulp of the logits' dtype


def localize_bound(senses, emb, target, dtype):
    """(V, k) float64: the first-order bound on |score - exact| of score = num / mx for logits stored in `dtype`.
      A        = max_j sum_i |c_i| |e_ji|
      d_mx    <= eps_out |m| + (d + 2) 2^-24 A                        (fp32 accumulation, one rounding to `dtype`)
      d_num   <= (d + V_t + 2) 2^-24 sum_i |c_i| |(E^T t)_i|          (V_t non-zero entries of the target)
      d_score <= d_num / |m| + |num| d_mx / m^2
    The tests allow twice this: the factor covers the second-order terms and the division's own rounding."""
    senses, emb, target = (np.asarray(a, dtype=np.float64) for a in (senses, emb, target))
    v, k, d = senses.shape
    c = senses.reshape(v * k, d)
    u = 2.0 ** -24
    m = (c @ emb.T).max(axis=1)
    a = (np.abs(c) @ np.abs(emb).T).max(axis=1)
    w = emb.T @ target
    num = c @ w
    d_mx = EPS_OUT[dtype] * np.abs(m) + (d + 2) * u * a
    d_num = (d + np.count_nonzero(target) + 2) * u * (np.abs(c) @ np.abs(w))
    return (d_num / np.abs(m) + np.abs(num) * d_mx / m ** 2).reshape(v, k)
