"""float64 numpy restatement of the contract of bp_sense_attribute (include/bp_hip.h) and of the two statistics of
src/utils/sense_attribution.contextual_localize, written from the formulas -- test infrastructure shared by
test_sense_attribution_host.py and test_gpu_sense_attribute.py.  Nothing here needs a device or the built library."""
import numpy as np
import torch


def f64(t):
    """A torch tensor (any dtype / device) or array as a float64 numpy array."""
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def bits_of(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.int32)


def clamp_queries(query_sample, query_pos, batch, seqlen):
    b = np.clip(np.asarray(query_sample, dtype=np.int64), 0, batch - 1)
    i = np.clip(np.asarray(query_pos, dtype=np.int64), 0, seqlen - 1)
    return b, i


def clamp_rows(row_index, table_rows):
    """row(b, j): the index as an unsigned 32-bit value, at most the last row."""
    r = np.asarray(row_index, dtype=np.int64) & 0xffffffff
    return np.minimum(r, table_rows - 1)


def sense_attribute(qk, table, row_index, query_sample, query_pos, vec, scale):
    """qk (B, S, 2, k, d_k), table (rows, k, d), row_index (B, S), vec (nq, nvec, d) -> (out (nq, nvec, k, S), probs
    (nq, k, S), unit (nq, nvec, k, S)) in float64; unit = p_j * sum_c |row_c| |vec_c|, the scale of an entry's rounding
    errors.  Only keys and rows 0 .. i_n of sample b_n are touched."""
    qk, vec = f64(qk), f64(vec)
    table = torch.as_tensor(table)                                             # (only the rows a query names become float64)
    batch, seqlen, _, k, _ = qk.shape
    nq, nvec, _ = vec.shape
    b, i = clamp_queries(query_sample, query_pos, batch, seqlen)
    rows = clamp_rows(row_index, table.shape[0])
    out = np.zeros((nq, nvec, k, seqlen))
    unit = np.zeros((nq, nvec, k, seqlen))
    probs = np.zeros((nq, k, seqlen))
    for n in range(nq):
        m = i[n] + 1
        s = float(scale) * np.einsum('lc,jlc->lj', qk[b[n], i[n], 0], qk[b[n], :m, 1])
        e = np.exp(s - s.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)                                   # (k, m)
        content = f64(table[torch.as_tensor(rows[b[n], :m], device=table.device)])   # (m, k, d)
        probs[n, :, :m] = p
        out[n, :, :, :m] = p[None] * np.einsum('jlc,vc->vlj', content, vec[n])
        unit[n, :, :, :m] = p[None] * np.einsum('jlc,vc->vlj', np.abs(content), np.abs(vec[n]))
    return out, probs, unit


def fp32_factor(qk, query_sample, query_pos, scale, d_out, extra=0):
    """First-order bound, in units of p_j sum_c |row_c| |vec_c|, on the error of ANY fp32 evaluation of the contract with
    exact 16-bit-or-fp32 operands (u = 2^-24, every sum of n terms in any order: n u relative to its absolute sum):
      the score     |ds| <= (d_k + 2) u A,  A = scale max_j sum_c |q_c| |k_c|   (d_k products, the scale, one subtraction)
      the weight    p (1 + 2 |ds| + (S + 4) u)    (numerator and normaliser both carry ds; exp, the sum of <= S terms, the division)
      the dot       (d_out + 1) u of its unit; the final product u
    `extra`: further terms a caller's own sums add (the fp32 sum of the vocabulary's embedding rows)."""
    qk = f64(qk)
    batch, seqlen, _, _, dk = qk.shape
    b, i = clamp_queries(query_sample, query_pos, batch, seqlen)
    a = 0.0
    for n in range(len(b)):
        a = max(a, float(scale) * np.einsum('lc,jlc->lj', np.abs(qk[b[n], i[n], 0]), np.abs(qk[b[n], :i[n] + 1, 1])).max())
    return (2 * (dk + 2) * a + seqlen + 4 + d_out + 2 + extra) * 2.0 ** -24


def contextual_localize(contexts, target_id, qk_of, senses, emb, scale):
    """(plus, minus, plus_unit, minus_unit) float64 (vocab rows, k): `qk_of(context)` gives the (S, 2, k, d_k) projection of
    one context alone, `senses` (vocab rows, k, d) the sense vectors of every word, `emb` (vocab rows, d) the LM head.  The
    units are the same sums over absolute values (p_j sum_c |C_c| sum_v |E[v]_c|)."""
    senses, emb = f64(senses), f64(emb)
    plus = np.zeros(senses.shape[:2])
    minus = np.zeros(senses.shape[:2])
    plus_unit = np.zeros(senses.shape[:2])
    minus_unit = np.zeros(senses.shape[:2])
    for ctx in contexts:
        ctx = np.asarray(ctx, dtype=np.int64)
        i = len(ctx) - 2
        qk = f64(qk_of(ctx))
        s = float(scale) * np.einsum('lc,jlc->lj', qk[i, 0], qk[:i + 1, 1])
        e = np.exp(s - s.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)                                   # (k, i + 1)
        logits = np.einsum('jlc,vc->jlv', senses[ctx[:i + 1]], emb)            # (i + 1, k, V): the reference's own route
        weighted = logits * p.T[:, :, None]
        pos = weighted[:, :, target_id]
        neg = weighted.sum(axis=2) - pos
        mass = np.einsum('jlc,vc->jlv', np.abs(senses[ctx[:i + 1]]), np.abs(emb)) * p.T[:, :, None]
        for j in range(i + 1):
            plus[ctx[j]] += pos[j]
            minus[ctx[j]] += neg[j]
            plus_unit[ctx[j]] += mass[j, :, target_id]
            minus_unit[ctx[j]] += mass[j].sum(axis=1) - mass[j, :, target_id]
    return plus, minus, plus_unit, minus_unit


def top_contributions(contributions, count):
    """Stable sorts of every (k S) row: (top_pos, top_sense, top_val, bot_pos, bot_sense, bot_val), (N, M, count) each;
    equal values keep ascending (sense, position) at either end.  (Numeric order: the test rows hold no signed zeros.)"""
    c = np.asarray(contributions, dtype=np.float32)
    n, m, k, s = c.shape
    flat = c.reshape(n * m, k * s)
    top = np.argsort(-flat.astype(np.float64), axis=1, kind='stable')[:, :count]
    bot = np.argsort(flat.astype(np.float64), axis=1, kind='stable')[:, :count]
    shape = (n, m, count)
    return ((top % s).reshape(shape), (top // s).reshape(shape), np.take_along_axis(flat, top, 1).reshape(shape),
            (bot % s).reshape(shape), (bot // s).reshape(shape), np.take_along_axis(flat, bot, 1).reshape(shape))
