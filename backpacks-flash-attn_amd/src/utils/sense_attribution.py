"""Which word, through which sense, produced this prediction -- the contextual half of the reference's sense analysis
(training/src/localize_pred.py:25-65), MI355X-native.

BackpackLMHeadModel.forward puts nothing between the combination of the senses and the tied LM head (no final norm, no
bias), so for every position i and word w
    logit_i[w] = sum_l sum_{j<=i} alpha^l_ij * < C_l(x_j), E[w] >
holds exactly, and the summand is the share of sense l of context word j in the prediction of w.  The reference multiplies
the whole content tensor with the LM head into (B, k, S, vocab), builds the full (B, k, S, S) alpha, and reads one row and
one column of each.  Here one bp_sense_attribute call (csrc/sense_attribute.hip) forms the (k, S) shares of a query
straight from the qk projection and the sense table: nothing of size k S^2, S k d or vocab exists.  CPU tensors, and models
without the fused senses, go through `_eager_sense_attribute`, which states the same contract in fp32 torch ops.

Everything runs under torch.no_grad() and takes a BackpackLMHeadModel on any device."""
from dataclasses import dataclass
from typing import Optional

import torch

import bp_hip
from src.utils.sense_vocab import _row_extremes


def _eager_sense_attribute(qk, table, row_index, query_sample, query_pos, vec, scale, want_probs=False):
    """The contract of bp_sense_attribute (include/bp_hip.h) in fp32 torch ops, for tensors the kernel does not take: returns
    what bp_hip.sense_attribute returns, (out (nq, nvec, k, S) fp32, probs (nq, k, S) fp32 or None).  The queries are clamped
    to the batch and the sequence, the row index as an unsigned value to the table; nothing behind a query's position
    reaches its result."""
    batch, seqlen = qk.shape[:2]
    b = query_sample.long().clamp(0, batch - 1)
    i = query_pos.long().clamp(0, seqlen - 1)
    visible = torch.arange(seqlen, device=qk.device)[None, :] <= i[:, None]                     # (nq, S)
    q = qk[b, i, 0].float()                                                                     # (nq, k, d_k)
    keys = qk[b, :, 1].float()                                                                  # (nq, S, k, d_k)
    s = float(scale) * torch.einsum('nld,nsld->nls', q, torch.where(visible[:, :, None, None], keys, 0.0))
    s = s.masked_fill(~visible[:, None, :], float('-inf'))
    e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    p = e / e.sum(dim=-1, keepdim=True)                                                         # (nq, k, S), 0 behind i
    rows = torch.minimum(row_index[b].long() & 0xffffffff, torch.tensor(table.shape[0] - 1, device=qk.device))
    content = torch.where(visible[:, :, None, None], table[rows].float(), 0.0)                  # (nq, S, k, d)
    out = p[:, None] * torch.einsum('nsld,nvd->nvls', content, vec.float())
    return out, (p if want_probs else None)


@dataclass
class SenseContributions:
    """What `sense_contributions` returns, N queries with M vectors each.
    contributions (N, M, k, S) fp32: the share of sense l of position j, exact zeros behind the query's position
    logits        (N, M) fp32: their sum over (k, S) -- the model's logit when the vector is a row of lm_head.weight
    probs         (N, k, S) fp32 sense weights alpha^l_ij of the query's row, or None
    samples, positions   (N,) int64: the queries"""
    contributions: torch.Tensor
    logits: torch.Tensor
    probs: Optional[torch.Tensor]
    samples: torch.Tensor
    positions: torch.Tensor


def _queries(positions, batch, device):
    """(samples, positions) int64 (N,) each from a (B,) list / tensor of positions or a list of (sample, position) pairs."""
    pos = torch.as_tensor(positions, device=device).long()
    if pos.dim() == 1:
        if pos.shape[0] != batch:
            raise ValueError(f'positions must hold one position per sample ({batch}) or (sample, position) pairs')
        return torch.arange(batch, device=device), pos
    if pos.dim() != 2 or pos.shape[1] != 2:
        raise ValueError('positions must be (B,) or a list of (sample, position) pairs')
    return pos[:, 0].contiguous(), pos[:, 1].contiguous()


def _rows_and_index(model, input_ids):
    """(table (rows, k, d), index (B, S)): the whole-vocabulary sense table when the model serves one, else the table of
    this batch's distinct tokens."""
    table = model.transformer.sense_table()
    if table is not None:
        return table, input_ids
    return model.transformer._table_of_unique_tokens(input_ids)


def _attribute(model, qk, table, index, samples, positions, vectors, want_probs):
    scale = model.transformer.contextualization_attn.scale()
    nq, nvec = vectors.shape[:2]
    if not (qk.is_cuda and model.transformer.fused_senses):
        return _eager_sense_attribute(qk, table, index, samples, positions, vectors, scale, want_probs)
    # the kernel holds up to four vectors of a query in registers: more of them are further calls into views of one result
    k, seqlen = qk.shape[3], qk.shape[1]
    out = torch.empty((nq, nvec, k, seqlen), dtype=torch.float32, device=qk.device)
    probs = None
    index, samples, positions = index.to(torch.int32), samples.to(torch.int32), positions.to(torch.int32)
    for v0 in range(0, nvec, bp_hip.ATTRIBUTE_MAX_VECS):
        v1 = min(nvec, v0 + bp_hip.ATTRIBUTE_MAX_VECS)
        _, pr = bp_hip.sense_attribute(qk, table, index, samples, positions, vectors[:, v0:v1].contiguous(), scale,
                                       want_probs=want_probs and v0 == 0, out=out[:, v0:v1])
        probs = pr if v0 == 0 else probs
    return out, probs


@torch.no_grad()
def sense_contributions(model, input_ids, positions, target_ids=None, vectors=None, return_probs=False):
    """The (sense, position) shares of logits: contributions[n, m, l, j] = alpha^l_ij <C_l(x_j), vectors[n, m]> for query
    n = (sample b, position i).

    input_ids    (B, S) ids on the model's device.  Right-padded batches need nothing special: the sense weights are
                 causal, so the pads behind a row's last token reach no query inside the row (a query placed ON a pad
                 sees the pads in front of it, as the model's own forward does)
    positions    (B,) -- one position per sample, in order -- or a list of (sample, position) pairs: the N queries
    target_ids   (N,) or (N, M) word ids: vectors = lm_head.weight[target_ids] in fp32, and `logits` are the model's logits
    vectors      (N, M, d) fp32, INSTEAD of target_ids: any directions, e.g. a sum of embedding rows
    return_probs also the (N, k, S) sense weights of every query's row
    One pass through the trunk, one bp_sense_attribute call per four vectors (M <= 4: one call).  Returns a
    SenseContributions."""
    weight = model.lm_head.weight
    input_ids = torch.as_tensor(input_ids, device=weight.device).long()
    if input_ids.dim() != 2:
        raise ValueError('input_ids must be (B, S)')
    samples, pos = _queries(positions, input_ids.shape[0], weight.device)
    if (samples < 0).any() or (samples >= input_ids.shape[0]).any() or (pos < 0).any() or (pos >= input_ids.shape[1]).any():
        raise ValueError('a query lies outside the batch or the sequence')
    if (target_ids is None) == (vectors is None):
        raise ValueError('give target_ids or vectors (one of them)')
    if vectors is None:
        ids = torch.as_tensor(target_ids, device=weight.device).long()
        ids = ids[:, None] if ids.dim() == 1 else ids
        if ids.dim() != 2 or ids.shape[0] != samples.shape[0]:
            raise ValueError(f'target_ids must be (N,) or (N, M) with N = {samples.shape[0]} queries')
        vectors = weight[ids].float()
    else:
        vectors = torch.as_tensor(vectors, device=weight.device).float()
        if vectors.dim() != 3 or vectors.shape[0] != samples.shape[0] or vectors.shape[2] != weight.shape[1]:
            raise ValueError(f'vectors must be (N, M, {weight.shape[1]}) with N = {samples.shape[0]} queries')
    tr = model.transformer
    hidden = tr.gpt2_model(input_ids)
    qk = tr.contextualization_attn.project(hidden)
    table, index = _rows_and_index(model, input_ids)
    out, probs = _attribute(model, qk, table, index, samples, pos, vectors.contiguous(), return_probs)
    return SenseContributions(contributions=out, logits=out.sum(dim=(2, 3)), probs=probs, samples=samples, positions=pos)


@torch.no_grad()
def contextual_localize(model, contexts, target_id):
    """(plus, minus), each (vocab rows, k) fp32: the statistics of the reference's `localize` (localize_pred.py:25-58).  For
    every context (a sequence of at least two ids) the query is the position in front of its last token, the one that
    predicts it; the share of sense l of context token x_j (j up to the query) in the logit of `target_id` is added to
    plus[x_j, l], its share in the logits of EVERY OTHER word, summed, to minus[x_j, l].

    The second term is linear in the embedding: sum_{v != target} <C, E[v]> = <C, sum_v E[v] - E[target]>, so both come
    from one call with two fp32 vectors per query and no pass over the vocabulary.  The contexts are right-padded into one
    batch (causality hides the pads); the sums over the contexts run in float64 (`index_add_`)."""
    weight = model.lm_head.weight
    contexts = [torch.as_tensor(c).reshape(-1).long() for c in contexts]
    if not contexts or min(c.numel() for c in contexts) < 2:
        raise ValueError('every context needs at least two ids: the last one is the word being predicted')
    lengths = torch.tensor([c.numel() for c in contexts], device=weight.device)
    ids = torch.nn.utils.rnn.pad_sequence(contexts, batch_first=True, padding_value=0).to(weight.device)
    k = model.transformer.num_content_vectors
    target = weight[int(target_id)].float()
    total = torch.zeros_like(target)
    for v0 in range(0, weight.shape[0], 8192):             # sum_v E[v] in fp32, no fp32 copy of the embedding
        total += weight[v0:v0 + 8192].float().sum(dim=0)
    vectors = torch.stack([target, total - target]).expand(len(contexts), 2, -1)
    res = sense_contributions(model, ids, lengths - 2, vectors=vectors)
    stats = torch.zeros((2, weight.shape[0], k), dtype=torch.float64, device=weight.device)
    counted = torch.arange(ids.shape[1], device=weight.device)[None, :] <= (lengths - 2)[:, None]        # (B, S)
    shares = res.contributions.permute(1, 0, 3, 2)[:, counted].double()                                   # (2, tokens, k)
    stats.index_add_(1, ids[counted], shares)
    return stats[0].float(), stats[1].float()


@dataclass
class TopContributions:
    """What `top_contributions` returns: (N, M, count) each; positions / senses int64, values fp32; largest / smallest
    first, equal values by ascending (sense, position)."""
    top_positions: torch.Tensor
    top_senses: torch.Tensor
    top_values: torch.Tensor
    bottom_positions: torch.Tensor
    bottom_senses: torch.Tensor
    bottom_values: torch.Tensor


@torch.no_grad()
def top_contributions(result, count=10):
    """The `count` (<= 64) largest and smallest shares of every (query, vector) of a SenseContributions, as (position,
    sense, value): bp_row_extremes on the (N M, k S) view of `contributions` on the GPU, its torch twin elsewhere."""
    c = result.contributions.contiguous()
    n, m, k, s = c.shape
    count = int(count)
    if not 1 <= count <= min(k * s, bp_hip.ROW_EXTREMES_MAX_N):
        raise ValueError(f'count must be in 1 .. min(k S, {bp_hip.ROW_EXTREMES_MAX_N})')
    tv, ti, bv, bi = _row_extremes(c.view(n * m, k * s), count, True, True)
    shape = (n, m, count)
    ti, bi = ti.long().view(shape), bi.long().view(shape)
    return TopContributions(top_positions=ti % s, top_senses=ti // s, top_values=tv.view(shape),
                            bottom_positions=bi % s, bottom_senses=bi // s, bottom_values=bv.view(shape))


def format_contributions(top, input_ids=None, samples=None, tokenizer=None):
    """Text for a TopContributions, one block per (query, vector).  With `input_ids` (B, S) and the queries' `samples`
    (SenseContributions.samples) every position is printed with its token -- decoded when a tokenizer is given, the id
    otherwise."""
    decode = (lambda i: tokenizer.decode(i)) if tokenizer is not None else str
    lines = []
    for n in range(top.top_values.shape[0]):
        for m in range(top.top_values.shape[1]):
            lines.append('~~~~~~~~~~~~~~~~~~~~~~~query {} vector {}~~~~~~~~~~~~~~~~~~~~~~~~'.format(n, m))
            for title, pos, sense, val in (('~~~Positive~~~', top.top_positions, top.top_senses, top.top_values),
                                           ('~~~Negative~~~', top.bottom_positions, top.bottom_senses, top.bottom_values)):
                lines.append(title)
                for c in range(val.shape[2]):
                    j = int(pos[n, m, c])
                    word = '' if input_ids is None else decode(int(input_ids[int(samples[n]) if samples is not None else n, j])) + ' \t '
                    lines.append('{}position {} sense {} \t {:.4f}'.format(word, j, int(sense[n, m, c]), float(val[n, m, c])))
    return '\n'.join(lines)
