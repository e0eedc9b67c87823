"""Sense vectors projected onto the vocabulary -- MI355X-native mirror of the reference's training/src/rank_vocab.py
(`non_contextual_localize` :69-100, `weights_from_scores` :37-67: the `content_weights` of WeightedBackpackLMHeadModel) and of
the data behind training/src/visualize_vocab.py (`visualize_word` :62-82: the sense tables of the paper).

Both read `C_l(v) @ E^T`, the logits a single sense vector gives the whole vocabulary.  The reference walks 50 256 tokens in
Python with a (16, 512, 50264) block per chunk and a full sort per sense.  Here the sense vectors of every token come from
`BackpackModel.sense_table()`, the product runs chunk by chunk as one GEMM into ONE reused block (`_project_rows`), and each
block is reduced to the two ends of its rows by bp_row_extremes (csrc/row_extremes.hip) before the next chunk overwrites
it: the (V k, V) matrix never exists.  CPU tensors, and shapes the kernel does not take, go through `_eager_row_extremes`,
which states the same contract in torch ops, bit for bit.

Everything runs under torch.no_grad() and takes a BackpackLMHeadModel on any device."""
from dataclasses import dataclass

import torch

import bp_hip

DEFAULT_CHUNK_ROWS = 8192   # 512 tokens x 16 senses, the reference's chunk (rank_vocab.py:72-73): 0.8 GB of bf16 logits at Small


def _ordered_keys(x):
    """The order-preserving integer key of every element's raw bits (csrc/vocab_row.h, RowElem::key) as non-negative
    integers: sign bit set -> all bits flipped, else the sign bit flipped."""
    if x.dtype == torch.float32:
        raw = x.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
        return raw ^ torch.where(raw >= 0x80000000, 0xffffffff, 0x80000000)
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError(f'row extremes: fp16, bf16 or fp32 rows, got {x.dtype}')
    raw = x.contiguous().view(torch.int16).to(torch.int32) & 0xffff
    return raw ^ torch.where(raw >= 0x8000, 0xffff, 0x8000)


def _eager_row_extremes(logits, n, largest=True, smallest=True):
    """The contract of bp_row_extremes (include/bp_hip.h) in torch ops, for tensors the kernel does not take (CPU): a
    STABLE sort on the integer keys, so equal keys keep ascending columns at either end.  Returns what bp_hip.row_extremes
    returns: (top_val, top_idx, bot_val, bot_idx), fp32 / int32 (rows, n), None for an end not asked for."""
    n = int(n)
    if logits.dim() != 2 or not 1 <= n <= min(logits.shape[1], bp_hip.ROW_EXTREMES_MAX_N):
        raise RuntimeError(f'row extremes: (rows, cols) logits and 1 <= n <= min(cols, {bp_hip.ROW_EXTREMES_MAX_N})')
    keys = _ordered_keys(logits)
    out = []
    for wanted, k in ((largest, -keys), (smallest, keys)):
        if not wanted:
            out += [None, None]
            continue
        idx = torch.sort(k, dim=1, stable=True).indices[:, :n]
        out += [torch.gather(logits, 1, idx).float(), idx.to(torch.int32)]
    return tuple(out)


def _row_extremes(block, n, largest, smallest, out=None):
    """bp_row_extremes on the HIP path, its torch twin elsewhere; `out`: four (rows, n) views to fill, or None."""
    if bp_hip.row_extremes_supported(block, n):
        return bp_hip.row_extremes(block, n, largest=largest, smallest=smallest, out=out)
    res = _eager_row_extremes(block, n, largest=largest, smallest=smallest)
    if out is None:
        return res
    for o, v in zip(out, res):
        if v is not None:
            o.copy_(v)
    return tuple(o if v is not None else None for o, v in zip(out, res))


def _content_rows(model, token_ids):
    """(T k, d): the sense vectors of `token_ids` (T,) as rows, token-major, from the content network."""
    senses = model.transformer.content_model(token_ids.reshape(1, -1))[0]          # (k, T, d)
    return senses.transpose(0, 1).reshape(-1, senses.shape[-1])


@torch.no_grad()
def _project_rows(model, senses, chunk_rows=DEFAULT_CHUNK_ROWS, n=1, largest=True, smallest=False, dot=None, tokens=None,
                  debug_blocks=False):
    """The shared driver: rows `senses` (R, d) times `lm_head.weight^T`, chunk by chunk into one reused (chunk_rows, V)
    block of the model's dtype (a dense product: it stays on the BLAS library), one row_extremes call per chunk.

    senses   (R, d) rows in the dtype of lm_head.weight; None: the sense vectors of tokens 0 .. `tokens` - 1 (all k of a
             token are consecutive rows) straight from the content network, a chunk of tokens at a time
    dot      optional (d,) fp32: also returns `num` (R,) fp32 = rows.float() @ dot, a chunk at a time
    Returns a dict: top_val / top_idx / bot_val / bot_idx ((R, n) fp32 / int32, None for an end not asked for), num, and
    with `debug_blocks` a list `blocks` of clones of every logits block as row_extremes saw it (tests)."""
    weight = model.lm_head.weight
    vocab_rows, d = weight.shape
    k = model.transformer.num_content_vectors
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError('chunk_rows must be positive')
    if senses is None:
        total = int(tokens) * k
        per_chunk = max(1, chunk_rows // k) * k            # whole tokens per chunk
    else:
        if senses.dim() != 2 or senses.shape[1] != d:
            raise ValueError(f'senses must be (rows, {d}), got {tuple(senses.shape)}')
        total, per_chunk = senses.shape[0], chunk_rows
    per_chunk = max(1, min(per_chunk, total))
    dev = weight.device
    out = [torch.empty((total, n), dtype=dt, device=dev) if wanted else None
           for wanted, dt in ((largest, torch.float32), (largest, torch.int32), (smallest, torch.float32), (smallest, torch.int32))]
    num = torch.empty((total,), dtype=torch.float32, device=dev) if dot is not None else None
    block = torch.empty((per_chunk, vocab_rows), dtype=weight.dtype, device=dev)
    blocks = []
    for r0 in range(0, total, per_chunk):
        r1 = min(total, r0 + per_chunk)
        if senses is None:
            rows = _content_rows(model, torch.arange(r0 // k, r1 // k, device=dev))
        else:
            rows = senses[r0:r1]
        rows = rows.to(weight.dtype)
        view = block[:r1 - r0]
        torch.matmul(rows, weight.t(), out=view)
        _row_extremes(view, n, largest, smallest, out=[o[r0:r1] if o is not None else None for o in out])
        if num is not None:
            torch.mv(rows.float(), dot, out=num[r0:r1])
        if debug_blocks:
            blocks.append(view.clone())
    res = dict(zip(('top_val', 'top_idx', 'bot_val', 'bot_idx'), out), num=num)
    if debug_blocks:
        res['blocks'] = blocks
    return res


def _table_rows(model):
    """The whole-vocabulary sense table as (V k, d) rows, or None when the model cannot serve it."""
    table = model.transformer.sense_table()
    return None if table is None else table.reshape(-1, table.shape[-1])


@dataclass
class SenseExtremes:
    """What `sense_extremes` returns: (T, k, count) each; ids int64, logits fp32; largest / smallest first."""
    top_ids: torch.Tensor
    top_logits: torch.Tensor
    bottom_ids: torch.Tensor
    bottom_logits: torch.Tensor


@torch.no_grad()
def sense_extremes(model, token_ids=None, count=20, contents=None, chunk_rows=DEFAULT_CHUNK_ROWS, _debug_blocks=False):
    """The `count` largest and smallest vocabulary logits of every sense vector: the data `visualize_word` prints
    (visualize_vocab.py:62-82, which sorts `contents[i] @ lm_head.weight.t()` and reads both ends).

    token_ids  the tokens to look up (a sequence or tensor of ids); None: the whole vocabulary, row v = token v
    contents   (k, d) or (T, k, d) sense vectors to use INSTEAD of a lookup -- word arithmetic and `mogrify_word` of the
               reference pass edited vectors this way
    Equal logits are listed by ascending id at both ends (the contract of bp_row_extremes).  `_debug_blocks` (tests): returns
    (result, the list of logits blocks the result was read from)."""
    weight = model.lm_head.weight
    k = model.transformer.num_content_vectors
    senses, tokens = None, None
    if contents is not None:
        contents = torch.as_tensor(contents, device=weight.device)
        if contents.dim() == 2:
            contents = contents.unsqueeze(0)
        if contents.dim() != 3 or contents.shape[2] != weight.shape[1]:
            raise ValueError(f'contents must be (k, d) or (T, k, d) with d = {weight.shape[1]}')
        k = contents.shape[1]
        senses = contents.reshape(-1, contents.shape[2]).to(weight.dtype)
    else:
        table = _table_rows(model)
        if token_ids is not None:
            ids = torch.as_tensor(token_ids, device=weight.device).reshape(-1).long()
            senses = table.view(-1, k, table.shape[1])[ids].reshape(-1, table.shape[1]) if table is not None \
                else _content_rows(model, ids)
        elif table is not None:
            senses = table
        else:
            tokens = weight.shape[0]
    res = _project_rows(model, senses, chunk_rows, n=int(count), largest=True, smallest=True, tokens=tokens,
                        debug_blocks=_debug_blocks)
    shape = (-1, k, int(count))
    result = SenseExtremes(top_ids=res['top_idx'].long().view(shape), top_logits=res['top_val'].view(shape),
                           bottom_ids=res['bot_idx'].long().view(shape), bottom_logits=res['bot_val'].view(shape))
    return (result, res['blocks']) if _debug_blocks else result


def format_sense_extremes(result, tokenizer=None, token_ids=None):
    """The text `visualize_word` prints for a SenseExtremes (visualize_vocab.py:72-81), one block per token and sense;
    without a tokenizer the ids themselves are printed."""
    decode = (lambda i: tokenizer.decode(i)) if tokenizer is not None else str
    lines = []
    for t in range(result.top_ids.shape[0]):
        if token_ids is not None:
            lines.append(decode(int(token_ids[t])))
        for sense in range(result.top_ids.shape[1]):
            lines.append('~~~~~~~~~~~~~~~~~~~~~~~{}~~~~~~~~~~~~~~~~~~~~~~~~'.format(sense))
            for title, ids, logits in (('~~~Positive~~~', result.top_ids, result.top_logits),
                                       ('~~~Negative~~~', result.bottom_ids, result.bottom_logits)):
                lines.append(title)
                for j in range(ids.shape[2]):
                    lines.append('{} \t {:.2f}'.format(decode(int(ids[t, sense, j])), float(logits[t, sense, j])))
    return '\n'.join(lines)


@torch.no_grad()
def non_contextual_localize(target_vector, model, nv=None, vocsize=None, tokenizer=None, verbose=False, last_token_id=50256,
                            chunk_rows=DEFAULT_CHUNK_ROWS):
    """scores (vocsize, nv) fp32: score[v, l] = (ld / max(ld)) @ target_vector with ld = C_l(v) @ E^T, zero for tokens
    v >= last_token_id (rank_vocab.py:69-100 clamps its ids to 50256 and skips that id).

    The sum over the vocabulary commutes with the division by the row's maximum, so the score is num / mx with
      mx   the row maximum of the logits block: bp_row_extremes with n = 1, largest only
      num  C_l(v) . (E^T target_vector), one fp32 GEMV that needs no pass over the logits
    (the reference divides every logit, then sums: another rounding order, the same mathematics).  `nv` and `vocsize`
    default to the model's and must match it."""
    weight = model.lm_head.weight
    k = model.transformer.num_content_vectors
    vocab_rows = weight.shape[0]
    nv = k if nv is None else int(nv)
    vocsize = vocab_rows if vocsize is None else int(vocsize)
    if nv != k:
        raise ValueError(f'nv = {nv}, but the model has {k} sense vectors per token')
    if vocsize != vocab_rows:
        raise ValueError(f'vocsize = {vocsize}, but the model\'s lm_head has {vocab_rows} vocabulary rows')
    target = torch.as_tensor(target_vector, device=weight.device).reshape(-1).float()
    if target.numel() != vocab_rows:
        raise ValueError(f'target_vector must have {vocab_rows} entries, got {target.numel()}')
    live = max(0, min(int(last_token_id), vocsize))
    scores = torch.zeros((vocsize, nv), dtype=torch.float32, device=weight.device)
    if live > 0:
        # E^T target in fp32, a chunk of vocabulary rows at a time (no fp32 copy of the embedding)
        dot = torch.zeros((weight.shape[1],), dtype=torch.float32, device=weight.device)
        step = max(1, int(chunk_rows))
        for v0 in range(0, vocab_rows, step):
            dot.addmv_(weight[v0:v0 + step].float().t(), target[v0:v0 + step])
        table = _table_rows(model)
        res = _project_rows(model, None if table is None else table[:live * k], chunk_rows, n=1, largest=True,
                            smallest=False, dot=dot, tokens=live)
        scores[:live] = (res['num'] / res['top_val'][:, 0]).view(live, nv)
    if verbose:
        sorted_plus, plus_indices = torch.sort(scores.reshape(-1), descending=True)
        for i in range(min(100, plus_indices.numel())):
            word, vec = int(plus_indices[i]) // nv, int(plus_indices[i]) % nv
            print(tokenizer.decode(word) if tokenizer is not None else word, vec, float(sorted_plus[i]))
    return scores


def weights_from_scores(scores, quantile_weights=(1.4, 1.2, 1.0, 0.8), verbose=False):
    """Per-(token, sense) multipliers from localisation scores by quantile, statement for statement rank_vocab.py:37-67
    (its prints behind `verbose`): above the 95 % quantile -> w[0], strictly between 80 % and 95 % -> w[1], strictly between
    60 % and 80 % -> w[2], below 60 % -> w[3]; a score equal to a quantile keeps 1."""
    flat = scores.reshape(-1)
    if verbose:
        print('q', torch.quantile(flat, q=torch.tensor([.95, .8, .6], device=scores.device)))
    quantile_95 = torch.quantile(flat, q=torch.tensor([.95], device=scores.device))
    quantile_80 = torch.quantile(flat, q=torch.tensor([.80], device=scores.device))
    quantile_60 = torch.quantile(flat, q=torch.tensor([.60], device=scores.device))
    multiplier = torch.ones_like(scores)
    multiplier = torch.where(quantile_95 < scores, quantile_weights[0], multiplier)
    multiplier = torch.where(torch.logical_and(quantile_80 < scores, scores < quantile_95), quantile_weights[1], multiplier)
    multiplier = torch.where(torch.logical_and(quantile_60 < scores, scores < quantile_80), quantile_weights[2], multiplier)
    multiplier = torch.where(scores < quantile_60, quantile_weights[3], multiplier)
    if verbose:
        print('q', torch.quantile(multiplier.reshape(-1), q=torch.tensor([.95, .8, .6], device=scores.device)))
    return multiplier
