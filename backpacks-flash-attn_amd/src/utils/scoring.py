"""Scoring text with a (Backpack) LM head model: per-token log-probability, rank of the gold token, greedy token and
predictive entropy, and what the paper's evaluations build from them -- perplexity and top-1 accuracy
(training/src/metrics/perplexity.py, accuracy.py, tasks/seq.py), the LAMBADA last-word protocol, minimal pairs, multiple
choice, and the p(' he') / p(' she') bias ratio of training/src/test_genderbias.py:187-203.

The reference takes `torch.log_softmax` (or `softmax`) of the full (B, S, vocab) logits for each of these.  Here the LM head
runs over the rows that are scored only, in blocks, and every block of logits is reduced by ONE pass of bp_score_rows
(csrc/score_rows.hip, contract in include/bp_hip.h) to five small arrays: peak memory is one block of logits (the idea of
src/utils/perplexity.py:lm_loss_chunked), and padded positions cost no head work.

Models: BackpackLMHeadModel, the GPTLMHeadModel mirror (`transformer`, `lm_head`) and the sense-intervened wrappers of
src/models/intervened_models.py (`_mixed`, `backpack_network.lm_head`).  A model built with `use_flash_attn=False`, or one on
the CPU, takes `_eager_score_rows`, the torch twin of the kernel's contract.
"""
import math
from collections import namedtuple

import torch

import bp_hip
from src.utils.packing import pack_sequences

TokenScores = namedtuple('TokenScores', ['logprobs', 'ranks', 'top1', 'entropy', 'lse', 'mask'])
SequenceScores = namedtuple('SequenceScores', ['logprob', 'count', 'all_top1'])
GenerationScores = namedtuple('GenerationScores', ['logprob', 'count', 'perplexity'])

SCORE_OUTPUTS = bp_hip.SCORE_OUTPUTS
HEAD_BLOCK_ROWS = 2048       # rows of one LM-head GEMM of score_tokens (_head_block): 206 MB of bf16 logits at 50 264 columns
_EAGER_CHUNK = 1024          # rows per step of the twin: (chunk, vocab) fp32 temporaries
_LOWEST = torch.finfo(torch.float32).min


def _eager_score_rows(logits, targets, want=SCORE_OUTPUTS):
    """The contract of bp_score_rows (include/bp_hip.h) in torch ops, fp32, in the kernel's order of definitions, for tensors
    the kernel does not take: with x = float(logits), m = the row's maximum (NaNs aside),
      lse = m + log(sum exp(x - m));   logprob = x_t - lse;   entropy = lse - sum(exp(x - m) * x) / sum(exp(x - m)), a -inf
      entry adding 0 to both sums;   rank = #{x_j > x_t} + #{j < t: x_j == x_t};   top1 = the lowest index of the maximum, a
      NaN counting as larger than every number.
    A target outside [0, cols) scores logprob 0 and rank -1.  Degenerate rows: a NaN anywhere makes lse, entropy and every
    logprob NaN; a +inf entry gives lse = +inf and entropy NaN; a row of -inf gives lse = -inf and entropy NaN; logprob is
    x_t - lse in each case.  The rank of a NaN target is 0.  Same signature and result as bp_hip.score_rows."""
    want = tuple(want)
    if not want or any(w not in SCORE_OUTPUTS for w in want):
        raise RuntimeError(f'_eager_score_rows: want must name some of {SCORE_OUTPUTS}')
    rows, cols = logits.shape
    flat = targets.reshape(rows, -1)
    if not 1 <= flat.shape[1] <= bp_hip.SCORE_MAX_TARGETS:
        raise RuntimeError(f'_eager_score_rows: 1 .. {bp_hip.SCORE_MAX_TARGETS} targets per row, got {flat.shape[1]}')
    parts = {n: [] for n in want}
    col = torch.arange(cols, device=logits.device)
    for lo in range(0, rows, _EAGER_CHUNK):
        x, tg = logits[lo:lo + _EAGER_CHUNK].float(), flat[lo:lo + _EAGER_CHUNK]
        nan = torch.isnan(x)
        has_nan = nan.any(dim=1)
        m = torch.where(nan, -math.inf, x).max(dim=1).values
        inf_row = torch.isinf(m)
        e = torch.exp(x - torch.where(inf_row, 0.0, m).unsqueeze(1))
        s = e.sum(dim=1)
        lse = torch.where(inf_row, m, m + torch.log(s))
        lse = torch.where(has_nan, math.nan, lse)
        inside = (tg >= 0) & (tg < cols)
        at = tg.clamp(0, cols - 1)
        xt = x.gather(1, at)
        if 'logprob' in parts:
            parts['logprob'].append(torch.where(inside, xt - lse.unsqueeze(1), 0.0))
        if 'rank' in parts:
            rank = torch.stack([(x > xt[:, i:i + 1]).sum(dim=1) + ((x == xt[:, i:i + 1]) & (col < at[:, i:i + 1])).sum(dim=1)
                                for i in range(tg.shape[1])], dim=1)
            parts['rank'].append(torch.where(inside, rank, -1).to(torch.int32))
        if 'lse' in parts:
            parts['lse'].append(lse)
        if 'top1' in parts:
            first_max = torch.where(x == m.unsqueeze(1), col, cols).min(dim=1).values
            first_nan = torch.where(nan, col, cols).min(dim=1).values
            parts['top1'].append(torch.where(has_nan, first_nan, first_max).to(torch.int32))
        if 'entropy' in parts:
            t = (e * x.clamp_min(_LOWEST)).sum(dim=1)
            parts['entropy'].append(torch.where(has_nan | inf_row, math.nan, lse - t / s))
    shapes = {n: tuple(targets.shape) if n in ('logprob', 'rank') else (rows,) for n in want}
    dtypes = {'logprob': torch.float32, 'rank': torch.int32, 'lse': torch.float32, 'top1': torch.int32, 'entropy': torch.float32}
    return {n: (torch.cat(parts[n]) if parts[n] else torch.empty(0, dtype=dtypes[n], device=logits.device)).reshape(shapes[n])
            for n in want}


def _network(model):
    return getattr(model, 'backpack_network', model)


def _hidden_and_head(model, input_ids, cu_seqlens=None, max_seqlen=None):
    """(hidden states (B, S, d), LM head) of a plain model or of a sense-intervened wrapper.  With cu_seqlens / max_seqlen
    the ids are a packed batch (total,) and the hidden states (total, d): BackpackModel's packed forward."""
    if hasattr(model, 'backpack_network') and hasattr(model, '_mixed'):
        if cu_seqlens is not None:
            raise NotImplementedError(f'{type(model).__name__} takes no packed batch: score with packed=False')
        if not _plain_wrapper_forward(model):
            raise NotImplementedError(f'{type(model).__name__} does not produce its logits as lm_head(hidden states): '
                                      'score its logits with bp_hip.score_rows instead')
        return model._mixed(input_ids, None), model.backpack_network.lm_head
    if hasattr(model, 'transformer') and hasattr(model, 'lm_head'):
        if cu_seqlens is not None:
            return model.transformer(input_ids, cu_seqlens=cu_seqlens, max_seqlen=max_seqlen), model.lm_head
        return model.transformer(input_ids), model.lm_head
    raise TypeError(f'{type(model).__name__}: expected a model with `transformer` and `lm_head`, or a sense-intervened wrapper')


def _plain_wrapper_forward(model):
    """Whether a wrapper's logits are lm_head(_mixed(ids)): true of every wrapper but the negative-weighted one, whose
    content is vocabulary-sized."""
    from src.models.intervened_models import NegativeWeightedBackpackLMHeadModel
    return not isinstance(model, NegativeWeightedBackpackLMHeadModel)


def _score(model, logits, targets, want):
    """The kernel for a HIP-path model on the GPU (a failure raises: no fallback), the twin otherwise."""
    config = getattr(_network(model), 'config', None)
    if logits.is_cuda and bool(getattr(config, 'use_flash_attn', False)):
        return bp_hip.score_rows(logits, targets, want=want)
    return _eager_score_rows(logits, targets, want=want)


def _head_block(total):
    """Rows of one LM-head GEMM: HEAD_BLOCK_ROWS, or for fewer scored rows their count rounded up to 128.  The bits a GEMM
    gives a row depend on the GEMM's shape (the library picks another kernel for 7 rows than for 128), and 16-bit logits tie,
    so a rank can move with them: every GEMM of a call has this one shape (the last block is padded with a repeated row),
    which depends on the number of scored rows alone -- not on chunk_tokens, nor on which rows are scored."""
    return min(HEAD_BLOCK_ROWS, max(128, -(-total // 128) * 128))


def _shifted(input_ids, ignore_index):
    labels = torch.full_like(input_ids, ignore_index)
    labels[:, :-1] = input_ids[:, 1:]
    return labels


@torch.no_grad()
def score_tokens(model, input_ids, labels=None, lengths=None, chunk_tokens=16384, ignore_index=-100, want=SCORE_OUTPUTS,
                 packed=False):
    """Per-token scores of `input_ids` (B, S) under `model`: TokenScores of (B, S) tensors -- `logprobs` fp32 (the
    log-probability of the label), `ranks` int32 (0-based rank of the label among the logits, ties towards the lower id),
    `top1` int32 (the greedy token), `entropy` and `lse` fp32, and `mask` (bool: the position was scored).

    labels (B, S) default to the inputs shifted left (the last position unscored); `ignore_index` entries are unscored.
    lengths (B,): rows are right-padded to S and positions >= length - 1 are unscored (their label is a pad).  The LM head and
    the scoring run over the scored rows only, gathered before the GEMM: the head in blocks of one fixed shape (_head_block, at
    most HEAD_BLOCK_ROWS rows -- the logits alive at once), the scoring at most `chunk_tokens` rows a launch.  The outputs do
    not depend on chunk_tokens, bit for bit.  Unscored positions hold 0 (logprobs, entropy, lse) and -1 (ranks, top1).
    `want`: the subset of outputs to compute; the others are None.
    packed=True (needs `lengths`): the model runs on the PACKED batch -- the rows' real tokens behind one another
    (src/utils/packing.py, BackpackModel.forward's cu_seqlens form) -- so the pads cost no trunk, sense or head work; the
    returned (B, S) tensors are laid out as without it.  The lengths are read on the host (one synchronisation)."""
    if labels is None:
        labels = _shifted(input_ids, ignore_index)
    batch, seqlen = input_ids.shape
    mask = labels != ignore_index
    if lengths is not None:
        lengths = torch.as_tensor(lengths, device=input_ids.device)
        mask = mask & (torch.arange(seqlen, device=input_ids.device)[None, :] < (lengths[:, None] - 1))
    if packed:
        if lengths is None:
            raise ValueError('score_tokens: packed=True needs lengths')
        ids, cu_seqlens, max_seqlen = pack_sequences(input_ids, lengths)
        hidden, head = _hidden_and_head(model, ids, cu_seqlens, max_seqlen)
    else:
        hidden, head = _hidden_and_head(model, input_ids)
    rows = hidden.reshape(-1, hidden.shape[-1])
    index = mask.reshape(-1).nonzero().squeeze(1)       # the scored positions as b * S + s: where the outputs go
    # ... and as rows of the hidden states: where the head reads
    source = cu_seqlens.long()[index // seqlen] + index % seqlen if packed else index
    flat_labels = labels.reshape(-1).to(torch.int64)
    names = {'logprob': 'logprobs', 'rank': 'ranks', 'top1': 'top1', 'entropy': 'entropy', 'lse': 'lse'}
    want = tuple(want)
    out = {n: torch.full((batch * seqlen,), -1, dtype=torch.int32, device=rows.device) if n in ('rank', 'top1')
           else torch.zeros(batch * seqlen, dtype=torch.float32, device=rows.device) for n in want}
    chunk, total = max(1, int(chunk_tokens)), index.shape[0]
    block = _head_block(total)
    for b0 in range(0, total, block):
        sel, src = index[b0:b0 + block], source[b0:b0 + block]
        take = src if src.shape[0] == block else torch.cat([src, src[-1:].expand(block - src.shape[0])])   # the last block, padded
        logits = head(rows[take])[:sel.shape[0]]
        for lo in range(0, sel.shape[0], chunk):
            got = _score(model, logits[lo:lo + chunk], flat_labels[sel[lo:lo + chunk]], want)
            for n in want:
                out[n][sel[lo:lo + chunk]] = got[n]
    fields = {names[n]: out[n].reshape(batch, seqlen) for n in want}
    return TokenScores(mask=mask, **{f: fields.get(f) for f in TokenScores._fields if f != 'mask'})


@torch.no_grad()
def sequence_scores(model, input_ids, lengths=None, prefix_lengths=None, chunk_tokens=16384, packed=False):
    """Per row of `input_ids` (B, S), the score of its tokens [prefix, length): SequenceScores of (B,) tensors -- `logprob`
    float64 (the sum of their log-probabilities), `count` int64 and `all_top1` (bool: every one of them was the greedy
    token).  Token j is predicted at position j - 1, so token 0 is never scored.  lengths default to S, prefix_lengths to 0.
    `packed`: as in score_tokens."""
    batch, seqlen = input_ids.shape
    labels = _shifted(input_ids, -100)
    if prefix_lengths is not None:
        prefix = torch.as_tensor(prefix_lengths, device=input_ids.device)
        before = torch.arange(seqlen, device=input_ids.device)[None, :] < (prefix[:, None] - 1)
        labels = labels.masked_fill(before, -100)
    got = score_tokens(model, input_ids, labels=labels, lengths=lengths, chunk_tokens=chunk_tokens, want=('logprob', 'rank'),
                       packed=packed)
    return SequenceScores(logprob=got.logprobs.double().sum(dim=1), count=got.mask.sum(dim=1),
                          all_top1=((got.ranks == 0) | ~got.mask).all(dim=1))


def generation_logprob(output, prompt_lengths=None):
    """The likelihood a generation had when it was produced, from the record of its picks: `output` is the DecoderOnlyOutput of
    greedy_decode / sample (or GenerationMixin.generate / .sample with return_dict_in_generate) under output_logprobs=True.
    Per row, over its generated tokens -- the columns with a rank >= 0: behind the prompt and in front of the row's end, the EOS
    itself included -- SequenceScores-like (logprob, count, perplexity): the float64 sum of `token_logprobs`, the int64 token
    count and exp(-logprob / count) (NaN for a row that generated nothing).  Unlike a second pass with sequence_scores this is
    the distribution each token was picked from, also for models whose cached step and full forward differ (the annealed
    WeightedBackpackLMHeadModel).  prompt_lengths (B,): count only columns >= the row's prompt length (the record holds nothing
    in front of it anyway; given for symmetry with greedy_decode)."""
    if output.token_logprobs is None or output.token_ranks is None:
        raise ValueError('generation_logprob: the output carries no record; generate with output_logprobs=True')
    live = output.token_ranks >= 0
    if prompt_lengths is not None:
        begin = torch.as_tensor(prompt_lengths, device=live.device).long()
        live = live & (torch.arange(live.shape[1], device=live.device)[None, :] >= begin[:, None])
    logprob = torch.where(live, output.token_logprobs.double(), 0.0).sum(dim=1)
    count = live.sum(dim=1)
    perplexity = torch.where(count > 0, torch.exp(-logprob / count.clamp(min=1)), math.nan)
    return GenerationScores(logprob=logprob, count=count, perplexity=perplexity)


def _batch_of(batch):
    if isinstance(batch, dict):
        return batch['input_ids'], batch.get('labels'), batch.get('lengths')
    if isinstance(batch, (tuple, list)):
        return batch[0], (batch[1] if len(batch) > 1 else None), (batch[2] if len(batch) > 2 else None)
    return batch, None, None


@torch.no_grad()
def evaluate_lm(model, batches, chunk_tokens=16384, ignore_index=-100, packed=False):
    """Loss, perplexity and top-1 accuracy of `model` over `batches`: an iterable of (B, S) id tensors, of (input_ids, labels[,
    lengths]) tuples or of dicts with those names.  Returns {'loss', 'perplexity', 'accuracy', 'tokens'}.  Sums are float64
    and the perplexity is the exponential of the mean loss, as the reference's Perplexity metric
    (training/src/metrics/perplexity.py); the accuracy counts positions whose label has rank 0 (metrics/accuracy.py).
    `packed`: batches that carry lengths run packed (score_tokens); the others as they are."""
    nll = correct = tokens = None
    for batch in batches:
        ids, labels, lengths = _batch_of(batch)
        got = score_tokens(model, ids, labels=labels, lengths=lengths, chunk_tokens=chunk_tokens, ignore_index=ignore_index,
                           want=('logprob', 'rank'), packed=packed and lengths is not None)
        part = (-got.logprobs.double().sum(), ((got.ranks == 0) & got.mask).sum(), got.mask.sum())
        nll, correct, tokens = part if nll is None else (nll + part[0], correct + part[1], tokens + part[2])
    if nll is None or int(tokens) == 0:
        return {'loss': math.nan, 'perplexity': math.nan, 'accuracy': math.nan, 'tokens': 0}
    loss = float(nll) / int(tokens)
    return {'loss': loss, 'perplexity': math.exp(loss), 'accuracy': int(correct) / int(tokens), 'tokens': int(tokens)}


def _padded(sequences, device, pad_id=0):
    """Right-padded (N, longest) ids and the (N,) lengths of a list of id sequences."""
    sequences = [list(map(int, s.tolist() if torch.is_tensor(s) else s)) for s in sequences]
    longest = max(len(s) for s in sequences)
    ids = torch.full((len(sequences), longest), pad_id, dtype=torch.int64)
    for i, s in enumerate(sequences):
        ids[i, :len(s)] = torch.tensor(s, dtype=torch.int64)
    return ids.to(device), torch.tensor([len(s) for s in sequences], dtype=torch.int64, device=device)


def _device_of(model):
    return _network(model).lm_head.weight.device


def _ragged_scores(model, sequences, prefixes=None, batch_size=32, packed=False):
    """sequence_scores of a list of id sequences of different lengths, `batch_size` at a time, right-padded; `packed`: the
    model runs on the packed batch instead (score_tokens).  last_word_eval, pair_accuracy and rank_choices pass it through."""
    device, parts = _device_of(model), []
    for lo in range(0, len(sequences), batch_size):
        ids, lengths = _padded(sequences[lo:lo + batch_size], device)
        prefix = None if prefixes is None else torch.tensor(prefixes[lo:lo + batch_size], dtype=torch.int64, device=device)
        parts.append(sequence_scores(model, ids, lengths=lengths, prefix_lengths=prefix, packed=packed))
    return SequenceScores(*[torch.cat(field) for field in zip(*parts)])


def _ids(sequence):
    return list(map(int, sequence.tolist() if torch.is_tensor(sequence) else sequence))


def last_word_eval(model, examples, batch_size=32, packed=False):
    """The LAMBADA protocol on (context ids, target ids) pairs: an example is right when every target token is the greedy
    token given what precedes it.  Returns {'accuracy', 'perplexity' (of the target tokens), 'examples', 'tokens'}."""
    examples = [(_ids(c), _ids(t)) for c, t in examples]
    if any(not c or not t for c, t in examples):
        raise ValueError('last_word_eval: every example needs a non-empty context and a non-empty target')
    got = _ragged_scores(model, [c + t for c, t in examples], [len(c) for c, _ in examples], batch_size, packed)
    tokens = int(got.count.sum())
    return {'accuracy': float(got.all_top1.double().mean()), 'perplexity': math.exp(-float(got.logprob.sum()) / tokens),
            'examples': len(examples), 'tokens': tokens}


def pair_accuracy(model, good, bad, batch_size=32, packed=False):
    """Minimal pairs: the share of pairs whose `good` sequence scores a higher total log-probability than its `bad` one
    (tokens 1 .. of each).  Returns {'accuracy', 'good', 'bad'}, the last two the (N,) float64 scores."""
    if len(good) != len(bad) or not len(good):
        raise ValueError('pair_accuracy: good and bad must be two lists of the same, non-zero length')
    a = _ragged_scores(model, [_ids(s) for s in good], None, batch_size, packed).logprob
    b = _ragged_scores(model, [_ids(s) for s in bad], None, batch_size, packed).logprob
    return {'accuracy': float((a > b).double().mean()), 'good': a, 'bad': b}


def rank_choices(model, context, choices, normalize=False, batch_size=32, packed=False):
    """Multiple choice: the log-probability of every continuation in `choices` after `context` (ids), divided by its token
    count with `normalize`.  Returns (order, scores): the indices of the choices best first (ties: the lower index) and the
    (len(choices),) float64 scores."""
    context, choices = _ids(context), [_ids(c) for c in choices]
    if not context or not choices or any(not c for c in choices):
        raise ValueError('rank_choices: a non-empty context and non-empty choices')
    got = _ragged_scores(model, [context + c for c in choices], [len(context)] * len(choices), batch_size, packed)
    scores = got.logprob / got.count if normalize else got.logprob
    return torch.sort(scores, descending=True, stable=True).indices, scores


@torch.no_grad()
def candidate_probs(model, input_ids, positions, candidate_ids):
    """Log-probabilities and ranks of up to 8 candidate next tokens at N places of a batch.  positions: N (sample, position)
    pairs; candidate_ids: (M,) for every place, or (N, M).  The LM head runs over the N rows only and the M-target form of
    bp_score_rows reads each row once.  Returns (logprobs (N, M) fp32, ranks (N, M) int32)."""
    hidden, head = _hidden_and_head(model, input_ids)
    where = torch.as_tensor(positions, dtype=torch.int64, device=hidden.device).reshape(-1, 2)
    cand = torch.as_tensor(candidate_ids, dtype=torch.int64, device=hidden.device)
    if cand.dim() == 1:
        cand = cand.unsqueeze(0).expand(where.shape[0], -1)
    if cand.dim() != 2 or cand.shape[0] != where.shape[0] or not 1 <= cand.shape[1] <= bp_hip.SCORE_MAX_TARGETS:
        raise ValueError(f'candidate_probs: candidate_ids must be (M,) or (N, M) with 1 <= M <= {bp_hip.SCORE_MAX_TARGETS}')
    got = _score(model, head(hidden[where[:, 0], where[:, 1]]), cand.contiguous(), ('logprob', 'rank'))
    return got['logprob'], got['rank']


def bias_ratio(model, input_ids, positions, id_a, id_b):
    """max(p_a / p_b, p_b / p_a) of two next tokens at N (sample, position) places: the bias measure of
    training/src/test_genderbias.py:194-197 (p(' he') against p(' she')).  Returns (N,) float64."""
    logprobs, _ = candidate_probs(model, input_ids, positions, [int(id_a), int(id_b)])
    return torch.exp((logprobs[:, 0].double() - logprobs[:, 1].double()).abs())
