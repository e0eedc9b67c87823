"""Lexical similarity of sense vectors -- MI355X-native mirror of the reference's training/src/run_simlex.py (the cosine
measures `Cos`, `MinPair`, `MaxPair`, `MinAll`, `MaxAll`, `CosSense{l}` of :189-241 and their Spearman correlations with
SimLex-999, SimVerb-3500, RG-65 and WordSim-353, :244-271) and of the neighbour search of training/src/visualize_sim.py
(:197-222, which walks the vocabulary in Python with one 16 x 16 cosine matrix per candidate word).

Every measure is a reduction of the k x k dot products of two words' sense vectors and of their 2 k squared norms, so all of
them come from ONE kernel, bp_sense_similarity (csrc/sense_similarity.hip): a group of query words against candidate rows of
`BackpackModel.sense_table()`, each candidate row read once.  CPU tensors, fp32 tensors and sense counts the kernel does not
take go through `_eager_sense_similarity`, which states the same contract in fp32 torch ops.

Everything runs under torch.no_grad() and takes a BackpackLMHeadModel on any device."""
from collections import namedtuple

import numpy as np
import torch

import bp_hip
from src.utils import sense_vocab

MEASURES = ('Cos', 'MinPair', 'MaxPair', 'MinAll', 'MaxAll')
_OUTPUT_OF = {'Cos': 'flat', 'MinPair': 'min_pair', 'MaxPair': 'max_pair', 'MinAll': 'min_all', 'MaxAll': 'max_all'}
_EAGER_CHUNK = 4096        # candidates per step of the torch twin: a (nq, chunk, k, k) fp32 block

_force_eager = False       # tests: take the torch twin whatever the operands are


def measure_names(k):
    """The reference's names for a model with k sense vectors, in its order (run_simlex.py:231-241)."""
    return list(MEASURES) + [f'CosSense{l}' for l in range(k)]


def _output_of(measure, k):
    """(kernel output, sense index or None) of a measure name."""
    if measure in _OUTPUT_OF:
        return _OUTPUT_OF[measure], None
    if measure.startswith('CosSense') and measure[8:].isdigit() and int(measure[8:]) < k:
        return 'per_sense', int(measure[8:])
    raise ValueError(f'unknown similarity measure {measure!r}; expected one of {measure_names(k)}')


def _eager_sense_similarity(table, query, cand_index=None, want=bp_hip.SIMILARITY_OUTPUTS, out=None):
    """The contract of bp_sense_similarity (include/bp_hip.h) in fp32 torch ops, with the signature of
    bp_hip.sense_similarity: table (rows, k, d), query (nq, k, d) of any floating dtype on any device; cand_index clamped as
    an unsigned number to the table.  Dots and squared norms are fp32 sums of exact products, a cosine is
    dot / (sqrt(A) * sqrt(B)) in the order of run_simlex.py:202-208, torch.min / torch.max carry a NaN."""
    rows, k, d = table.shape
    nq = query.shape[0]
    if cand_index is None:
        idx = torch.arange(rows, device=table.device)
    else:
        idx = torch.clamp(cand_index.to(torch.int64) & 0xffffffff, max=rows - 1)
    ncand = idx.numel()
    want = tuple(want)
    res = {}
    for name in want:
        shape = (nq, k, ncand) if name == 'per_sense' else (nq, ncand)
        given = out.get(name) if out is not None else None
        res[name] = given if given is not None else torch.empty(shape, dtype=torch.float32, device=table.device)
    q = query.float()
    qa = (q * q).sum(-1)                                                  # (nq, k)
    for c0 in range(0, ncand, _EAGER_CHUNK):
        sl = slice(c0, min(ncand, c0 + _EAGER_CHUNK))
        cand = table[idx[sl]].float()                                     # (c, k, d)
        cb = (cand * cand).sum(-1)                                        # (c, k)
        g = torch.einsum('nie,cje->ncij', q, cand)                        # (nq, c, k, k): [l', l]
        cos = g / (qa.sqrt()[:, None, :, None] * cb.sqrt()[None, :, None, :])
        diag = torch.diagonal(cos, dim1=2, dim2=3)                        # (nq, c, k)
        every = cos.reshape(nq, cos.shape[1], k * k)
        parts = {'per_sense': lambda: diag.transpose(1, 2),
                 'min_pair': lambda: diag.min(-1).values, 'max_pair': lambda: diag.max(-1).values,
                 'min_all': lambda: every.min(-1).values, 'max_all': lambda: every.max(-1).values,
                 'flat': lambda: torch.diagonal(g, dim1=2, dim2=3).sum(-1)
                 / (qa.sum(-1).sqrt()[:, None] * cb.sum(-1).sqrt()[None, :])}
        for name in want:
            res[name][..., sl] = parts[name]()
    return res


def _similarity(table, query, cand_index=None, want=bp_hip.SIMILARITY_OUTPUTS):
    """bp_sense_similarity on the HIP path, its torch twin for everything the kernel does not take."""
    if not _force_eager and bp_hip.sense_similarity_supported(table, query):
        return bp_hip.sense_similarity(table, query, cand_index=cand_index, want=want)
    return _eager_sense_similarity(table, query, cand_index=cand_index, want=want)


def _query_group(k):
    return max(1, bp_hip.SIMILARITY_MAX_QUERY_ROWS // k)


# ---- vectors of words -----------------------------------------------------------------------------------------------------------------

def _word_ids(words):
    """A list of token-id lists from a list of token ids or of token-id lists."""
    out = []
    for w in words:
        ids = [int(w)] if not hasattr(w, '__len__') else [int(t) for t in w]
        if not ids:
            raise ValueError('a word needs at least one token')
        out.append(ids)
    return out


def _pool(rows, words, use_first, dtype):
    """rows (T, ...) of all tokens of all words in order -> (N, ...): a single token's row as it is, the fp32 mean over a
    multi-token word's rows rounded once to `dtype` (run_simlex.py:181-185), or its first token's row."""
    starts = np.cumsum([0] + [len(w) for w in words])
    first = torch.as_tensor(starts[:-1], device=rows.device)
    res = rows[first].to(dtype)
    if not use_first:
        for i, w in enumerate(words):
            if len(w) > 1:
                res[i] = rows[starts[i]:starts[i + 1]].float().mean(0).to(dtype)
    return res


@torch.no_grad()
def sense_vectors(model, words, use_first=False):
    """(N, k, d) in the model's dtype: the sense vectors of every word of `words` (token ids, or token-id lists for words
    the tokenizer splits).  Rows of `sense_table()`, or the content network's output when the model serves no table."""
    words = _word_ids(words)
    dev = model.lm_head.weight.device
    ids = torch.as_tensor([t for w in words for t in w], device=dev, dtype=torch.long)
    table = model.transformer.sense_table()
    if table is not None:
        rows = table[ids]
    else:
        k = model.transformer.num_content_vectors
        rows = sense_vocab._content_rows(model, ids).reshape(ids.numel(), k, -1)
    return _pool(rows, words, use_first, model.lm_head.weight.dtype)


@torch.no_grad()
def softmax_vectors(model, words, use_first=False):
    """(N, 1, d): the softmax-matrix baseline of run_simlex.py:137-160, rows of `lm_head.weight` (tied with the input
    embedding) pooled like the sense vectors.  One vector per word: every measure is the plain cosine, the kernel with k = 1."""
    words = _word_ids(words)
    weight = model.lm_head.weight
    ids = torch.as_tensor([t for w in words for t in w], device=weight.device, dtype=torch.long)
    return _pool(weight.detach()[ids], words, use_first, weight.dtype).unsqueeze(1)


# ---- paired scores and neighbours -------------------------------------------------------------------------------------------------------

def _distinct(x):
    """(distinct rows of x (N, k, d) by their bits, index of every row among them)."""
    n = x.shape[0]
    as_int = x.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]).reshape(n, -1)
    _, inverse = torch.unique(as_int, dim=0, return_inverse=True)
    first = torch.full((int(inverse.max()) + 1,), n, dtype=torch.long, device=x.device)
    first.scatter_reduce_(0, inverse, torch.arange(n, device=x.device), reduce='amin')
    return x[first].contiguous(), inverse


@torch.no_grad()
def sense_similarity(a, b, measures=None):
    """The similarity of word pair i = (a[i], b[i]); a, b (N, k, d) as `sense_vectors` / `softmax_vectors` return them.
    Returns a dict measure name -> (N,) fp32 over `measures` (default: all of `measure_names(k)`).  The kernel runs on the
    DISTINCT words: groups of distinct first words are the queries, the distinct second words are the table, a pair's
    partners are the candidates of its group, and every pair reads its own score out of the group's block."""
    if a.dim() != 3 or a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError(f'a and b must be (N, k, d) tensors of one dtype, got {tuple(a.shape)} and {tuple(b.shape)}')
    n, k, d = a.shape
    names = measure_names(k) if measures is None else list(measures)
    outputs = [_output_of(m, k) for m in names]
    want = tuple(dict.fromkeys(o for o, _ in outputs))
    res = {m: torch.empty((n,), dtype=torch.float32, device=a.device) for m in names}
    if n == 0:
        return res
    ua, ia = _distinct(a)
    ub, ib = _distinct(b)
    order = torch.argsort(ia, stable=True)                               # pairs by first word: a group's pairs are one run
    sorted_ia = ia[order]
    step = _query_group(k)
    for q0 in range(0, ua.shape[0], step):
        q1 = min(ua.shape[0], q0 + step)
        lo = int(torch.searchsorted(sorted_ia, q0))
        hi = int(torch.searchsorted(sorted_ia, q1))
        pairs = order[lo:hi]
        block = _similarity(ub, ua[q0:q1], cand_index=ib[pairs].to(torch.int32), want=want)
        rows = sorted_ia[lo:hi] - q0
        cols = torch.arange(hi - lo, device=a.device)
        for m, (o, sense) in zip(names, outputs):
            res[m][pairs] = block[o][rows, cols] if sense is None else block[o][rows, sense, cols]
    return res


@torch.no_grad()
def sense_neighbors(model, words, count=100, measure='MinPair', largest=True, candidates=None, use_first=False, vocab_size=None):
    """The `count` nearest (or, with largest=False, farthest) words of every query word in sense space by `measure`: the
    search of visualize_sim.py:197-222 in one kernel call per group of query words, then bp_row_extremes on the (queries,
    candidates) scores.

    words       token ids or token-id lists (`sense_vectors`)
    candidates  token ids to search; default: the ids below the tokenizer's vocabulary size -- `vocab_size`, or the
                `vocab_size` the config had before it was padded to a multiple (`config.unpadded_vocab_size`): the rows
                the embedding was padded with are not words
    Returns (ids int64, scores fp32), (N, count) each, best first.  Scores are ordered by the integer key of their bits (the
    contract of bp_row_extremes: a NaN score -- a zero sense vector -- sorts beyond the largest numbers), equal scores by
    ascending position in `candidates`, i.e. by ascending id for the default."""
    k = model.transformer.num_content_vectors
    output, sense = _output_of(measure, k)
    queries = sense_vectors(model, words, use_first=use_first)
    dev = queries.device
    vocab = int(vocab_size if vocab_size is not None
                else getattr(model.config, 'unpadded_vocab_size', model.config.vocab_size))
    cand = None if candidates is None else torch.as_tensor(candidates, device=dev).reshape(-1).long()
    table = model.transformer.sense_table()
    if table is None:                                                     # no table: the candidates' rows ARE the table
        ids = torch.arange(vocab, device=dev) if cand is None else cand
        table = torch.cat([sense_vocab._content_rows(model, ids[i:i + 512]).reshape(-1, k, queries.shape[-1])
                           for i in range(0, ids.numel(), 512)])
        index = None
    else:
        index = None if cand is None else cand.to(torch.int32)
        if cand is None:
            table = table[:vocab]
    ncand = table.shape[0] if index is None else index.numel()
    count = int(count)
    if not 1 <= count <= ncand:
        raise ValueError(f'count must be in [1, {ncand}] (the number of candidates), got {count}')
    n = queries.shape[0]
    ids_out = torch.empty((n, count), dtype=torch.int64, device=dev)
    scores_out = torch.empty((n, count), dtype=torch.float32, device=dev)
    step = _query_group(k)
    for q0 in range(0, n, step):
        block = _similarity(table, queries[q0:q0 + step], cand_index=index, want=(output,))[output]
        scores = block if sense is None else block[:, sense]
        val, idx = _extremes(scores, count, largest)
        scores_out[q0:q0 + step] = val
        ids_out[q0:q0 + step] = idx.long() if cand is None else cand[idx.long()]
    return ids_out, scores_out


def _extremes(scores, count, largest):
    """(values, columns) of the `count` largest / smallest scores of every row, in the order of bp_row_extremes.  The kernel
    keeps at most bp_hip.ROW_EXTREMES_MAX_N per end; a longer list is a stable sort on the same integer keys."""
    if count <= bp_hip.ROW_EXTREMES_MAX_N:
        tv, ti, bv, bi = sense_vocab._row_extremes(scores, count, largest, not largest)
        return (tv, ti) if largest else (bv, bi)
    keys = sense_vocab._ordered_keys(scores)
    idx = torch.sort(-keys if largest else keys, dim=1, stable=True).indices[:, :count]
    return torch.gather(scores, 1, idx), idx


# ---- evaluation ---------------------------------------------------------------------------------------------------------------------------

SimilarityExample = namedtuple('SimilarityExample', ['word1', 'word2', 'gold_score'])

# kind -> (delimiter, skip the first line, column of the gold score): run_simlex.py:53-106
_FORMATS = {'simlex999': ('\t', True, 3), 'simverb3500': ('\t', False, 3), 'rg65': (';', False, 2), 'ws353': (',', True, 2)}


def load_similarity_file(path, kind):
    """The examples of a similarity dataset file as SimilarityExample(word1, word2, gold_score); `kind` one of 'simlex999'
    (tab-separated, header line, score in the fourth column), 'simverb3500' (the same without a header), 'rg65'
    (semicolons, score in the third column) and 'ws353' (commas, header line, score in the third column)."""
    if kind not in _FORMATS:
        raise ValueError(f'unknown dataset kind {kind!r}; expected one of {sorted(_FORMATS)}')
    delimiter, skip_first, column = _FORMATS[kind]
    examples = []
    with open(path) as fin:
        for i, line in enumerate(fin):
            if (i == 0 and skip_first) or not line.strip():
                continue
            data = [x.strip() for x in line.split(delimiter)]
            examples.append(SimilarityExample(data[0], data[1], float(data[column])))
    return examples


def tokenize_examples(examples, tokenizer, single_token_only=False):
    """Examples with their words as token-id lists: a word is tokenized with a leading space (`mogrify_word`,
    run_simlex.py:109-117); `single_token_only` drops the examples with a word of several tokens (`filter_to_tokenizer`)."""
    out = []
    for ex in examples:
        ids = [list(tokenizer(' ' + w)['input_ids']) for w in (ex[0], ex[1])]
        if single_token_only and any(len(t) != 1 for t in ids):
            continue
        out.append(SimilarityExample(ids[0], ids[1], float(ex[2])))
    return out


def _average_ranks(v):
    v = np.asarray(v, dtype=np.float64)
    _, inverse, counts = np.unique(v, return_inverse=True, return_counts=True)
    ends = np.cumsum(counts)                       # 1-based rank of the last element of every run of equal values
    return (ends - (counts - 1) / 2.0)[inverse.reshape(-1)]


def spearman(pred, gold):
    """Spearman's rank correlation with average ranks for ties, float64 on the host (scipy.stats.spearmanr's statistic,
    run_simlex.py:260-271).  NaN when either side is constant or holds a NaN."""
    pred = np.asarray(torch.as_tensor(pred).detach().cpu().double().numpy() if torch.is_tensor(pred) else pred, dtype=np.float64)
    gold = np.asarray(torch.as_tensor(gold).detach().cpu().double().numpy() if torch.is_tensor(gold) else gold, dtype=np.float64)
    if pred.shape != gold.shape or pred.ndim != 1:
        raise ValueError('spearman: two vectors of one length')
    if pred.size < 2 or np.isnan(pred).any() or np.isnan(gold).any():
        return float('nan')
    rp, rg = _average_ranks(pred), _average_ranks(gold)
    rp, rg = rp - rp.mean(), rg - rg.mean()
    den = np.sqrt((rp * rp).sum() * (rg * rg).sum())
    return float((rp * rg).sum() / den) if den > 0 else float('nan')


@torch.no_grad()
def evaluate_similarity(model, examples, use_softmax=False, use_first=False, tokenizer=None):
    """Spearman's rho of every measure against the gold scores of `examples` (`get_sims_for_fn` + `get_evals_of_sims`,
    run_simlex.py:244-271): a dict measure name -> rho.  An example is (word1, word2, gold_score) with words as token ids or
    token-id lists, or as strings when a `tokenizer` is given.  `use_softmax`: the softmax-matrix baseline, `Cos` only."""
    if tokenizer is not None:
        examples = tokenize_examples(examples, tokenizer)
    vectors = softmax_vectors if use_softmax else sense_vectors
    a = vectors(model, [ex[0] for ex in examples], use_first=use_first)
    b = vectors(model, [ex[1] for ex in examples], use_first=use_first)
    gold = [float(ex[2]) for ex in examples]
    sims = sense_similarity(a, b, measures=['Cos'] if use_softmax else None)
    return {name: spearman(score, gold) for name, score in sims.items()}
