"""GPU: bp_pick_token_lim (csrc/pick_token_lim.hip) against the numpy restatement of tests/pick_lim_ref.py -- controls off equals
bp_pick_token_ctl bit for bit, every bit of the ban bitmap, the edges of the n-gram scan, exact counts through planted
collisions of the count table, the kept set and the draw under all controls, graph capture with a growing history -- and the
generation loops on the decode models."""
import numpy as np
import pytest
import torch

import pick_lim_ref as L
import pick_ref as R
from decode_support import DEV, VOCAB, _bp, _model

pytestmark = pytest.mark.gpu

SEED, OFFSET = 1234, 77
INF, NAN = float('inf'), float('nan')
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}


def _state(seed=SEED, offset=OFFSET):
    return torch.tensor([seed, offset], dtype=torch.int64, device=DEV)


def _place(rows, dtype, pad=0, misalign=0):
    """(B, vocab) host fp32 rows -> a device tensor of `dtype` with row stride vocab + pad whose base is `misalign`
    elements behind a 16-byte boundary (test_gpu_pick_control.py's, restated)."""
    rows = torch.as_tensor(rows, dtype=torch.float32)
    b, v = rows.shape
    flat = torch.zeros(b * (v + pad) + 16, dtype=dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = flat[misalign:misalign + b * (v + pad)].view(b, v + pad)[:, :v]
    view.copy_(rows.to(dtype))
    return view


def _host(t):
    return t.float().cpu().numpy()


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _positions(vocab):
    if vocab <= 257:
        return list(range(vocab))
    fixed = [0, 1, 31, 32, 63, 64, 65, 4095 if vocab > 4096 else vocab - 2, vocab - 1]
    seeded = np.random.default_rng(vocab).integers(0, vocab, size=32).tolist()
    return fixed + [int(t) for t in seeded]


# ---- controls off: bp_pick_token_ctl, bit for bit ------------------------------------------------------------------------------------

def _mixed_rows(batch, vocab, rng):
    x = (2.0 * rng.standard_normal((batch, vocab))).astype(np.float32)
    x[1] = np.round(x[1] * 2) / 2
    x[2, vocab // 2:] = -INF
    x[3] *= 8.0
    x[4, vocab // 3] = NAN
    x[5, :] = -INF
    x[6, vocab - 1] = INF
    x[7] = -np.abs(x[7])
    return x


@pytest.mark.parametrize('layout', ['dense', 'strided-misaligned'])
@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('vocab', [7, 257, 4096, 50264])
def test_controls_off_equals_the_controlled_pick_bit_for_bit(vocab, dtype, layout):
    bp = _bp()
    batch, cols = 10, 24
    rng = np.random.default_rng(vocab)
    x = _mixed_rows(batch, vocab, rng)
    pad, mis = (0, 0) if layout == 'dense' else (13, 3 if dtype != 'fp32' else 1)
    logits = _place(x, DTYPES[dtype], pad, mis)
    counters = _dev([0, 1, 5, 23, 24, 30, 7, 7, 2, 9], torch.int32)          # 24 and 30: the write is skipped
    seq = rng.integers(0, vocab, size=(batch, cols)).astype(np.int64)
    seq[:, 3] = -1
    entry = _dev([0, 0, 0, 0, 0, 0, 0, 0, 1, 0], torch.int32)                # row 8 is finished on entry
    eos = vocab - 2
    for sampling in (dict(do_sample=False), dict(do_sample=True, temperature=0.7, top_k=40, top_p=0.95)):
        outs = []
        for limits in (dict(), dict(penalty_begin=1)):         # penalty_begin alone selects bp_pick_token_lim and switches nothing on
            sequences, finished = _dev(seq, torch.int64), entry.clone()
            tokens, stats = bp.pick_token(logits, rng_state=_state(), counters=counters, sequences=sequences, return_stats=True,
                                          repetition_penalty=1.3, eos_token_id=eos, pad_token_id=1, min_length=6, finished=finished,
                                          **sampling, **limits)
            outs.append((tokens, _bits(stats), sequences, finished))
        for a, b in zip(*outs):
            assert torch.equal(a, b), (sampling, a.tolist(), b.tolist())


# ---- every bit of the ban bitmap ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('misalign', [0, 1])
@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
@pytest.mark.parametrize('vocab', [7, 257, 4096, 50264])
def test_every_bit_of_the_ban_bitmap(vocab, dtype, misalign):
    bp = _bp()
    value = 2.0
    ts = _positions(vocab)
    rows = len(ts)
    logits = _place(np.full((rows, vocab), value, dtype=np.float32), DTYPES[dtype], pad=5, misalign=misalign)
    assert misalign == 0 or logits.data_ptr() % 16 != 0
    ones = torch.ones(rows, dtype=torch.int32, device=DEV)
    # planted as the continuation of a bigram: the history (a, t, a) bans t and nothing else
    others = [(t + 1) % vocab for t in ts]
    sequences = _dev(np.array([others, ts, others, [0] * rows]).T, torch.int64).contiguous()
    tokens, stats = bp.pick_token(logits, True, 1.0, vocab - 1, 1.0, _state(), 3 * ones, sequences=sequences, return_stats=True,
                                  no_repeat_ngram_size=2)
    stats, tokens = stats.cpu().numpy(), tokens.cpu().tolist()
    assert stats[:, 2].tolist() == [float(vocab - 1)] * rows
    assert stats[:, 0].tolist() == [value] * rows
    assert all(tok != t for tok, t in zip(tokens, ts))
    assert sequences[:, 3].cpu().tolist() == tokens and sequences[:, 1].cpu().tolist() == ts
    # planted through suppress_tokens: the list belongs to the call, so one call per id, on that id's row (results read once)
    tokens = torch.empty(rows, dtype=torch.int64, device=DEV)
    stats = torch.empty((rows, 4), dtype=torch.float32, device=DEV)
    for r, t in enumerate(ts):
        tok, st = bp.pick_token(logits[r:r + 1], True, 1.0, vocab - 1, 1.0, _state(), ones[:1], return_stats=True,
                                suppress_tokens=_dev([t, t, -1, vocab], torch.int32))
        tokens[r], stats[r] = tok[0], st[0]
    stats, tokens = stats.cpu().numpy(), tokens.cpu().tolist()
    assert stats[:, 2].tolist() == [float(vocab - 1)] * rows and stats[:, 0].tolist() == [value] * rows
    assert all(tok != t for tok, t in zip(tokens, ts))
    # with the ids 0 .. m - 1 banned the greedy pick is m: as the 1-grams of the history, and as a list
    ms = sorted(set(ts) - {0})
    history = torch.arange(max(ms) + 1, dtype=torch.int64, device=DEV).repeat(len(ms), 1).contiguous()
    got = bp.pick_token(logits[:len(ms)], counters=_dev(ms, torch.int32), sequences=history, no_repeat_ngram_size=1)
    assert got.cpu().tolist() == [m % vocab if m < vocab else 0 for m in ms]
    for m in ms[:3] + ms[-2:]:
        got = bp.pick_token(logits[:1], suppress_tokens=torch.arange(m, dtype=torch.int32, device=DEV))
        assert got.item() == m


# ---- the edges of the n-gram scan, exact through the greedy answer --------------------------------------------------------------------

def _ngram_cases():
    """(name, history, n, seq_cols, counter, target, banned): `target` carries the largest logit, so the greedy pick is the
    target unless it is banned, and then the runner-up (id 5)."""
    cases = [
        ('match at i = 0', [9, 8, 7] + list(range(20, 40)) + [9, 8], 3, 30, 25, 7, True),
        ('match at i = Lh - n, overlapping the suffix', [1, 2, 3, 4, 4, 4], 3, 8, 6, 4, True),
        ('Lh = n - 1 bans nothing', [6, 6, 6, 6], 5, 8, 4, 6, False),
        ('Lh = n', [6, 6, 6, 6, 6], 5, 8, 5, 6, True),
        ('differs in the first compared position', [11, 2, 3, 7, 50, 51, 1, 2, 3], 4, 16, 9, 7, False),
        ('differs in the last compared position', [1, 2, 13, 7, 50, 51, 1, 2, 3], 4, 16, 9, 7, False),
        ('the exact match next to them', [1, 2, 3, 7, 50, 51, 1, 2, 3], 4, 16, 9, 7, True),
        ('ids outside the vocabulary match each other', [2 ** 40, -1, 7, 30, 2 ** 40, -1], 3, 6, 6, 7, True),
    ]
    for length in (1023, 1024, 1025, 2049):                       # the thread-stride trips of the scan
        cases.append((f'all equal, {length}', [12] * length, 2, 2050, length, 12, True))
        cases.append((f'one match at the last start position of {length}', [100 + j % 3 for j in range(length - 3)] + [77, 12, 77],
                      2, 2050, length, 12, True))
    long = [200 + j % 50 for j in range(300)]
    cases.append(('n = 64', long[:63] + [7] + long[:150] + long[:63], 64, 300, 277, 7, True))
    cases.append(('n = 64, one id off in the middle', long[:30] + [0] + long[31:63] + [7] + long[:150] + long[:63], 64, 300, 277, 7,
                  False))
    clamped = [3, 4, 7] + [60 + j for j in range(10)] + [3, 4]
    cases.append(('c > seq_cols: the clamped history, the write skipped', clamped, 3, len(clamped), len(clamped) + 5, 7, True))
    return cases


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_ngram_edges_through_the_greedy_answer(dtype):
    bp = _bp()
    vocab = 257
    x = np.zeros((1, vocab), dtype=np.float32)
    results = []
    for name, history, n, cols, counter, target, banned in _ngram_cases():
        row = np.full(cols + 1, -9, dtype=np.int64)
        row[:len(history)] = history
        h = L.clamped_history(row[:cols], counter)
        assert (target in L.ngram_set(h, n, vocab)) == banned, name
        x[:] = 0.0
        x[0, target], x[0, 5] = 3.0, 2.0
        sequences = _dev(row, torch.int64).view(1, -1)
        got = bp.pick_token(_place(x, DTYPES[dtype]), counters=_dev([counter], torch.int32), sequences=sequences[:, :cols],
                            no_repeat_ngram_size=n)
        results.append((name, got, sequences, row, cols, counter, 5 if banned else target))
    for name, got, sequences, row, cols, counter, want in results:
        assert got.item() == want, (name, got.item(), want)
        after = row.copy()
        if counter < cols:
            after[counter] = want
        assert sequences.cpu().numpy()[0].tolist() == after.tolist(), name          # the column behind seq_cols stays


# ---- counts, exact ---------------------------------------------------------------------------------------------------------------------
#
# Logits 8.0 and penalties 0.5 / 0.25: every intermediate has a few mantissa bits, so the values are exact with or without a
# contraction, in fp32 and in fp16 (the needle of the count 1000 is 508.5: ten bits, two more than bf16 holds).

COUNT_COLS, COUNT_VOCAB = 1024, 16384            # eight ids of the vocabulary start in every slot of the 2048


def _count_history():
    """A history of 1024 columns whose counts are known: four ids that start their probe in ONE slot of the 2048-slot table
    (chains of up to four), with the counts 1, 2, 3 and 1000, and ids with one occurrence each behind them."""
    a, b, c, d = L.colliding_ids(COUNT_COLS, COUNT_VOCAB, 4)
    row = [d] * 1000 + [c] * 3 + [b] * 2 + [a]
    filler = [t for t in range(COUNT_VOCAB - 1, 0, -1) if t not in (a, b, c, d)][:COUNT_COLS - len(row)]
    return row + filler, {a: 1, b: 2, c: 3, d: 1000}


@pytest.mark.parametrize('dtype', ['fp16', 'fp32'])
def test_counts_are_exact_through_stats_and_needles(dtype):
    bp = _bp()
    vocab, cols = COUNT_VOCAB, COUNT_COLS
    history, planted = _count_history()
    assert len(history) == cols and len({L.table_slot(t, cols) for t in planted}) == 1
    fp, pp = 0.5, 0.25
    rng = np.random.default_rng(3)
    order = rng.permutation(cols)                                  # the counts do not depend on where the occurrences are
    shuffled = [history[j] for j in order]
    cases = []                                                     # (history row, counter, penalty_begin, id, its count)
    for t, n in planted.items():
        cases.append((history, cols, 0, t, n))
        cases.append((shuffled, cols, 0, t, n))
    d = max(planted, key=planted.get)
    cases.append((history, cols, 400, d, 600))                     # penalty_begin in the middle
    cases.append((history, 700, 400, d, 300))                      # and the history cut at 700
    cases.append((history, 700, 699, d, 1))                        # the last position alone
    cases.append((history, 1500, 1023, history[-1], 1))            # c > seq_cols: Lh = 1024
    rows = []
    for hist_row, counter, begin, t, n in cases:
        for sign, wins in ((+0.25, True), (-0.25, False)):
            x = np.full(vocab, 8.0, dtype=np.float32)
            x[t] = 8.0 + (fp * n + pp) + sign                      # 8.25 after the penalty wins, 7.75 loses to a non-member at 8
            rows.append((hist_row, counter, begin, t, n, x, wins))
    # one launch per penalty_begin (it belongs to the call); all of them queued, then read
    launched = []
    for begin in sorted({r[2] for r in rows}):
        mine = [r for r in rows if r[2] == begin]
        logits = _place(np.stack([r[5] for r in mine]), DTYPES[dtype], pad=3, misalign=1)
        sequences = _dev(np.array([r[0] for r in mine]), torch.int64)
        counters = _dev([r[1] for r in mine], torch.int32)
        kw = dict(counters=counters, sequences=sequences, frequency_penalty=fp, presence_penalty=pp, penalty_begin=begin)
        greedy = bp.pick_token(logits, **kw)
        _, stats = bp.pick_token(logits, True, 1.0, 0, 1.0, _state(), return_stats=True, **{**kw, 'sequences': sequences.clone()})
        launched.append((mine, greedy, stats))
    for mine, greedy, stats in launched:
        greedy, stats = greedy.cpu().tolist(), stats.cpu().numpy()
        for r, (hist_row, counter, begin, t, n, x, wins) in enumerate(mine):
            h = L.clamped_history(hist_row, counter)
            tally = L.counts(h, begin, vocab)
            assert tally[t] == n, (t, n, tally[t])
            z = L.values(x, None, hist_row, counter, vocab, frequency_penalty=fp, presence_penalty=pp, penalty_begin=begin)
            assert greedy[r] == R.greedy(z) and (greedy[r] == t) == wins, (r, counter, begin, t, n, greedy[r])
            assert stats[r, 2] == vocab and stats[r, 0] == z.min(), (r, stats[r], z.min())
            others = max([v for k, v in tally.items() if k != t], default=0)
            low = 8.0 - (fp * others + pp) if others else 8.0                       # the lowest kept z reads the largest count out
            assert z.min() == min(low, z[t]), (r, others)


@pytest.mark.parametrize('dtype', ['fp16', 'fp32'])
def test_a_full_table_of_distinct_ids_and_a_member_that_is_not_counted(dtype):
    bp = _bp()
    vocab, cols = COUNT_VOCAB, COUNT_COLS
    rng = np.random.default_rng(11)
    distinct = rng.permutation(vocab)[:cols]                       # load 0.5: every id once
    logits = _place(np.full((2, vocab), 8.0, dtype=np.float32), DTYPES[dtype])
    sequences = _dev(np.stack([distinct, distinct]), torch.int64)
    counters = _dev([cols, cols], torch.int32)
    # top_k = vocab - cols keeps exactly the non-members at 8; the members all sit at 8 - 0.75
    _, stats = bp.pick_token(logits, True, 1.0, vocab - cols, 1.0, _state(), counters, sequences=sequences.clone(), return_stats=True,
                             frequency_penalty=0.5, presence_penalty=0.25)
    _, full = bp.pick_token(logits, True, 1.0, 0, 1.0, _state(), counters, sequences=sequences.clone(), return_stats=True,
                            frequency_penalty=0.5, presence_penalty=0.25)
    assert stats[:, 2].tolist() == [float(vocab - cols)] * 2 and stats[:, 0].tolist() == [8.0] * 2
    assert full[:, 2].tolist() == [float(vocab)] * 2 and full[:, 0].tolist() == [7.25] * 2
    greedy = bp.pick_token(logits, counters=counters, sequences=sequences.clone(), frequency_penalty=0.5, presence_penalty=0.25)
    first_free = min(set(range(vocab)) - set(distinct.tolist()))
    assert greedy.tolist() == [first_free] * 2
    # a member with count 0 (in the prompt only) under theta = 2: its value changes by pen alone, 16.5 -> 8.25 wins and
    # 15.5 -> 7.75 loses; a count penalty on top (0.75) would make both lose
    prompt_only = int(distinct[3])
    x = np.full((2, vocab), 8.0, dtype=np.float32)
    x[0, prompt_only], x[1, prompt_only] = 16.5, 15.5
    got = bp.pick_token(_place(x, DTYPES[dtype]), counters=counters, sequences=sequences.clone(), repetition_penalty=2.0,
                        frequency_penalty=0.5, presence_penalty=0.25, penalty_begin=10)
    z = [L.values(x[r], None, distinct, cols, vocab, repetition_penalty=2.0, frequency_penalty=0.5, presence_penalty=0.25,
                  penalty_begin=10) for r in range(2)]
    assert z[0][prompt_only] == 8.25 and z[1][prompt_only] == 7.75
    assert got.tolist() == [R.greedy(z[0]), R.greedy(z[1])] and got[0].item() == prompt_only and got[1].item() != prompt_only
    # penalty_begin at and beyond Lh: nothing is counted
    for begin in (cols, cols + 1, 2 ** 30):
        _, st = bp.pick_token(logits, True, 1.0, 0, 1.0, _state(), counters, sequences=sequences.clone(), return_stats=True,
                              frequency_penalty=0.5, presence_penalty=0.25, penalty_begin=begin)
        assert st[:, 0].tolist() == [8.0] * 2, begin


# ---- the kept set and the draw, all controls together ---------------------------------------------------------------------------------

def _sampling_rows(batch, vocab, dtype, seed=0):
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((batch, vocab))).astype(np.float32)
    x[1] = np.round(x[1] * 2) / 2
    x[2, vocab // 2:] = -INF
    x[3] *= 8.0
    x[4] *= 0.01
    return _place(x, dtype, pad=8, misalign=0)


HISTORY_LENGTHS = [0, 1, 63, 64, 65, 1024, 2000, 7]        # 2000 > the 1200 columns: clamped, and the write is skipped
COLS = 1200


def _history_rows(batch, vocab, seed):
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, vocab, size=(batch, COLS)).astype(np.int64)
    seq[:, 40:60] = seq[:, 0:20]
    seq[:, 3] = -1
    seq[:, 4] = vocab
    seq[:, 5] = 2 ** 40
    seq[:, 0] = np.arange(batch) % vocab
    counters = np.array([HISTORY_LENGTHS[b % len(HISTORY_LENGTHS)] for b in range(batch)], dtype=np.int32)
    for b in range(batch):                                   # the history ends on a bigram it holds already: something is banned
        if counters[b] >= 63:
            lh = min(int(counters[b]), COLS)
            seq[b, lh - 1] = seq[b, 10]
    return seq, counters


def _top_p_margin(z, top_k, top_p):
    keep = R.kept_set(z, top_k, 1.0)
    w = R.masses(z) * keep
    _, inverse = np.unique(z[keep], return_inverse=True)
    mass = np.bincount(inverse, weights=w[keep])[::-1]
    above = (np.cumsum(mass) - mass) / w.sum()
    return float(np.abs(above - top_p).min())


CTL_CASES = [   # vocab, dtype, theta, temperature, top_k, top_p
    (1000, 'fp32', 1.2, 0.8, 50, 1.0), (1000, 'fp32', 0.8, 1.0, 0, 0.9), (4096, 'fp16', 1.2, 1.3, 10, 1.0),
    (4096, 'bf16', 0.8, 0.7, 40, 0.95), (50264, 'bf16', 1.2, 0.7, 40, 0.95), (50264, 'bf16', 1.2, 1.0, 0, 1.0),
    (50264, 'fp16', 0.8, 1.0, 1000, 1.0), (257, 'bf16', 1.2, 1.0, 256, 0.5), (7, 'fp32', 1.2, 1.0, 3, 1.0),
]


@pytest.mark.parametrize('vocab,dtype,theta,temperature,top_k,top_p', CTL_CASES)
def test_kept_set_and_draw_under_all_controls(vocab, dtype, theta, temperature, top_k, top_p):
    bp = _bp()
    batch = 16
    logits = _sampling_rows(batch, vocab, DTYPES[dtype], seed=vocab + top_k)
    seq, counters = _history_rows(batch, vocab, seed=vocab + 1)
    x = _host(logits)
    eps = R.epsilon(vocab)
    suppress = [int(np.argmax(x[0])), int(np.argmax(x[3])), vocab, -4, int(np.argmax(x[0]))]
    limits = dict(no_repeat_ngram_size=2, frequency_penalty=0.5, presence_penalty=0.25, penalty_begin=3)
    sequences = _dev(seq, torch.int64)
    args = dict(rng_state=_state(), counters=_dev(counters, torch.int32), sequences=sequences, repetition_penalty=theta,
                eos_token_id=vocab - 1, min_length=70, finished=torch.zeros(batch, dtype=torch.int32, device=DEV),
                suppress_tokens=_dev(suppress, torch.int32), **limits)
    tokens, stats = bp.pick_token(logits, True, temperature, top_k, top_p, return_stats=True, **args)
    tokens, stats = tokens.cpu().tolist(), stats.cpu().numpy()
    kw = dict(repetition_penalty=theta, eos_token_id=vocab - 1, min_length=70, suppress_tokens=suppress, **limits)
    drawn = 0
    for b in range(batch):
        what = (vocab, dtype, theta, temperature, top_k, top_p, b)
        c = int(counters[b])
        z = L.values(x[b], temperature, seq[b], c, vocab, **kw)
        u = R.uniform(SEED, OFFSET, b, c)
        assert stats[b, 3] == np.float32(u), what
        if R.degenerate(z):                                  # nothing finite is left (small vocabularies): the greedy answer
            assert tokens[b] == R.greedy(L.values(x[b], None, seq[b], c, vocab, **kw)), what
            continue
        drawn += 1
        lo, count = stats[b, 0], int(stats[b, 2])
        keep = R.kept_set(z, top_k, top_p)
        if top_p >= 1.0 or _top_p_margin(z, top_k, top_p) > eps:
            assert count == int(keep.sum()) and lo == z[keep].min(), (what, count, int(keep.sum()), lo, z[keep].min())
        else:
            keep = R.kept_set(z, top_k, 1.0) & (z >= lo)
            assert count == int(keep.sum()) and lo == z[keep].min(), what
        R.assert_draw(tokens[b], z, keep, u, eps, what=what)
        assert tokens[b] not in suppress and (c >= 70 or tokens[b] != vocab - 1), what
    assert drawn >= (batch // 2 if vocab > 7 else 1)
    want = torch.as_tensor(seq).clone()
    for b in range(batch):
        if 0 <= counters[b] < COLS:
            want[b, counters[b]] = tokens[b]
    assert torch.equal(sequences.cpu(), want)
    greedy = bp.pick_token(logits, **{**args, 'sequences': _dev(seq, torch.int64)})
    for b in range(batch):
        assert greedy[b].item() == R.greedy(L.values(x[b], None, seq[b], int(counters[b]), vocab, **kw)), b
    again, stats2 = bp.pick_token(logits, True, temperature, top_k, top_p, return_stats=True,
                                  **{**args, 'sequences': _dev(seq, torch.int64)})
    assert again.cpu().tolist() == tokens and torch.equal(_bits(stats2).cpu(), torch.as_tensor(stats).view(torch.int32))


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_top_k_selects_on_the_values_under_the_frequency_penalty_not_on_the_raw_elements(dtype):
    bp = _bp()
    vocab = 4096
    x = np.full((2, vocab), -5.0, dtype=np.float32)
    x[:, 100:120] = 8.0 - 0.25 * np.arange(20)           # exact in both 16-bit formats: 8, 7.75, ... at columns 100 ..
    logits = _place(x, DTYPES[dtype])
    # the raw top-3 occur 4, 4 and 3 times: at a_f = 1 they drop to 4, 3.75 and 4.5, below the 7.25 of column 103
    seq = np.array([[100, 101, 102, 100, 101, 102, 100, 101, 102, 100, 101]] * 2, dtype=np.int64)
    counters = _dev([11, 11], torch.int32)
    for top_k, top_p in ((2, 1.0), (3, 1.0), (2, 0.5)):
        tokens, stats = bp.pick_token(logits, True, 1.0, top_k, top_p, _state(), counters, sequences=_dev(seq, torch.int64),
                                      return_stats=True, frequency_penalty=1.0)
        for b in range(2):
            z = L.values(_host(logits)[b], 1.0, seq[b], 11, vocab, frequency_penalty=1.0)
            assert z[100] == 4.0 and z[101] == 3.75 and z[102] == 4.5
            keep = R.kept_set(z, top_k, top_p)
            assert set(np.nonzero(keep)[0]) <= set(range(103, 103 + top_k))
            assert int(stats[b, 2]) == int(keep.sum()) and stats[b, 0].item() == z[keep].min(), (b, top_k, top_p)
            assert keep[tokens[b].item()], (b, top_k, top_p, tokens[b].item())


def test_the_largest_vocabulary_a_ban_takes_and_the_refusals():
    bp = _bp()
    vocab = 2 ** 19
    x = np.zeros((2, vocab), dtype=np.float32)
    x[:, [5, vocab - 1, 70000]] = [[3.0, 2.5, 2.0]]
    logits = _place(x, torch.bfloat16)
    sequences = _dev([[9, 5, 9, 0], [9, vocab - 1, 9, 0]], torch.int64)
    counters = _dev([3, 3], torch.int32)
    got = bp.pick_token(logits, counters=counters, sequences=sequences, no_repeat_ngram_size=2)
    assert got.cpu().tolist() == [vocab - 1, 5]
    got = bp.pick_token(logits, counters=counters, sequences=sequences.clone(), no_repeat_ngram_size=2,
                        suppress_tokens=_dev([5, vocab - 1], torch.int32))
    assert got.cpu().tolist() == [70000, 70000]
    one = _dev([1], torch.int32)
    with pytest.raises(RuntimeError):                                  # two bitmaps of 64 KB next to the 68 112 static bytes
        bp.pick_token(logits, counters=counters, sequences=sequences.clone(), no_repeat_ngram_size=2, repetition_penalty=1.2)
    with pytest.raises(RuntimeError):
        bp.pick_token(_place(np.zeros((1, vocab + 1), dtype=np.float32), torch.bfloat16), counters=one,
                      sequences=_dev([[0]], torch.int64), no_repeat_ngram_size=1)
    with pytest.raises(RuntimeError):                                  # 8192 columns under a count penalty
        bp.pick_token(logits[:1, :4096], counters=one, sequences=torch.zeros((1, 8192), dtype=torch.int64, device=DEV),
                      frequency_penalty=0.5)
    with pytest.raises(RuntimeError):
        bp.pick_token(logits[:1, :4096], counters=one, sequences=torch.zeros((1, 64), dtype=torch.int64, device=DEV),
                      no_repeat_ngram_size=65)


# ---- capture and replay ---------------------------------------------------------------------------------------------------------------

def test_capture_and_replay_with_the_history_growing_on_the_device():
    bp = _bp()
    batch, vocab, steps, start = 6, 4096, 40, 3
    logits = _sampling_rows(batch, vocab, torch.bfloat16, seed=9)
    x = _host(logits)
    state = _state()
    prompt = torch.randint(0, vocab, (batch, start), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    suppress = [int(np.argmax(x[b])) for b in range(batch)]
    limits = dict(no_repeat_ngram_size=2, frequency_penalty=0.5, presence_penalty=0.25, penalty_begin=start)
    suppress_dev = _dev(suppress, torch.int32)

    def fresh():
        sequences = torch.full((batch, start + steps + 2), -1, dtype=torch.int64, device=DEV)
        sequences[:, :start] = prompt
        return sequences, torch.full((batch,), start - 1, dtype=torch.int32, device=DEV), torch.zeros(batch, dtype=torch.int64, device=DEV)

    def step(sequences, counters, tokens):                 # the length increment, then the pick: what a decode loop captures
        counters.add_(1)
        bp.pick_token(logits, True, 0.8, 8, 1.0, state, counters, tokens=tokens, sequences=sequences, repetition_penalty=1.5,
                      suppress_tokens=suppress_dev, **limits)

    sequences, counters, tokens = fresh()
    eager = []
    for _ in range(steps):
        step(sequences, counters, tokens)
        eager.append(tokens.clone())
    want_seq = sequences.clone()
    sequences, counters, tokens = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(sequences, counters, tokens)
    replayed = []
    for i in range(steps):
        graph.replay()
        replayed.append(tokens.clone())
    assert all(torch.equal(a, b) for a, b in zip(eager, replayed))
    assert torch.equal(sequences, want_seq) and (sequences[:, start + steps:] == -1).all()
    # and the restatement at every step, on the history as it stood: top_k = 8 of constant rows soon runs into its own counts and bans
    rows = want_seq.cpu().numpy()
    eps = R.epsilon(vocab)
    for i in range(steps):
        t = start + i
        for b in range(batch):
            z = L.values(x[b], 0.8, rows[b], t, vocab, repetition_penalty=1.5, suppress_tokens=suppress, **limits)
            R.assert_draw(int(rows[b, t]), z, R.kept_set(z, 8, 1.0), R.uniform(SEED, OFFSET, b, t), eps, what=(i, b))
    for b in range(batch):
        row = rows[b, :start + steps].tolist()
        assert len({(row[j], row[j + 1]) for j in range(len(row) - 1)}) == len(row) - 1 and suppress[b] not in row[start:], b


# ---- the generation loops -------------------------------------------------------------------------------------------------------------

PROMPT, MAX_LENGTH = 8, 40


def _ids(batch, seed=5):
    return torch.randint(0, VOCAB, (batch, PROMPT), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _teacher_forced_logits(model, seq):
    """Logits of every generated position of `seq`, by the calls of the cached loop itself (test_gpu_pick.py's, restated)."""
    from src.utils.generation import InferenceParams
    batch, n = seq.shape
    ip = InferenceParams(max_sequence_len=n, max_batch_size=batch)
    ip.lengths_per_sample = torch.zeros((batch,), dtype=torch.int32, device=DEV)
    out = {}
    with torch.inference_mode():
        out[PROMPT] = model(seq[:, :PROMPT].contiguous(), inference_params=ip).logits[:, -1].clone()
        ip.sequence_len_offset = PROMPT
        ip.lengths_per_sample.fill_(PROMPT)
        for t in range(PROMPT, n - 1):
            out[t + 1] = model(seq[:, t:t + 1].contiguous(), inference_params=ip).logits[:, -1].clone()
            ip.lengths_per_sample += 1
            ip.sequence_len_offset += 1
    return out


def _no_repeated_trigram(row):
    return len({tuple(row[j:j + 3]) for j in range(len(row) - 2)}) == len(row) - 2


@pytest.mark.parametrize('name', ['small', 'mini_k4'])
def test_generation_under_the_limits_eager_and_graphed(name):
    model = _model(name, seed=2)
    vocab = model.lm_head.weight.shape[0]
    ids = _ids(3)
    free = model.generate(ids, MAX_LENGTH, kv_cache=True, cg=True, device_pick=True)
    common = [int(t) for t in torch.bincount(free[:, PROMPT:].reshape(-1), minlength=vocab).topk(3).indices]
    kw = dict(kv_cache=True, no_repeat_ngram_size=3, suppress_tokens=common, frequency_penalty=0.5)
    limits = dict(no_repeat_ngram_size=3, suppress_tokens=common, frequency_penalty=0.5, penalty_begin=PROMPT)
    eager = model.generate(ids, MAX_LENGTH, **kw)
    graph = model.generate(ids, MAX_LENGTH, cg=True, **kw)
    assert eager.shape == (3, MAX_LENGTH - 1) and torch.equal(eager, graph) and torch.equal(eager[:, :PROMPT], ids)
    assert not torch.equal(eager, free), 'the limits changed nothing: a weak test'
    drawn = model.sample(ids, MAX_LENGTH, rng_state=_state(), top_k=10, temperature=0.9, **kw)
    drawn_graph = model.sample(ids, MAX_LENGTH, cg=True, rng_state=_state(), top_k=10, temperature=0.9, **kw)
    assert torch.equal(drawn, drawn_graph)
    for out in (eager, drawn):
        assert all(_no_repeated_trigram(r.tolist()) for r in out)
        assert not np.isin(out[:, PROMPT:].cpu().numpy(), common).any()
    # every step against the restatement on the logits the pick saw: the teacher-forced run makes the calls of the loop itself
    # (same kernels, same shapes, no atomics), so its logits are the loop's bit for bit and a greedy pick is decided wherever the
    # two best values differ at all; where they tie, the pick must be one of the tied ids
    lg, ld = _teacher_forced_logits(model, eager), _teacher_forced_logits(model, drawn)
    rows_g, rows_d = eager.cpu().numpy(), drawn.cpu().numpy()
    eps = R.epsilon(vocab)
    undecided = picks = 0
    for t in range(PROMPT, MAX_LENGTH - 1):
        xg, xd = _host(lg[t]), _host(ld[t])
        for b in range(3):
            v = L.values(xg[b], None, rows_g[b], t, vocab, **limits)
            top2 = np.sort(v)[-2:]
            picks += 1
            if top2[1] > top2[0]:
                assert int(rows_g[b, t]) == int(np.argmax(v)), (t, b)
            else:
                undecided += 1
                assert v[int(rows_g[b, t])] == top2[1], (t, b)
            z = L.values(xd[b], 0.9, rows_d[b], t, vocab, **limits)
            R.assert_draw(int(rows_d[b, t]), z, R.kept_set(z, 10, 1.0), R.uniform(SEED, OFFSET, b, t), eps, what=(t, b))
    assert undecided <= 0.05 * picks, f'{undecided} of {picks} greedy picks undecided'
