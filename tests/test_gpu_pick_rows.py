"""GPU: bp_pick_token_lim_rows (csrc/pick_token_rows.hip), the limited pick whose penalty_begin and min_length come per row --
arrays that hold the scalar equal bp_pick_token_lim bit for bit, every kind of begin on one call with the counts read out
exactly, the per-row minimum around its edge, the restatement of tests/pick_lim_ref.py called with every row's own values,
canaries round every output, capture and replay with the history growing on the device."""
import numpy as np
import pytest
import torch

import pick_lim_ref as L
import pick_ref as R
from decode_support import DEV, _bp

pytestmark = pytest.mark.gpu

SEED, OFFSET = 1234, 77
INF, NAN = float('inf'), float('nan')
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
CANARY = -9


def _state(seed=SEED, offset=OFFSET):
    return torch.tensor([seed, offset], dtype=torch.int64, device=DEV)


def _place(rows, dtype, pad=0, misalign=0):
    """(B, vocab) host fp32 rows -> a device tensor of `dtype` with row stride vocab + pad whose base is `misalign` elements
    behind a 16-byte boundary (test_gpu_pick_limits.py's, restated)."""
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


# ---- arrays that hold the scalar: bp_pick_token_lim, bit for bit ------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('vocab', [100, 4099, 50264])
def test_arrays_holding_the_scalar_equal_the_limited_pick_bit_for_bit(vocab, dtype):
    bp = _bp()
    batch, cols, begin, minimum = 5, 24, 6, 9
    rng = np.random.default_rng(vocab)
    x = (2.0 * rng.standard_normal((batch, vocab))).astype(np.float32)
    x[1] = np.round(x[1] * 2) / 2                                  # ties
    x[2, vocab // 3] = NAN                                         # a degenerate row
    logits = _place(x, DTYPES[dtype], pad=13, misalign=3 if dtype != 'fp32' else 1)
    counters = _dev([3, 8, 9, 23, 30], torch.int32)                # below, around and above the minimum; 30: the write is skipped
    seq = rng.integers(0, min(vocab, 12), size=(batch, cols)).astype(np.int64)
    seq[:, 3] = -1
    entry = _dev([0, 0, 0, 0, 1], torch.int32)                     # the last row is finished on entry
    eos = int(np.argmax(x[0]))                                     # masked in row 0 (c = 3 < 9): the mask decides its greedy pick
    begins, mins = _dev([begin] * batch, torch.int32), _dev([minimum] * batch, torch.int32)
    common = dict(rng_state=_state(), counters=counters, return_stats=True, repetition_penalty=1.3, eos_token_id=eos, pad_token_id=1,
                  no_repeat_ngram_size=2, frequency_penalty=0.5, presence_penalty=0.25,
                  suppress_tokens=_dev([int(np.argmax(x[3])), -1, vocab], torch.int32))
    for sampling in (dict(do_sample=False), dict(do_sample=True, temperature=0.7, top_k=40, top_p=0.95)):
        outs = []
        for per_row in (dict(penalty_begin=begin, min_length=minimum), dict(penalty_begin=begins, min_length=minimum),
                        dict(penalty_begin=begin, min_length=mins), dict(penalty_begin=begins, min_length=mins)):
            assert bp.pick_form(**per_row) == ('lim' if len(outs) == 0 else 'rows')
            sequences, finished = _dev(seq, torch.int64), entry.clone()
            tokens, stats = bp.pick_token(logits, sequences=sequences, finished=finished, **common, **sampling, **per_row)
            outs.append((tokens, _bits(stats), sequences, finished))
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert torch.equal(a, b), (sampling, a.tolist(), b.tolist())
        assert outs[0][0][0].item() != eos
    assert begins.tolist() == [begin] * batch and mins.tolist() == [minimum] * batch       # only read


# ---- every kind of begin on one call, the counts exact -----------------------------------------------------------------------------------
#
# Logits 8.0 and penalties 0.5 / 0.25 (test_gpu_pick_limits.py): every intermediate has a few mantissa bits, so the values are
# exact in fp32 and in fp16 (the needle of the largest count, 513, is 265: ten bits).

def _begin_cases(cols):
    """(counter, begin): 0, mid-history, == Lh, > Lh, negative, a history cut short of the columns, and c > seq_cols."""
    mid = cols // 2 - 1
    return [(cols, 0), (cols, mid), (cols, cols), (cols, cols + 5), (cols, -3), (cols - 2, mid), (cols - 2, cols - 3),
            (cols - 2, cols - 2), (cols, cols - 2), (cols + 40, cols - 1), (cols + 40, -2 ** 31), (cols, 2 ** 31 - 1), (0, 0)]


@pytest.mark.parametrize('dtype', ['fp16', 'fp32'])
@pytest.mark.parametrize('cols', [8, 1025])
def test_per_row_begins_are_exact_through_stats_and_needles(cols, dtype):
    bp = _bp()
    vocab, fp, pp = 4099, 0.5, 0.25
    d, e = 77, 3001                                                # d fills the even columns, e the odd ones
    history = [d if j % 2 == 0 else e for j in range(cols)]
    rows = []
    for counter, begin in _begin_cases(cols):
        h = L.clamped_history(history, counter)
        n = L.counts(h, begin, vocab)[d]
        assert n == len([j for j in range(max(begin, 0), len(h)) if j % 2 == 0])
        for sign, wins in ((+0.25, True), (-0.25, False)):
            x = np.full(vocab, 8.0, dtype=np.float32)
            x[d] = 8.0 + ((fp * n + pp) if n else 0.0) + sign      # 8.25 after the penalty wins, 7.75 loses to a non-member at 8
            rows.append((counter, begin, n, x, wins))
    assert {r[2] for r in rows} >= {0, 1, (cols + 1) // 2} and len({r[2] for r in rows}) >= 4
    logits = _place(np.stack([r[3] for r in rows]), DTYPES[dtype], pad=3, misalign=1)
    sequences = _dev(np.array([history] * len(rows)), torch.int64)
    kw = dict(counters=_dev([r[0] for r in rows], torch.int32), frequency_penalty=fp, presence_penalty=pp,
              penalty_begin=_dev([r[1] for r in rows], torch.int32))
    greedy = bp.pick_token(logits, sequences=sequences.clone(), **kw)
    _, stats = bp.pick_token(logits, True, 1.0, 0, 1.0, _state(), sequences=sequences.clone(), return_stats=True, **kw)
    greedy, stats = greedy.cpu().tolist(), stats.cpu().numpy()
    for r, (counter, begin, n, x, wins) in enumerate(rows):
        z = L.values(x, None, history, counter, vocab, frequency_penalty=fp, presence_penalty=pp, penalty_begin=max(begin, 0))
        assert z[d] == (8.25 if wins else 7.75), (r, z[d])
        assert greedy[r] == R.greedy(z) and (greedy[r] == d) == wins, (r, counter, begin, n, greedy[r])
        assert stats[r, 2] == vocab and stats[r, 0] == z.min(), (r, counter, begin, stats[r], z.min())   # e's count is in z.min()


def test_per_row_minimum_at_its_edge():
    bp = _bp()
    vocab, eos, runner_up = 4099, 4098, 17
    x = np.zeros((8, vocab), dtype=np.float32)
    x[:, eos], x[:, runner_up] = 3.0, 2.0
    logits = _place(x, torch.bfloat16, pad=5, misalign=1)
    #             c = m - 1, m, m + 1;  a negative and a zero minimum at c = 0;  c = 0 below a minimum;  a huge minimum;  c < 0
    counters = _dev([6, 7, 8, 0, 0, 0, 50, -1], torch.int32)
    mins = _dev([7, 7, 7, -5, 0, 1, 2 ** 31 - 1, 0], torch.int32)
    masked = [True, False, False, False, False, True, True, True]
    sequences = torch.zeros((8, 64), dtype=torch.int64, device=DEV)
    for begin in (0, _dev([0] * 8, torch.int32)):
        finished = torch.zeros(8, dtype=torch.int32, device=DEV)
        got = bp.pick_token(logits, counters=counters, sequences=sequences.clone(), eos_token_id=eos, finished=finished,
                            min_length=mins, penalty_begin=begin)
        assert got.cpu().tolist() == [runner_up if m else eos for m in masked]
        assert finished.cpu().tolist() == [0 if m else 1 for m in masked]
        # top_k = vocab - 1 keeps every finite value: all but the masked EOS, or, by the tie at 0, the whole row
        _, stats = bp.pick_token(logits, True, 1.0, vocab - 1, 1.0, _state(), counters, sequences=sequences.clone(), eos_token_id=eos,
                                 finished=torch.zeros(8, dtype=torch.int32, device=DEV), min_length=mins, penalty_begin=begin,
                                 return_stats=True)
        assert stats[:, 2].cpu().tolist() == [float(vocab - 1 if m else vocab) for m in masked]


@pytest.mark.parametrize('vocab,dtype', [(100, 'fp32'), (4099, 'bf16'), (50264, 'fp16')])
def test_kept_set_and_draw_with_every_rows_own_values(vocab, dtype):
    bp = _bp()
    batch, cols = 12, 1025
    rng = np.random.default_rng(vocab + 5)
    x = (2.0 * rng.standard_normal((batch, vocab))).astype(np.float32)
    logits = _place(x, DTYPES[dtype], pad=8)
    x = _host(logits)
    seq = rng.integers(0, min(vocab, 40), size=(batch, cols)).astype(np.int64)
    seq[:, 3], seq[:, 4] = -1, vocab
    counters = np.array([0, 1, 63, 64, 65, 1024, 1025, 2000, 7, 500, 500, 500], dtype=np.int32)
    begins = np.array([0, 5, 10, 64, 30, 1000, 0, 1025, -4, 0, 250, 499], dtype=np.int32)
    mins = np.array([0, 2, 63, 70, 65, 0, 2000, 0, -1, 500, 501, 499], dtype=np.int32)
    eos = int(np.argmax(x[3]))
    limits = dict(no_repeat_ngram_size=2, frequency_penalty=0.5, presence_penalty=0.25)
    sequences = _dev(seq, torch.int64)
    args = dict(rng_state=_state(), counters=_dev(counters, torch.int32), sequences=sequences, repetition_penalty=1.2,
                eos_token_id=eos, finished=torch.zeros(batch, dtype=torch.int32, device=DEV),
                penalty_begin=_dev(begins, torch.int32), min_length=_dev(mins, torch.int32), **limits)
    tokens, stats = bp.pick_token(logits, True, 0.8, 50, 1.0, return_stats=True, **args)
    greedy = bp.pick_token(logits, **{**args, 'sequences': _dev(seq, torch.int64),
                                      'finished': torch.zeros(batch, dtype=torch.int32, device=DEV)})
    tokens, stats, greedy = tokens.cpu().tolist(), stats.cpu().numpy(), greedy.cpu().tolist()
    eps = R.epsilon(vocab)
    for b in range(batch):
        kw = dict(repetition_penalty=1.2, eos_token_id=eos, min_length=max(int(mins[b]), 0),
                  penalty_begin=max(int(begins[b]), 0), **limits)
        c = int(counters[b])
        assert greedy[b] == R.greedy(L.values(x[b], None, seq[b], c, vocab, **kw)), b
        z = L.values(x[b], 0.8, seq[b], c, vocab, **kw)
        u = R.uniform(SEED, OFFSET, b, c)
        assert stats[b, 3] == np.float32(u) and not R.degenerate(z), b
        keep = R.kept_set(z, 50, 1.0)
        assert int(stats[b, 2]) == int(keep.sum()) and stats[b, 0] == z[keep].min(), (b, stats[b], int(keep.sum()), z[keep].min())
        R.assert_draw(tokens[b], z, keep, u, eps, what=(vocab, dtype, b))
    assert greedy[3] != eos and mins[3] > counters[3]              # the fourth row's best id is its masked EOS


# ---- canaries round every output -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('do_sample', [False, True])
def test_nothing_is_written_outside_the_outputs(do_sample):
    bp = _bp()
    batch, vocab, cols, stride = 5, 4099, 8, 12
    rng = np.random.default_rng(2)
    logits = _place((2.0 * rng.standard_normal((batch, vocab))).astype(np.float32), torch.bfloat16, pad=3, misalign=1)
    seq_w = torch.full((batch + 2, stride), CANARY, dtype=torch.int64, device=DEV)
    seq_w[1:-1, :cols] = _dev(rng.integers(0, 9, size=(batch, cols)), torch.int64)
    tok_w = torch.full((batch + 2, 3), CANARY, dtype=torch.int64, device=DEV)        # tokens: column 1, stride 3
    stats_w = torch.full((batch + 2, 4), float(CANARY), dtype=torch.float32, device=DEV)
    fin_w = torch.full((batch + 2,), CANARY, dtype=torch.int32, device=DEV)
    fin_w[1:-1] = _dev([0, 0, 1, 0, 0], torch.int32)
    counters = _dev([5, 7, 3, 8, 20], torch.int32)                                    # 8 and 20: no column to write
    begins, mins = _dev([2, 0, 1, -1, 9], torch.int32), _dev([9, 0, 0, 3, -2], torch.int32)
    suppress = _dev([1, 2], torch.int32)
    inputs = [t.clone() for t in (counters, begins, mins, suppress)]
    before = seq_w.clone()
    eos, state = 4, _state()
    bp._call('bp_pick_token_lim_rows', DEV, logits.data_ptr(), tok_w[1:-1, 1].data_ptr(), seq_w[1:-1].data_ptr(),
             stats_w[1:-1].data_ptr(), state.data_ptr(), counters.data_ptr(), fin_w[1:-1].data_ptr(), batch, vocab,
             logits.stride(0), 3, stride, cols, int(do_sample), 0.9, 20, 0.95, 1.3, eos, 6, 0, 2, 0.5, 0.25, 0,
             suppress.data_ptr(), 2, begins.data_ptr(), mins.data_ptr(), 1)
    torch.cuda.synchronize()
    tokens = tok_w[1:-1, 1].cpu().tolist()
    assert all(0 <= t < vocab for t in tokens) and tokens[2] == 6                     # the finished row holds the pad
    tok_w[1:-1, 1] = CANARY
    assert (tok_w == CANARY).all()
    want = before.clone()
    for b, c in enumerate(counters.tolist()):
        if c < cols:
            want[1 + b, c] = tokens[b]
    assert torch.equal(seq_w, want)
    assert (stats_w[0] == CANARY).all() and (stats_w[-1] == CANARY).all() and (stats_w[1:-1] != CANARY).all()
    assert fin_w[0].item() == CANARY and fin_w[-1].item() == CANARY
    assert fin_w[1:-1].cpu().tolist() == [int(f or t == eos) for f, t in zip([0, 0, 1, 0, 0], tokens)]
    for now, then in zip((counters, begins, mins, suppress), inputs):
        assert torch.equal(now, then)


# ---- capture and replay ---------------------------------------------------------------------------------------------------------------

def test_capture_and_replay_with_the_counters_growing_on_the_device():
    bp = _bp()
    batch, vocab, steps = 5, 4099, 21                                # one captured step, 20 replays behind it
    starts = [1, 3, 5, 8, 8]                                         # the rows begin at different positions
    rng = np.random.default_rng(9)
    logits = _place((2.0 * rng.standard_normal((batch, vocab))).astype(np.float32), torch.bfloat16, pad=8)
    x = _host(logits)
    state = _state()
    eos = int(np.argmax(x[0]))
    begins = _dev(starts, torch.int32)
    mins = _dev([s + 4 for s in starts], torch.int32)                # four new tokens before a row may end
    limits = dict(no_repeat_ngram_size=2, frequency_penalty=0.5, presence_penalty=0.25)
    cols = max(starts) + steps + 2
    prompt = rng.integers(0, vocab, size=(batch, cols))

    def fresh():
        sequences = torch.full((batch, cols), -1, dtype=torch.int64, device=DEV)
        for b, s in enumerate(starts):
            sequences[b, :s] = _dev(prompt[b, :s], torch.int64)
        counters = _dev([s - 1 for s in starts], torch.int32)
        return sequences, counters, torch.zeros(batch, dtype=torch.int64, device=DEV), torch.zeros(batch, dtype=torch.int32, device=DEV)

    def step(sequences, counters, tokens, finished):                 # the length increment, then the pick: what a decode loop captures
        counters.add_(1)
        bp.pick_token(logits, True, 0.8, 8, 1.0, state, counters, tokens=tokens, sequences=sequences, repetition_penalty=1.5,
                      eos_token_id=eos, pad_token_id=2, finished=finished, penalty_begin=begins, min_length=mins, **limits)

    buffers = fresh()
    eager = []
    for _ in range(steps):
        step(*buffers)
        eager.append(buffers[2].clone())
    want_seq, want_fin = buffers[0].clone(), buffers[3].clone()
    buffers = fresh()
    step(*buffers)                                                   # the first step eagerly, as the loops run it
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(*buffers)
    replayed = [buffers[2].clone()]
    for _ in range(steps - 1):
        graph.replay()
        replayed.append(buffers[2].clone())
    assert all(torch.equal(a, b) for a, b in zip(eager, replayed))
    assert torch.equal(buffers[0], want_seq) and torch.equal(buffers[3], want_fin)
    # and the restatement with every row's own begin and minimum, until the row ends
    rows = want_seq.cpu().numpy()
    eps = R.epsilon(vocab)
    ended = 0
    for b, s in enumerate(starts):
        assert (rows[b, s + steps:] == -1).all()
        for t in range(s, s + steps):
            z = L.values(x[b], 0.8, rows[b], t, vocab, repetition_penalty=1.5, eos_token_id=eos, min_length=s + 4,
                         penalty_begin=s, **limits)
            R.assert_draw(int(rows[b, t]), z, R.kept_set(z, 8, 1.0), R.uniform(SEED, OFFSET, b, t), eps, what=(b, t))
            assert t >= s + 4 or int(rows[b, t]) != eos
            if int(rows[b, t]) == eos:
                assert (rows[b, t + 1:s + steps] == 2).all() and want_fin[b].item() == 1
                ended += 1
                break
    print(f'{ended} of {batch} rows ended at their EOS')
