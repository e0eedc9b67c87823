"""GPU: bp_pick_token_phrases (csrc/pick_token_phrases.hip), the row-limited pick with banned phrases and stop phrases -- without
phrases it equals bp_pick_token_lim_rows bit for bit; every edge of the two matches on exact designs (greedy rows, and sampled
rows whose logits are needles 30 apart, so that the draw is decided for any u) against the restatement of
tests/pick_phrase_ref.py, with canaries round every output and the phrase arrays compared after the call; phrase lists the
device must ignore; lists of 1024 phrases; capture and replay with the history growing on the device; generation end to end."""
import numpy as np
import pytest
import torch

import pick_lim_ref as L
import pick_phrase_ref as P
import pick_ref as R
from decode_support import DEV, VOCAB as MODEL_VOCAB, _bp, _model

pytestmark = pytest.mark.gpu

SEED, OFFSET = 1234, 77
INF, NAN = float('inf'), float('nan')
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
CODES = {'fp16': 0, 'bf16': 1, 'fp32': 2}
CANARY = -9
COLS, STRIDE = 80, 83
SHAPES = [(100, 'fp32'), (100, 'bf16'), (4099, 'bf16'), (4099, 'fp32')]


def _state(seed=SEED, offset=OFFSET):
    return torch.tensor([seed, offset], dtype=torch.int64, device=DEV)


def _place(rows, dtype, pad=0, misalign=0):
    """(B, vocab) host fp32 rows -> a device tensor of `dtype` with row stride vocab + pad whose base is `misalign` elements
    behind a 16-byte boundary (test_gpu_pick_rows.py's, restated)."""
    rows = torch.as_tensor(rows, dtype=torch.float32)
    b, v = rows.shape
    flat = torch.zeros(b * (v + pad) + 16, dtype=dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = flat[misalign:misalign + b * (v + pad)].view(b, v + pad)[:, :v]
    view.copy_(rows.to(dtype))
    return view


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _needles(vocab, first, second=None, base=0.0):
    """A row that is `base` everywhere but 60 at `first` and 30 at `second`: the argmax, and the draw for any u, is `first`,
    or `second` once `first` is banned (what lies 30 below the maximum has no mass in 40-bit fixed point: e^-30 2^40 < 1)."""
    x = np.full(vocab, base, dtype=np.float32)
    if second is not None:
        x[second] = 30.0
    x[first] = 60.0
    return x


def _packed(phrases):
    """(ids, offsets, total) of a list of lists, or of an (ids, offsets[, total]) triple given as arrays (broken lists)."""
    if isinstance(phrases, tuple):
        ids, offsets = phrases[:2]
        return list(ids), list(offsets), phrases[2] if len(phrases) > 2 else len(ids)
    ids, offsets = P.pack(phrases if phrases is not None else [])
    return ids.tolist(), offsets.tolist(), len(ids)


def _run(vocab, dtype, do_sample, rows, ban=None, stop=None, eos=-1, pad=1, outputs=True, **limits):
    """One call of bp_pick_token_phrases on `rows` -- dicts of x (vocab,), h (the row of `sequences`, a list), c, begin, minimum,
    finished -- through the raw ABI, every output inside canaries; everything it wrote, and everything it must not have written,
    against the restatement.  Returns (tokens, reasons as the restatement gives them)."""
    bp = _bp()
    batch = len(rows)
    assert batch <= 16
    logits = _place(np.stack([r['x'] for r in rows]), DTYPES[dtype], pad=5, misalign=3 if dtype != 'fp32' else 1)
    x = logits.float().cpu().numpy()
    seq = np.full((batch, COLS), 2, dtype=np.int64)
    for b, r in enumerate(rows):
        seq[b, :len(r['h'])] = r['h']
    seq_w = torch.full((batch + 2, STRIDE), CANARY, dtype=torch.int64, device=DEV)
    seq_w[1:-1, :COLS] = _dev(seq, torch.int64)
    tok_w = torch.full((batch + 2, 3), CANARY, dtype=torch.int64, device=DEV)          # tokens: column 1, stride 3
    stats_w = torch.full((batch + 2, 4), float(CANARY), dtype=torch.float32, device=DEV)
    fin_w, ends_w, why_w = (torch.full((batch + 2,), CANARY, dtype=torch.int32, device=DEV) for _ in range(3))
    entry = [int(r.get('finished', 0)) for r in rows]
    fin_w[1:-1] = _dev(entry, torch.int32)
    counters = _dev([r.get('c', len(r['h'])) for r in rows], torch.int32)
    begins, mins = _dev([r.get('begin', 0) for r in rows], torch.int32), _dev([r.get('minimum', 0) for r in rows], torch.int32)
    lists = []
    for phrases in (ban, stop):
        ids, offsets, total = _packed(phrases)
        lists.append((_dev(ids if ids else [0], torch.int32), _dev(offsets, torch.int32), len(offsets) - 1, total))
    inputs = [counters, begins, mins] + [t for ls in lists for t in ls[:2]]
    kept = [t.clone() for t in inputs]
    before = seq_w.clone()
    state = _state()
    phrase_args = [a for ids, offsets, n, total in lists
                   for a in ((ids.data_ptr(), offsets.data_ptr(), n, total) if n else (None, None, 0, 0))]
    bp._call('bp_pick_token_phrases', DEV, logits.data_ptr(), tok_w[1:-1, 1].data_ptr(), seq_w[1:-1].data_ptr(),
             stats_w[1:-1].data_ptr(), state.data_ptr(), counters.data_ptr(), fin_w[1:-1].data_ptr(), batch, vocab,
             logits.stride(0), 3, STRIDE, COLS, int(do_sample), 1.0, 2, 1.0, 1.0, eos, pad, 0,
             limits.get('no_repeat_ngram_size', 0), 0.0, 0.0, 0, None, 0, begins.data_ptr(), mins.data_ptr(), *phrase_args,
             ends_w[1:-1].data_ptr() if outputs else None, why_w[1:-1].data_ptr() if outputs else None, CODES[dtype])
    torch.cuda.synchronize()
    for now, then in zip(inputs, kept):
        assert torch.equal(now, then)                                                   # only read
    ban_p, stop_p = P.unpack(*_packed(ban)), P.unpack(*_packed(stop))
    tokens, stats = tok_w[1:-1, 1].cpu().tolist(), stats_w[1:-1].cpu().numpy()
    want_seq, reasons = before.clone(), []
    for b, r in enumerate(rows):
        c, fin = int(counters[b]), bool(entry[b])
        begin, minimum = max(r.get('begin', 0), 0), max(r.get('minimum', 0), 0)
        tok, why = P.step(x[b], seq[b], c, fin, begin, minimum, ban_p, stop_p, eos=eos if eos >= 0 else None, pad=pad, **limits)
        reasons.append(why)
        assert tokens[b] == tok, (b, tokens[b], tok)
        if 0 <= c < COLS:
            want_seq[1 + b, c] = tok
        assert fin_w[1 + b].item() == int(fin or why is not None), (b, why)
        if outputs:
            assert (ends_w[1 + b].item(), why_w[1 + b].item()) == ((CANARY, CANARY) if why is None else (c + 1, why)), (b, why)
        u = np.float32(R.uniform(SEED, OFFSET, b, c)) if do_sample else np.float32(0.0)
        if fin:
            want = [0.0, 0.0, 0.0, u]
        else:
            z = P.values(x[b], None, seq[b], c, vocab, ban_p, eos_token_id=eos if eos >= 0 else None, min_length=minimum,
                         penalty_begin=begin, **limits)
            top = np.sort(z)[-2:]
            assert top[1] == -INF or top[1] - top[0] >= 30.0, 'not an exact design'     # decided for any u
            if not do_sample or R.degenerate(z):
                want = [z.max(), z.max(), 1.0, u]
            else:
                keep = R.kept_set(z, 2, 1.0)
                want = [z[keep].min(), z.max(), float(keep.sum()), u]                   # the rest of the kept set has no mass
        assert stats[b].view(np.int32).tolist() == np.array(want, dtype=np.float32).view(np.int32).tolist(), (b, stats[b], want)
    assert torch.equal(seq_w, want_seq)
    tok_w[1:-1, 1] = CANARY
    assert (tok_w == CANARY).all() and (stats_w[0] == CANARY).all() and (stats_w[-1] == CANARY).all()
    for w in (fin_w, ends_w, why_w):
        assert w[0].item() == CANARY and w[-1].item() == CANARY
    if not outputs:
        assert (ends_w == CANARY).all() and (why_w == CANARY).all()
    return tokens, reasons


# ---- without phrases: bp_pick_token_lim_rows, bit for bit ----------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('vocab', [100, 50264])
def test_without_phrases_the_pick_equals_the_row_limited_one_bit_for_bit(vocab, dtype):
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
    x = logits.float().cpu().numpy()
    eos = int(np.nanargmax(x[1]))                                  # row 1 sits at its own minimum, 8: its EOS id is not masked
    begins, mins = _dev([begin] * batch, torch.int32), _dev([minimum, 8, 9, 9, 9], torch.int32)
    common = dict(rng_state=_state(), counters=counters, return_stats=True, repetition_penalty=1.3, eos_token_id=eos, pad_token_id=1,
                  no_repeat_ngram_size=2, frequency_penalty=0.5, presence_penalty=0.25,
                  suppress_tokens=_dev([int(np.argmax(x[3])), -1, vocab], torch.int32), penalty_begin=begins, min_length=mins)
    for sampling in (dict(do_sample=False), dict(do_sample=True, temperature=0.7, top_k=40, top_p=0.95)):
        outs = []
        for phrases in (dict(), dict(bad_words_ids=[]), dict(stop_sequences=[]), dict(bad_words_ids=[], stop_sequences=[])):
            assert bp.pick_form(penalty_begin=begins, **phrases) == ('rows' if len(outs) == 0 else 'phrases')
            sequences, finished = _dev(seq, torch.int64), entry.clone()
            tokens, stats = bp.pick_token(logits, sequences=sequences, finished=finished, **common, **sampling, **phrases)
            outs.append((tokens, _bits(stats), sequences, finished))
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert torch.equal(a, b), (sampling, a.tolist(), b.tolist())
    assert outs[0][3].tolist()[4] == 1 and outs[0][0][4].item() == 1


# ---- banned phrases ------------------------------------------------------------------------------------------------------------------

def _long(n, salt):
    """n history ids in 30..36 with no period that a shifted copy would match."""
    return [30 + (i * i + salt * i) % 7 for i in range(n)]


@pytest.mark.parametrize('do_sample', [False, True])
@pytest.mark.parametrize('vocab,dtype', SHAPES)
def test_ban_phrases_at_every_edge(vocab, dtype, do_sample):
    A, B = vocab - 3, vocab - 6                                      # the needles: in the run of the row's last wave
    long63 = _long(63, 1)
    everything = list(range(vocab)) if vocab == 100 else [0, 1, 2, 50, A, B, vocab - 1]
    ban = [[vocab - 9],                                              # 0  L = 1: always
           [5, A],                                                   # 1  L = 2
           [7, 8, A],                                                # 2  L = 3
           long63 + [A],                                             # 3  L = 64
           [11, 0], [12, vocab - 1],                                 # 4, 5  the first and the last id of the vocabulary
           [13, -1], [13, vocab],                                    # 6, 7  last ids outside it: nothing to ban, nothing written
           [-1, 14, A], [vocab + 5, 15, A],                          # 8, 9  raw values in the prefix
           ] + [[16, t] for t in everything]                         # a row left without a value
    rest = np.full(vocab, -INF, dtype=np.float32)
    rest[everything] = np.linspace(1.0, 2.0, len(everything))
    rest[everything[-1]] = 60.0
    rows = [dict(x=_needles(vocab, vocab - 9, B), h=[1, 2, 3]),                   # L = 1 bans the argmax
            dict(x=_needles(vocab, vocab - 9, B), h=[], c=0),                     # ... with no history at all
            dict(x=_needles(vocab, A, B), h=[4, 5]),                              # L = 2
            dict(x=_needles(vocab, A, B), h=[5]),                                 # ... its prefix begins at column 0
            dict(x=_needles(vocab, A, B), h=[4, 6]),                              # ... and does not match
            dict(x=_needles(vocab, A, B), h=[5, 4, 5], begin=3),                  # the prefix lies in the prompt
            dict(x=_needles(vocab, A, B), h=[8]),                                 # a history shorter than L - 1 = 2
            dict(x=_needles(vocab, A, B), h=[7, 8]),                              # L = 3 from column 0
            dict(x=_needles(vocab, A, B), h=long63),                              # L = 64 from column 0
            dict(x=_needles(vocab, A, B), h=long63[1:]),                          # one entry short of it
            dict(x=_needles(vocab, A, B), h=[9] * 10 + long63),                   # L = 64 at the end of a longer history
            dict(x=_needles(vocab, 0, B), h=[3, 11]),                             # id 0
            dict(x=_needles(vocab, vocab - 1, B), h=[3, 12]),                     # id vocab - 1
            dict(x=_needles(vocab, A, B), h=[3, 13]),                             # last ids -1 and vocab
            dict(x=_needles(vocab, A, B), h=[3, -1, 14]),                         # -1 in the prefix
            dict(x=_needles(vocab, A, B), h=[3, vocab + 5, 15])]                  # an id >= vocab in the prefix
    tokens, _ = _run(vocab, dtype, do_sample, rows, ban=ban)
    assert tokens == [B, B, B, B, A, B, A, B, B, A, B, B, B, A, B, B]
    rows = [dict(x=rest, h=[16]),                                                 # every value banned: index 0
            dict(x=rest, h=[15]),                                                 # ... not banned: the largest
            dict(x=_needles(vocab, A, B), h=[5] * COLS, c=COLS),                  # the history is the whole row
            dict(x=_needles(vocab, A, B), h=[4] * (COLS - 1) + [5], c=COLS + 7),  # ... clamped to it
            dict(x=_needles(vocab, A, B), h=[4, 5], c=-3),                        # no history
            dict(x=_needles(vocab, A, B), h=[4, 5], finished=1)]                  # finished on entry: the pad
    tokens, _ = _run(vocab, dtype, do_sample, rows, ban=ban)
    assert tokens == [0, everything[-1], B, B, A, 1]


@pytest.mark.parametrize('do_sample', [False, True])
@pytest.mark.parametrize('vocab,dtype', [(100, 'bf16'), (4099, 'fp32')])
def test_phrases_with_broken_offsets_are_ignored(vocab, dtype, do_sample):
    A, B = vocab - 3, vocab - 6
    ids = [A] * 70                                                   # whatever a broken phrase were taken for, it would ban or stop at A
    rows = [dict(x=_needles(vocab, A, B), h=[A] * 70), dict(x=_needles(vocab, A, B), h=[])]
    #          end < begin  negative  decreasing  beyond the ids  ...      65 and 66 ids
    offsets = [0, -1,       2,        1,          200,            3,       68, 2, 70, 5, 2 ** 31 - 1, -2 ** 31, 0]
    assert P.unpack(ids, offsets) == [None] * (len(offsets) - 1)
    for total, offs in ((70, offsets), (2, [0, 1 + 2, 3, 3 + 1])):   # a total below the array's length bounds the offsets, too
        tokens, reasons = _run(vocab, dtype, do_sample, rows, ban=(ids, offs, total), stop=(ids, offs, total))
        assert tokens == [A, A] and reasons == [None, None]
    # the same ids behind sound offsets: the test has teeth
    tokens, reasons = _run(vocab, dtype, do_sample, rows, ban=(ids, [0, 3, 4], 70))
    assert tokens == [B, B]
    tokens, reasons = _run(vocab, dtype, do_sample, rows, stop=(ids, [0, 0, 64, 65], 70))
    assert tokens == [A, A] and reasons == [2, 3]


# ---- stop phrases --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('do_sample', [False, True])
@pytest.mark.parametrize('vocab,dtype', SHAPES)
def test_stop_phrases_at_every_edge(vocab, dtype, do_sample):
    T, U, EOS, Y, B = vocab - 3, vocab - 5, vocab - 7, vocab - 2, vocab - 11
    long63 = _long(63, 2)
    stop = [[21, 22, T], [22, T], [U], [23, EOS], long63 + [Y], [T, T, T]]
    rows = [dict(x=_needles(vocab, T, B), h=[3, 21, 22]),                         # two phrases end here: the lower index
            dict(x=_needles(vocab, T, B), h=[3, 21, 22], begin=1),                # the longer one begins at the row's begin
            dict(x=_needles(vocab, T, B), h=[3, 21, 22], begin=2),                # ... one column in front of it
            dict(x=_needles(vocab, T, B), h=[3, 21, 22], begin=3),                # nothing lies behind the begin
            dict(x=_needles(vocab, T, B), h=[3, 21, 22], minimum=3),              # c == m
            dict(x=_needles(vocab, T, B), h=[3, 21, 22], minimum=4),              # c == m - 1
            dict(x=_needles(vocab, U, B), h=[3, 4]),                              # L = 1
            dict(x=_needles(vocab, U, B), h=[], c=0),                             # c = 0
            dict(x=_needles(vocab, T, B), h=[], c=0),                             # ... and a phrase that would begin in front of column 0
            dict(x=_needles(vocab, EOS, B), h=[3, 23]),                           # the EOS id that completes a phrase: reason 0
            dict(x=_needles(vocab, T, B), h=[3, 21, 22], finished=1),             # finished on entry
            dict(x=_needles(vocab, T, B), h=[4] * (COLS - 2) + [21, 22], c=COLS), # no column for the token: no match
            dict(x=_needles(vocab, EOS, B), h=[4] * COLS, c=COLS + 2),            # ... but the EOS id still ends the row
            dict(x=_needles(vocab, T, B), h=[3, 21, 22], begin=-7, minimum=-3),   # negative values count as 0
            dict(x=_needles(vocab, Y, B), h=[1, 2, 3, 4, 5] + long63, begin=5),   # L = 64, begins at the row's begin
            dict(x=_needles(vocab, Y, B), h=[1, 2, 3, 4, 5] + long63, begin=6)]
    want = [1, 1, 2, None, 1, None, 3, 3, None, 0, None, None, 0, 1, 5, None]
    for outputs in (True, False):                                    # with `ends` and `reasons`, and with both NULL
        tokens, reasons = _run(vocab, dtype, do_sample, rows, stop=stop, eos=EOS, pad=1, outputs=outputs)
        assert reasons == want
        assert tokens == [1 if r.get('finished') else int(np.argmax(r['x'])) for r in rows]
    rows = [dict(x=_needles(vocab, T, B), h=[T] * (COLS - 1)),                    # the last column, the phrase in front of it
            dict(x=_needles(vocab, T, B), h=[T, T], begin=1),
            dict(x=_needles(vocab, EOS, B), h=[3, 23], minimum=3),                # the EOS id is masked below the minimum: no end
            dict(x=_needles(vocab, T, EOS), h=[3, 23], minimum=3),
            dict(x=_needles(vocab, long63[-1], B), h=long63[:-1]),                # the phrase lacks its last id: no match
            dict(x=_needles(vocab, Y, B), h=[-1] + long63[1:])]                   # a mismatch at the far end of 64 ids
    tokens, reasons = _run(vocab, dtype, do_sample, rows, stop=stop, eos=EOS, pad=1)
    assert reasons == [6, None, None, None, None, None] and tokens[2] == B


@pytest.mark.parametrize('do_sample', [False, True])
def test_lists_of_1024_phrases_with_only_the_last_one_matching(do_sample):
    vocab = 4099
    A, B = vocab - 3, vocab - 6
    near = [[40 + j % 9, 50 + j % 11, 60, A] for j in range(1023)]   # the last two ids agree with the text: compared further back
    rows = [dict(x=_needles(vocab, A, B), h=[3, 39, 50, 60]), dict(x=_needles(vocab, A, B), h=[5])]
    tokens, reasons = _run(vocab, 'bf16', do_sample, rows, ban=[w[:3] + [B] for w in near] + [[39, 50, 60, A]], stop=near + [[5, A]])
    assert tokens == [B, A] and reasons == [None, 1024]
    tokens, reasons = _run(vocab, 'bf16', do_sample, rows, ban=[[5, A]] + near, stop=[[39, 50, 60, A]] + near[:1022] + [[3, 39, 50, 60, A]])
    assert tokens == [A, B] and reasons == [1, None]
    bp = _bp()
    with pytest.raises(ValueError):
        bp.pick_token(_place(np.zeros((1, 8)), torch.float32), bad_words_ids=near + [[1], [2]],
                      sequences=torch.zeros((1, 4), dtype=torch.int64, device=DEV))


# ---- capture and replay --------------------------------------------------------------------------------------------------------------

def test_capture_and_replay_with_the_history_growing_on_the_device():
    bp = _bp()
    batch, vocab, replays = 2, 4099, 12
    starts = [3, 5]
    # n-gram blocking with n = 1 bans what the row holds: static logits give every row its ids in the order of their values
    order = [[4000 - 7 * i for i in range(20)], [100 + 5 * i for i in range(20)]]
    x = np.zeros((batch, vocab), dtype=np.float32)
    for b in range(batch):
        x[b, order[b]] = 90.0 - 2.0 * np.arange(20)
    logits = _place(x, torch.bfloat16, pad=8, misalign=1)
    x = logits.float().cpu().numpy()
    prompt = [[7, 8, 9], [7, 8, 9, 10, 11]]
    # row 0 writes order[0][0], [1], [2] (the eager step, replays 1 and 2); at replay 3 the ban phrase is active and [3] is
    # skipped for [4]; replay 4 takes [3], replay 5 [5], which completes the stop phrase.  Row 1 never meets either.
    ban = [[order[0][2], order[0][3]], [order[0][0], order[1][1]]]
    stop = [[order[1][0], order[0][1]], [order[0][3], order[0][5]]]
    cols = max(starts) + replays + 3
    kw = dict(no_repeat_ngram_size=1, pad_token_id=2)

    def fresh():
        sequences = torch.full((batch, cols), -1, dtype=torch.int64, device=DEV)
        for b, s in enumerate(starts):
            sequences[b, :s] = _dev(prompt[b], torch.int64)
        counters = _dev([s - 1 for s in starts], torch.int32)
        return (sequences, counters, torch.zeros(batch, dtype=torch.int64, device=DEV),
                torch.zeros(batch, dtype=torch.int32, device=DEV), torch.full((batch,), CANARY, dtype=torch.int32, device=DEV),
                torch.full((batch,), CANARY, dtype=torch.int32, device=DEV))
    begins = _dev(starts, torch.int32)
    packed = dict(bad_words_ids=bp.pack_phrases(ban, DEV), stop_sequences=bp.pack_phrases(stop, DEV))

    def step(sequences, counters, tokens, finished, ends, reasons):  # the length increment, then the pick: what a decode loop captures
        counters.add_(1)
        bp.pick_token(logits, counters=counters, tokens=tokens, sequences=sequences, finished=finished, penalty_begin=begins,
                      ends=ends, reasons=reasons, **packed, **kw)

    buffers = fresh()
    step(*buffers)                                                   # the first step eagerly, as the loops run it
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(*buffers)
    for _ in range(replays):
        graph.replay()
    torch.cuda.synchronize()
    # the restatement's loop
    rows = np.full((batch, cols), -1, dtype=np.int64)
    finished, ends, reasons = [0] * batch, [CANARY] * batch, [CANARY] * batch
    for b, s in enumerate(starts):
        rows[b, :s] = prompt[b]
        for c in range(s, s + 1 + replays):
            tok, why = P.step(x[b], rows[b], c, bool(finished[b]), s, 0, ban, stop, pad=2, no_repeat_ngram_size=1)
            rows[b, c] = tok
            if why is not None:
                finished[b], ends[b], reasons[b] = 1, c + 1, why
    assert rows[0, starts[0]:starts[0] + 8].tolist() == [order[0][i] for i in (0, 1, 2, 4, 3, 5)] + [2, 2]
    assert rows[1, starts[1]:starts[1] + 1 + replays].tolist() == order[1][:1 + replays]
    assert (finished, ends, reasons) == ([1, 0], [starts[0] + 6, CANARY], [2, CANARY])
    assert buffers[0].cpu().numpy().tolist() == rows.tolist()
    assert buffers[3].tolist() == finished and buffers[4].tolist() == ends and buffers[5].tolist() == reasons
    assert buffers[1].tolist() == [s + replays for s in starts]


# ---- generation ----------------------------------------------------------------------------------------------------------------------

def test_sampling_with_both_options_graphed_equals_eager():
    PROMPT, NEW = 8, 24
    model = _model('small', seed=2)
    ids = torch.randint(0, MODEL_VOCAB, (3, PROMPT), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    n = PROMPT + NEW
    kw = dict(kv_cache=True, rng_state=_state(), top_k=8, return_dict_in_generate=True)
    free = model.sample(ids, n, cg=True, **kw).sequences.tolist()
    stops = [free[0][PROMPT + 6:PROMPT + 8], [free[2][PROMPT + 12]], [MODEL_VOCAB - 1] * 3]
    bad = [free[1][PROMPT + 3:PROMPT + 5]]
    eager = model.sample(ids, n, stop_sequences=stops, bad_words_ids=bad, stop_check_every=1, **kw)
    graph = model.sample(ids, n, cg=True, stop_sequences=stops, bad_words_ids=bad, **kw)
    assert torch.equal(eager.sequences, graph.sequences) and torch.equal(eager.lengths, graph.lengths)
    assert torch.equal(eager.stop_reasons, graph.stop_reasons) and graph.stop_reasons.dtype == torch.int64
    out, lengths, why = graph.sequences.tolist(), graph.lengths.tolist(), graph.stop_reasons.tolist()
    assert graph.sequences.shape[1] == max(lengths)
    for b in range(3):
        row = free[b]
        # the free run up to its first stop, unless the banned phrase comes first: there the two part
        end, reason = next(((c + 1, 1 + j) for c in range(PROMPT, n - 1) for j, w in enumerate(stops)
                            if c + 1 - len(w) >= PROMPT and row[c + 1 - len(w):c + 1] == w), (n - 1, -1))
        parted = next((t for t in range(PROMPT, n - 1) if row[t - 1:t + 1] == bad[0]), n)
        if parted >= end:
            assert (lengths[b], why[b]) == (end, reason) and out[b][:end] == row[:end], b
        else:
            assert out[b][:parted] == row[:parted] and out[b][parted] != row[parted] and lengths[b] > parted, b
        assert all(t == 0 for t in out[b][lengths[b]:])
        assert not any(out[b][t - 1:t + 1] == bad[0] for t in range(PROMPT, lengths[b]))
        if why[b] > 0:
            assert out[b][lengths[b] - len(stops[why[b] - 1]):lengths[b]] == stops[why[b] - 1]
    print('lengths', lengths, 'reasons', why)
