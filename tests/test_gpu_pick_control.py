"""GPU: bp_pick_token_ctl (csrc/pick_token_ctl.hip) against the numpy restatement of tests/pick_ctl_ref.py -- controls off equals
bp_pick_token bit for bit, every bit of the history bitmap, the kept set and the draw under the penalty, EOS / finished /
min_length, purity, graph capture -- and the stopping generation loops on the decode models."""
import numpy as np
import pytest
import torch

import pick_ctl_ref as C
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
    elements behind a 16-byte boundary (test_gpu_pick.py's, restated)."""
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


# ---- controls off: bp_pick_token, bit for bit -----------------------------------------------------------------------------------------

def _mixed_rows(batch, vocab, rng):
    x = (2.0 * rng.standard_normal((batch, vocab))).astype(np.float32)
    x[1] = np.round(x[1] * 2) / 2                  # heavy ties
    x[2, vocab // 2:] = -INF
    x[3] *= 8.0
    x[4, vocab // 3] = NAN                         # degenerate: stats of the greedy form
    x[5, :] = -INF
    x[6, vocab - 1] = INF
    x[7] = -np.abs(x[7])
    return x


@pytest.mark.parametrize('layout', ['dense', 'strided-misaligned'])
@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('vocab', [1, 7, 255, 256, 257, 4096, 50264])
def test_controls_off_equals_the_plain_pick_bit_for_bit(vocab, dtype, layout):
    bp = _bp()
    batch = 10
    x = _mixed_rows(batch, vocab, np.random.default_rng(vocab))
    pad, mis = (0, 0) if layout == 'dense' else (13, 3 if dtype != 'fp32' else 1)
    logits = _place(x, DTYPES[dtype], pad, mis)
    counters = ((torch.arange(batch, device=DEV) * 5) % 7).int()
    for sampling in (dict(do_sample=False), dict(do_sample=True, temperature=0.7, top_k=40, top_p=0.95)):
        seq_a = torch.full((batch, 6), -1, dtype=torch.int64, device=DEV)
        seq_b = seq_a.clone()
        plain, plain_stats = bp.pick_token(logits, rng_state=_state(), counters=counters, sequences=seq_a, return_stats=True,
                                           **sampling)
        # pad_token_id alone selects bp_pick_token_ctl and switches nothing on: theta 1, no EOS id, no flags
        ctl, ctl_stats = bp.pick_token(logits, rng_state=_state(), counters=counters, sequences=seq_b, return_stats=True,
                                       pad_token_id=0, **sampling)
        assert torch.equal(plain, ctl), (sampling, plain.tolist(), ctl.tolist())
        assert torch.equal(_bits(plain_stats), _bits(ctl_stats)), sampling
        assert torch.equal(seq_a, seq_b)


# ---- every bit of the bitmap ----------------------------------------------------------------------------------------------------------

def _positions(vocab):
    if vocab <= 257:
        return list(range(vocab))
    fixed = [0, 1, 31, 32, 63, 64, 65, 4095 if vocab > 4096 else vocab - 2, vocab - 1]
    seeded = np.random.default_rng(vocab).integers(0, vocab, size=32).tolist()
    return fixed + [int(t) for t in seeded]


@pytest.mark.parametrize('misalign', [0, 1])
@pytest.mark.parametrize('value', [2.0, -2.0])
@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
@pytest.mark.parametrize('vocab', [257, 4096, 50264])
def test_every_bit_of_the_history_bitmap(vocab, dtype, value, misalign):
    bp = _bp()
    ts = _positions(vocab)
    rows = len(ts)
    logits = _place(np.full((rows, vocab), value, dtype=np.float32), DTYPES[dtype], pad=5, misalign=misalign)
    assert misalign == 0 or logits.data_ptr() % 16 != 0
    # row r has the one-token history {t_r}: with theta = 2 exactly t_r leaves the top vocab - 1
    sequences = _dev(np.array(ts)[:, None], torch.int64).repeat(1, 2).contiguous()
    counters = torch.ones(rows, dtype=torch.int32, device=DEV)
    tokens, stats = bp.pick_token(logits, True, 1.0, vocab - 1, 1.0, _state(), counters, sequences=sequences, return_stats=True,
                                  repetition_penalty=2.0)
    stats, tokens = stats.cpu().numpy(), tokens.cpu().tolist()
    assert stats[:, 2].tolist() == [float(vocab - 1)] * rows
    assert stats[:, 0].tolist() == [value] * rows
    assert all(tok != t for tok, t in zip(tokens, ts))
    assert sequences[:, 0].cpu().tolist() == ts and sequences[:, 1].cpu().tolist() == tokens
    # the greedy pick with the history {0 .. m - 1} is m
    ms = sorted(set(ts))
    history = torch.arange(max(ms) + 1, dtype=torch.int64, device=DEV).repeat(len(ms), 1).contiguous()
    got = bp.pick_token(logits[:len(ms)], counters=_dev(ms, torch.int32), sequences=history, repetition_penalty=2.0)
    assert got.cpu().tolist() == ms


# ---- the kept set and the draw under the penalty --------------------------------------------------------------------------------------

def _sampling_rows(batch, vocab, dtype, seed=0):
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((batch, vocab))).astype(np.float32)
    x[1] = np.round(x[1] * 2) / 2                  # heavy ties, at every threshold
    x[2, vocab // 2:] = -INF                       # half the row carries no mass
    x[3] *= 8.0                                    # one dominant token
    x[4] *= 0.01                                   # nearly uniform
    return _place(x, dtype, pad=8, misalign=0)


HISTORY_LENGTHS = [0, 1, 63, 64, 65, 1024, 2000, 7]        # 2000 > the 1200 columns: clamped, and the write is skipped
COLS = 1200


def _history_rows(batch, vocab, seed):
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, vocab, size=(batch, COLS)).astype(np.int64)
    seq[:, 40:60] = seq[:, 0:20]                   # duplicates
    seq[:, 3] = -1                                 # ids outside the vocabulary are ignored
    seq[:, 4] = vocab
    seq[:, 5] = 2 ** 40
    seq[:, 0] = np.arange(batch) % vocab
    counters = np.array([HISTORY_LENGTHS[b % len(HISTORY_LENGTHS)] for b in range(batch)], dtype=np.int32)
    return seq, counters


def _top_p_margin(z, top_k, top_p):
    """Smallest distance, as a probability, between top_p and the mass above a distinct kept value: where it exceeds eps the
    float64 walk of pick_ref.kept_set and the fixed-point select cannot disagree about the threshold."""
    keep = R.kept_set(z, top_k, 1.0)
    w = R.masses(z) * keep
    _, inverse = np.unique(z[keep], return_inverse=True)
    mass = np.bincount(inverse, weights=w[keep])[::-1]             # per distinct kept value, largest first
    above = (np.cumsum(mass) - mass) / w.sum()
    return float(np.abs(above - top_p).min())


CTL_CASES = [   # vocab, dtype, theta, temperature, top_k, top_p
    (1000, 'fp32', 1.2, 0.8, 50, 1.0), (1000, 'fp32', 0.8, 1.0, 0, 0.9), (4096, 'fp16', 1.2, 1.3, 10, 1.0),
    (4096, 'bf16', 0.8, 0.7, 40, 0.95), (50264, 'bf16', 1.2, 0.7, 40, 0.95), (50264, 'bf16', 1.2, 1.0, 0, 1.0),
    (50264, 'fp16', 0.8, 1.0, 1000, 1.0), (257, 'bf16', 1.2, 1.0, 256, 0.5), (7, 'fp32', 1.2, 1.0, 3, 1.0),
]


@pytest.mark.parametrize('vocab,dtype,theta,temperature,top_k,top_p', CTL_CASES)
def test_kept_set_and_draw_under_the_penalty(vocab, dtype, theta, temperature, top_k, top_p):
    bp = _bp()
    batch = 16
    logits = _sampling_rows(batch, vocab, DTYPES[dtype], seed=vocab + top_k)
    seq, counters = _history_rows(batch, vocab, seed=vocab + 1)
    x = _host(logits)
    eps = R.epsilon(vocab)
    for with_counters in (True, False):
        sequences = _dev(seq, torch.int64)
        c_dev = _dev(counters, torch.int32) if with_counters else None
        c_host = counters if with_counters else np.zeros(batch, dtype=np.int32)
        args = dict(rng_state=_state(), counters=c_dev, sequences=sequences, repetition_penalty=theta)
        tokens, stats = bp.pick_token(logits, True, temperature, top_k, top_p, return_stats=True, **args)
        tokens, stats = tokens.cpu().tolist(), stats.cpu().numpy()
        for b in range(batch):
            what = (vocab, dtype, theta, temperature, top_k, top_p, with_counters, b)
            hist = C.history(seq[b], int(c_host[b]), vocab)
            assert (len(hist) > 0) == (c_host[b] > 0)
            z = C.scaled_values(x[b], temperature, hist, theta, int(c_host[b]), None, 0)
            assert not R.degenerate(z)
            u = R.uniform(SEED, OFFSET, b, int(c_host[b]))
            assert stats[b, 3] == np.float32(u), what
            lo, count = stats[b, 0], int(stats[b, 2])
            keep = R.kept_set(z, top_k, top_p)
            if top_p >= 1.0 or _top_p_margin(z, top_k, top_p) > eps:
                assert count == int(keep.sum()) and lo == z[keep].min(), (what, count, int(keep.sum()), lo, z[keep].min())
            else:                                    # top_p within eps of a boundary: either neighbouring threshold
                keep = R.kept_set(z, top_k, 1.0) & (z >= lo)
                assert count == int(keep.sum()) and lo == z[keep].min(), what
            R.assert_draw(tokens[b], z, keep, u, eps, what=what)
        # the writes: column counters[b] where it exists, nothing else
        want = torch.as_tensor(seq).clone()
        for b in range(batch):
            if 0 <= c_host[b] < COLS:
                want[b, c_host[b]] = tokens[b]
        assert torch.equal(sequences.cpu(), want)
        # greedy with the penalty: numpy's argmax of the float32 pen(x)
        greedy = bp.pick_token(logits, counters=c_dev, sequences=_dev(seq, torch.int64), repetition_penalty=theta)
        for b in range(batch):
            hist = C.history(seq[b], int(c_host[b]), vocab)
            assert greedy[b].item() == R.greedy(C.greedy_values(x[b], hist, theta, int(c_host[b]), None, 0)), b
        # two calls on the same inputs agree bit for bit
        again, stats2 = bp.pick_token(logits, True, temperature, top_k, top_p, return_stats=True,
                                      **{**args, 'sequences': _dev(seq, torch.int64)})
        assert again.cpu().tolist() == tokens and torch.equal(_bits(stats2).cpu(), torch.as_tensor(stats).view(torch.int32))


def test_a_penalty_at_the_largest_vocabulary_it_takes():
    bp = _bp()
    vocab = 2 ** 19
    x = np.zeros((2, vocab), dtype=np.float32)
    x[:, [5, vocab - 1, 70000]] = [[3.0, 2.5, 2.0]]
    logits = _place(x, torch.bfloat16)
    sequences = _dev([[5, vocab - 1, 0], [5, 5, 0]], torch.int64)
    got = bp.pick_token(logits, counters=_dev([2, 2], torch.int32), sequences=sequences, repetition_penalty=2.0)
    assert got.cpu().tolist() == [70000, vocab - 1]                    # 1.5 and 1.25 against 2.0; 1.5 against 2.5
    with pytest.raises(RuntimeError):
        bp.pick_token(_place(np.zeros((1, vocab + 1), dtype=np.float32), torch.bfloat16),
                      counters=_dev([1], torch.int32), sequences=_dev([[0]], torch.int64), repetition_penalty=2.0)


# ---- 16-bit rows whose penalised order differs from the raw order ---------------------------------------------------------------------

@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_top_k_selects_on_the_penalised_values_not_on_the_raw_elements(dtype):
    bp = _bp()
    vocab = 4096
    x = np.full((4, vocab), -5.0, dtype=np.float32)
    x[:, 100:120] = 8.0 - 0.25 * np.arange(20)           # exact in both 16-bit formats: 8, 7.75, ... at columns 100 ..
    x[2:, 200:220] = -1.0 - 0.25 * np.arange(20)         # rows 2, 3: the same with negative values on top
    x[2:, 100:120] = -9.0
    logits = _place(x, DTYPES[dtype])
    # the raw top-3 of every row are in its history: theta = 4 quarters 8, 7.75, 7.5 (quadruples -1, -1.25, -1.5)
    seq = np.array([[100, 101, 102], [100, 101, 102], [200, 201, 202], [200, 201, 202]], dtype=np.int64)
    counters = _dev([3, 3, 3, 3], torch.int32)
    for top_k, top_p in ((2, 1.0), (3, 1.0), (2, 0.5)):
        tokens, stats = bp.pick_token(logits, True, 1.0, top_k, top_p, _state(), counters, sequences=_dev(seq, torch.int64),
                                      return_stats=True, repetition_penalty=4.0)
        for b in range(4):
            hist = C.history(seq[b], 3, vocab)
            z = C.scaled_values(_host(logits)[b], 1.0, hist, 4.0, 3, None, 0)
            keep = R.kept_set(z, top_k, top_p)
            first = 103 if b < 2 else 203
            assert set(np.nonzero(keep)[0]) <= set(range(first, first + top_k))
            assert int(stats[b, 2]) == int(keep.sum()) and stats[b, 0].item() == z[keep].min(), (b, top_k, top_p)
            assert keep[tokens[b].item()], (b, top_k, top_p, tokens[b].item())


# ---- EOS, finished rows, min_length ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('vocab,dtype', [(50264, 'bf16'), (257, 'fp32'), (7, 'fp16')])
def test_eos_mask_finished_rows_and_flags(vocab, dtype):
    bp = _bp()
    batch, cols, eos, pad, min_length = 8, 12, vocab - 2, 1, 6
    rng = np.random.default_rng(vocab)
    x = (2.0 * rng.standard_normal((batch, vocab))).astype(np.float32)
    x[:, eos] = 50.0                                     # the EOS id is the argmax of every row
    x[6, :] = -INF
    x[6, eos] = 1.0                                      # row 6: the masked EOS is its only finite logit
    logits = _place(x, DTYPES[dtype], pad=3, misalign=1)
    xh = _host(logits)
    counters = np.array([0, 5, 6, 7, 2, 11, 3, 9], dtype=np.int32)
    entry = np.array([0, 0, 0, 0, 1, 5, 0, 0], dtype=np.int32)        # rows 4 and 5 are finished on entry
    for sampling in (dict(do_sample=False), dict(do_sample=True, top_k=1), dict(do_sample=True, temperature=0.9, top_p=0.3)):
        tok_buf = torch.full((batch, 2), -7, dtype=torch.int64, device=DEV)
        seq_buf = torch.full((batch, cols + 2), -7, dtype=torch.int64, device=DEV)
        fin_buf = torch.full((batch + 2,), -7, dtype=torch.int32, device=DEV)
        fin_buf[1:1 + batch] = _dev(entry, torch.int32)
        tokens, stats = bp.pick_token(logits, rng_state=_state(), counters=_dev(counters, torch.int32), tokens=tok_buf[:, 0],
                                      sequences=seq_buf[:, :cols], return_stats=True, eos_token_id=eos, pad_token_id=pad,
                                      min_length=min_length, finished=fin_buf[1:1 + batch], **sampling)
        torch.cuda.synchronize()
        tokens, stats = tokens.cpu().tolist(), stats.cpu().numpy()
        want_fin = []
        for b in range(batch):
            token, z, keep, u, fin = C.pick(xh[b], seed=SEED, offset=OFFSET, row=b, counter=int(counters[b]), eos_token_id=eos,
                                            pad_token_id=pad, min_length=min_length, finished=bool(entry[b]), **sampling)
            want_fin.append(int(entry[b]) if entry[b] else int(fin))
            if entry[b]:
                assert tokens[b] == pad and stats[b, :3].tolist() == [0.0, 0.0, 0.0], (sampling, b)
                assert stats[b, 3] == (np.float32(u) if sampling['do_sample'] else 0.0)
            elif keep is None:
                assert tokens[b] == token, (sampling, b, tokens[b], token)
            else:
                R.assert_draw(tokens[b], z, keep, u, R.epsilon(vocab), what=(sampling, b))
            if not entry[b] and b != 6:
                assert (tokens[b] == eos) == (counters[b] >= min_length), (sampling, b)
        assert tokens[6] == 0                                   # nothing finite is left: the greedy answer of a row of -inf
        fin = fin_buf.cpu().tolist()
        assert fin[0] == -7 and fin[-1] == -7 and fin[1:-1] == want_fin, (sampling, fin)
        assert want_fin == [0, 0, 1, 1, 1, 5, 0, 1]
        tok = tok_buf.cpu()
        assert (tok[:, 1] == -7).all() and tok[:, 0].tolist() == tokens
        want = torch.full((batch, cols + 2), -7, dtype=torch.int64)
        for b in range(batch):
            want[b, counters[b]] = tokens[b]
        assert torch.equal(seq_buf.cpu(), want)


# ---- capture and replay ---------------------------------------------------------------------------------------------------------------

def test_capture_and_replay_with_history_and_flags_on_the_device():
    bp = _bp()
    batch, vocab, steps, start = 6, 4096, 8, 3
    logits = _sampling_rows(batch, vocab, torch.bfloat16, seed=9)
    state = _state()
    prompt = torch.randint(0, vocab, (batch, start), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))

    def fresh():
        sequences = torch.full((batch, start + steps + 2), -1, dtype=torch.int64, device=DEV)
        sequences[:, :start] = prompt
        return (sequences, torch.zeros(batch, dtype=torch.int32, device=DEV), torch.full((batch,), start, dtype=torch.int32, device=DEV),
                torch.zeros(batch, dtype=torch.int64, device=DEV))

    def pick(sequences, finished, counters, tokens, eos):
        bp.pick_token(logits, True, 0.8, 50, 0.9, state, counters, tokens=tokens, sequences=sequences, repetition_penalty=1.5,
                      eos_token_id=eos, pad_token_id=0, finished=finished)

    # a dry run without flags being hit tells which id row 0 draws third: that id is the EOS of the real runs
    sequences, finished, counters, tokens = fresh()
    for _ in range(steps):
        pick(sequences, finished, counters, tokens, vocab - 1)
        counters += 1
    eos = int(sequences[0, start + 2])
    sequences, finished, counters, tokens = fresh()
    eager = []
    for _ in range(steps):
        pick(sequences, finished, counters, tokens, eos)
        eager.append(tokens.clone())
        counters += 1
    want_seq, want_fin = sequences.clone(), finished.clone()
    assert want_fin[0].item() == 1 and eager[3][0].item() == 0           # row 0 ended at its third pick, then pads
    sequences, finished, counters, tokens = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pick(sequences, finished, counters, tokens, eos)
    for i in range(steps):
        graph.replay()
        assert torch.equal(tokens, eager[i]), i
        counters += 1
    # the history grew by the pick's own writes and the flags persisted: the same sequences and flags as the eager calls
    assert torch.equal(sequences, want_seq) and torch.equal(finished, want_fin)
    assert (sequences[:, start + steps:] == -1).all()


# ---- the generation loops -------------------------------------------------------------------------------------------------------------

PROMPT, NEW = 8, 24


def _ids(batch, seed=5):
    return torch.randint(0, VOCAB, (batch, PROMPT), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _expected(free, eos, pad):
    free = free.clone()
    width = free.shape[1]
    lengths = []
    for b in range(free.shape[0]):
        hits = [t for t in range(PROMPT, width) if int(free[b, t]) == eos]
        end = hits[0] + 1 if hits else width
        free[b, end:] = pad
        lengths.append(end)
    return free[:, :max(lengths)], lengths


@pytest.mark.parametrize('decode', ['generate', 'sample'])
@pytest.mark.parametrize('name', ['small', 'mini_k4'])
def test_generation_stops_at_eos_eager_and_graphed(name, decode):
    model = _model(name, seed=2)
    ids = _ids(3)
    n = PROMPT + NEW
    run = getattr(model, decode)
    kw = dict(kv_cache=True, rng_state=_state()) if decode == 'sample' else dict(kv_cache=True, device_pick=True)
    for theta in (1.0, 1.2):
        free = run(ids, n, cg=True, repetition_penalty=theta, **kw)
        assert free.shape == (3, n - 1)
        eos = int(free[0, PROMPT + 3])
        want, lengths = _expected(free, eos, eos)
        eager = run(ids, n, repetition_penalty=theta, eos_token_id=eos, stop_check_every=1, return_dict_in_generate=True, **kw)
        graph = run(ids, n, cg=True, repetition_penalty=theta, eos_token_id=eos, stop_check_every=2, return_dict_in_generate=True,
                    **kw)
        late = run(ids, n, cg=True, repetition_penalty=theta, eos_token_id=eos, return_dict_in_generate=True, **kw)
        for out in (eager, graph, late):
            assert torch.equal(out.sequences, want) and out.lengths.tolist() == lengths, theta
            assert out.lengths.dtype == torch.int64 and out.sequences.dtype == ids.dtype
        if theta != 1.0:
            assert not torch.equal(free, run(ids, n, cg=True, **kw)), 'the penalty changed nothing: a weak test'
    # min_length keeps the EOS out of the columns in front of it
    held = run(ids, n, cg=True, eos_token_id=eos, min_length=PROMPT + 8, **kw)
    assert not (held[:, PROMPT:PROMPT + 8] == eos).any()


def test_intervened_wrapper_takes_the_controls():
    from src.models.intervened_models import WeightedBackpackLMHeadModel
    model = _model('small', seed=4)
    cfg = model.config
    cw = (torch.rand(model.lm_head.weight.shape[0], cfg.num_content_vectors, generator=torch.Generator().manual_seed(11)) * 3)
    wrapper = WeightedBackpackLMHeadModel(model, cw.to(DEV), None, 0.1, anneal=False, upweight_nearby=True).eval()
    ids = _ids(2)
    n = PROMPT + NEW
    free = wrapper.generate(ids, n, kv_cache=True, cg=True, repetition_penalty=1.2)
    eos = int(free[0, PROMPT + 3])
    want, lengths = _expected(free, eos, eos)
    for cg in (False, True):
        out = wrapper.generate(ids, n, kv_cache=True, cg=cg, repetition_penalty=1.2, eos_token_id=eos, return_dict_in_generate=True)
        assert torch.equal(out.sequences, want) and out.lengths.tolist() == lengths
    a = wrapper.sample(ids, n, kv_cache=True, cg=True, rng_state=_state(), top_k=10, repetition_penalty=1.2, eos_token_id=eos)
    b = wrapper.sample(ids, n, kv_cache=True, rng_state=_state(), top_k=10, repetition_penalty=1.2, eos_token_id=eos)
    assert torch.equal(a, b) and torch.equal(a[:, :PROMPT], ids)
