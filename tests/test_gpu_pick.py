"""GPU: bp_pick_token (csrc/pick_token.hip) against the float64 restatement of tests/pick_ref.py -- the argmax exactly, the kept
set exactly through `stats`, the draw within the derived bound eps = (vocab + 64) 2^-24 (pick_ref.epsilon), the distribution by a
chi-square test, purity, guard values, graph capture -- and the generation options on the decode models."""
import numpy as np
import pytest
import torch

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
    elements behind a 16-byte boundary."""
    rows = torch.as_tensor(rows, dtype=torch.float32)
    b, v = rows.shape
    flat = torch.zeros(b * (v + pad) + 16, dtype=dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = flat[misalign:misalign + b * (v + pad)].view(b, v + pad)[:, :v]
    view.copy_(rows.to(dtype))
    return view


def _host(t):
    return t.float().cpu().numpy()


# ---- greedy: exact --------------------------------------------------------------------------------------------------------------------

def _greedy_rows(vocab, rng):
    x = (2.0 * rng.standard_normal((10, vocab))).astype(np.float32)
    top = np.abs(x).max() + 1.0
    x[1, 0] = x[1, -1] = top                       # tie between the first and the last column
    x[2, -1] = top                                 # the last column alone
    x[3, -1] = INF
    x[4, :] = -INF
    x[4, vocab // 2] = -3.0
    x[5, vocab // 3] = NAN                          # the first NaN wins, over the +inf in front of it too
    x[5, -1] = NAN
    x[5, 0] = INF if vocab > 3 else x[5, 0]
    x[6, :] = -INF                                 # nothing finite: column 0
    x[7, :] = 0.25                                 # all equal
    x[8, vocab // 2:] = top                        # a long run of ties
    x[9, :] = 0.0
    x[9, ::2] = -0.0                               # signed zeros are equal
    return x


@pytest.mark.parametrize('layout', ['dense', 'strided-misaligned'])
@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('vocab', [1, 7, 255, 256, 257, 4096, 50257, 50264, 131072])
def test_greedy_is_numpy_argmax(vocab, dtype, layout):
    bp = _bp()
    x = _greedy_rows(vocab, np.random.default_rng(vocab))
    pad, mis = (0, 0) if layout == 'dense' else (13, 3 if dtype != 'fp32' else 1)
    logits = _place(x, DTYPES[dtype], pad, mis)
    assert layout == 'dense' or (logits.data_ptr() % 16 != 0 and logits.stride(0) > vocab)
    before = logits.clone()
    got, stats = bp.pick_token(logits, return_stats=True)
    want = np.argmax(_host(logits), axis=-1)
    assert got.cpu().tolist() == want.tolist()
    assert torch.equal(before.view(torch.int16 if dtype != 'fp32' else torch.int32),
                       logits.view(torch.int16 if dtype != 'fp32' else torch.int32))
    assert stats[:, 2].cpu().tolist() == [1.0] * 10
    # sampling the degenerate rows gives the same answer
    drawn = bp.pick_token(logits, do_sample=True, temperature=0.7, top_k=5, top_p=0.9, rng_state=_state())
    for b in (3, 5, 6):
        assert drawn[b].item() == want[b], b


# ---- the kept set, exactly, and the draw within eps -------------------------------------------------------------------------------------

def _sampling_rows(batch, vocab, dtype, seed=0):
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((batch, vocab))).astype(np.float32)
    x[1] = np.round(x[1] * 2) / 2                  # heavy ties, at every threshold
    x[2, vocab // 2:] = -INF                       # half the row carries no mass
    x[3] *= 8.0                                    # one dominant token
    x[4] *= 0.01                                   # nearly uniform
    return _place(x, dtype, pad=8, misalign=0)


def _check_picks(logits, counters, tokens, stats, temperature, top_k, top_p, what):
    """Every row: the reported threshold against the float64 restatement, then the draw."""
    vocab = logits.shape[1]
    eps = R.epsilon(vocab)
    x = _host(logits)
    tokens, stats, counters = tokens.cpu().tolist(), stats.cpu().numpy(), counters.cpu().tolist()
    for b in range(x.shape[0]):
        z = R.scaled(x[b], temperature)
        assert not R.degenerate(z)
        u = R.uniform(SEED, OFFSET, b, counters[b])
        assert stats[b, 3] == np.float32(u), (what, b)
        lo, count = stats[b, 0], int(stats[b, 2])
        keep_k = np.ones(vocab, dtype=bool)
        if 0 < top_k < vocab:
            tau = np.sort(z)[vocab - top_k]
            keep_k = z >= tau
            if top_p >= 1.0:
                assert lo == tau, (what, b, lo, tau)          # the k-th largest scaled logit, exactly
        keep = keep_k & (z >= lo)
        assert count == int(keep.sum()), (what, b, count, int(keep.sum()))
        assert lo == z[keep].min(), (what, b)
        w = R.masses(z) * keep_k
        total = w.sum()
        if top_p < 1.0:
            above = w[z > lo].sum() / total
            at_or_above = w[z >= lo].sum() / total
            assert above < top_p + eps and at_or_above >= top_p - eps, (what, b, above, at_or_above, top_p)
        lse = np.log((R.masses(z) * keep).sum()) + np.float64(z.max())
        assert abs(stats[b, 1] - lse) <= eps + 4 * 2.0 ** -23 * max(1.0, abs(lse)), (what, b, stats[b, 1], lse)
        R.assert_draw(tokens[b], z, keep, u, eps, what=(what, b))


CASES = [   # vocab, dtype, temperature, top_k, top_p
    (1000, 'fp32', 1.0, 0, 1.0), (1000, 'fp32', 0.8, 50, 0.9), (1000, 'bf16', 0.7, 10, 1.0), (1000, 'fp16', 1.3, 0, 0.9),
    (257, 'bf16', 1.0, 1, 1.0), (257, 'fp32', 0.5, 256, 0.5), (257, 'fp16', 2.0, 257, 0.99), (7, 'bf16', 1.0, 3, 0.6),
    (4096, 'bf16', 0.7, 10, 1.0), (4096, 'bf16', 1.0, 0, 0.9), (50257, 'bf16', 0.7, 40, 0.95), (50264, 'fp16', 1.0, 0, 0.9),
    (50257, 'fp32', 0.9, 1000, 0.8), (131072, 'bf16', 1.0, 50, 0.95), (131072, 'fp32', 1.0, 0, 1.0), (50264, 'bf16', 1.0, 0, 1.0),
]


@pytest.mark.parametrize('vocab,dtype,temperature,top_k,top_p', CASES)
def test_kept_set_and_draw(vocab, dtype, temperature, top_k, top_p):
    from src.utils.generation import _eager_pick
    bp = _bp()
    batch = 24
    logits = _sampling_rows(batch, vocab, DTYPES[dtype], seed=vocab + top_k)
    counters = ((torch.arange(batch, device=DEV) * 37) % 101).int()
    tokens, stats = bp.pick_token(logits, True, temperature, top_k, top_p, _state(), counters, return_stats=True)
    what = (vocab, dtype, temperature, top_k, top_p)
    _check_picks(logits, counters, tokens, stats, temperature, top_k, top_p, what)
    eager = _eager_pick(logits.cpu(), True, temperature, top_k, top_p, _state().cpu(), counters.cpu())
    same = (eager == tokens.cpu()).float().mean().item()
    print(f'{what}: {100 * same:.1f} % of the tokens equal _eager_pick\'s')
    # without stats the same tokens
    assert torch.equal(bp.pick_token(logits, True, temperature, top_k, top_p, _state(), counters), tokens)


# ---- the distribution --------------------------------------------------------------------------------------------------------------------

CHI_CASES = [(1000, 'fp32', 0.8, 50, 0.9), (1000, 'fp32', 1.0, 0, 1.0), (50257, 'bf16', 0.7, 40, 0.95)]


@pytest.mark.parametrize('vocab,dtype,temperature,top_k,top_p', CHI_CASES)
def test_distribution_chi_square(vocab, dtype, temperature, top_k, top_p):
    from scipy.stats import chi2
    bp = _bp()
    rows, ncounters = 4096, 64
    x = (2.0 * np.random.default_rng(0).standard_normal(vocab)).astype(np.float32)
    logits = _place(x[None], DTYPES[dtype]).expand(rows, vocab).contiguous()     # one row, replicated
    z = R.scaled(_host(logits[:1])[0], temperature)
    keep = R.kept_set(z, top_k, top_p)
    probs = R.masses(z) * keep
    probs /= probs.sum()
    counts = torch.zeros(vocab, dtype=torch.int64, device=DEV)
    state = _state()
    for c in range(ncounters):
        counters = torch.full((rows,), c, dtype=torch.int32, device=DEV)
        counts += torch.bincount(bp.pick_token(logits, True, temperature, top_k, top_p, state, counters), minlength=vocab)
    counts = counts.cpu().numpy()
    assert counts.sum() == rows * ncounters and counts[~keep].sum() == 0
    stat, df = R.chi_square(counts, probs, rows * ncounters)
    bound = chi2.ppf(1 - 1e-9, df)
    print(f'chi-square {stat:.1f} at df {df} (bound {bound:.1f}) for {(vocab, dtype, temperature, top_k, top_p)}')
    assert stat < bound


# ---- purity and safety -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_repeated_calls_are_bit_identical_and_write_nothing_else(dtype):
    bp = _bp()
    batch, vocab, cols = 12, 50257, 9
    logits = _sampling_rows(batch, vocab, DTYPES[dtype], seed=3)
    bits = torch.int16 if dtype != 'fp32' else torch.int32
    before = logits.clone()
    # columns: in range, the edges, and outside on both sides (those writes are skipped)
    counters = torch.tensor([0, 8, 4, -1, 9, 10, 2 ** 31 - 1, -2 ** 31, 3, 3, 7, 1], dtype=torch.int32, device=DEV)
    runs = []
    for _ in range(3):
        tok_buf = torch.full((batch, 2), -7, dtype=torch.int64, device=DEV)          # tokens at stride 2, guards between
        seq_buf = torch.full((batch, cols + 3), -7, dtype=torch.int64, device=DEV)   # guards behind every row
        tokens, stats = bp.pick_token(logits, True, 0.7, 40, 0.95, _state(), counters, tokens=tok_buf[:, 0],
                                      sequences=seq_buf[:, :cols], return_stats=True)
        runs.append((tok_buf.cpu(), seq_buf.cpu(), stats.cpu()))
    for tok_buf, seq_buf, stats in runs[1:]:
        assert torch.equal(tok_buf, runs[0][0]) and torch.equal(seq_buf, runs[0][1])
        assert torch.equal(stats.view(torch.int32), runs[0][2].view(torch.int32))
    assert torch.equal(before.view(bits), logits.view(bits)), 'the logits are read-only'
    tok_buf, seq_buf, _ = runs[0]
    assert (tok_buf[:, 1] == -7).all() and ((tok_buf[:, 0] >= 0) & (tok_buf[:, 0] < vocab)).all()
    want = torch.full((batch, cols + 3), -7, dtype=torch.int64)
    for b, c in enumerate(counters.cpu().tolist()):
        if 0 <= c < cols:
            want[b, c] = tok_buf[b, 0]
    assert torch.equal(seq_buf, want), 'only column counters[b] of row b may change, and only inside [0, seq_cols)'
    # a NULL counters means 0
    zero = bp.pick_token(logits, True, 0.7, 40, 0.95, _state(), torch.zeros(batch, dtype=torch.int32, device=DEV))
    assert torch.equal(bp.pick_token(logits, True, 0.7, 40, 0.95, _state()), zero)


def test_capture_and_replay_with_counters_on_the_device():
    bp = _bp()
    batch, vocab = 8, 50264
    logits = _sampling_rows(batch, vocab, torch.bfloat16, seed=9)
    state = _state()
    counters = torch.full((batch,), 5, dtype=torch.int32, device=DEV)
    eager = []
    for i in range(3):
        eager.append(bp.pick_token(logits, True, 0.8, 50, 0.9, state, counters + i).clone())
    tokens = torch.zeros(batch, dtype=torch.int64, device=DEV)
    sequences = torch.full((batch, 16), -1, dtype=torch.int64, device=DEV)
    bp.pick_token(logits, True, 0.8, 50, 0.9, state, counters, tokens=tokens)       # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bp.pick_token(logits, True, 0.8, 50, 0.9, state, counters, tokens=tokens, sequences=sequences)
    for i in range(3):
        graph.replay()
        assert torch.equal(tokens, eager[i]), i
        assert torch.equal(sequences[:, 5 + i], eager[i])
        counters += 1
    assert (sequences[:, :5] == -1).all() and (sequences[:, 8:] == -1).all()


# ---- the generation loops ---------------------------------------------------------------------------------------------------------------

PROMPT, MAX_LENGTH = 12, 40


def _ids(batch, seed=5):
    return torch.randint(0, VOCAB, (batch, PROMPT), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _teacher_forced_logits(model, seq):
    """Logits of every generated position of `seq`, by the calls of the cached loop itself: prefill on the prompt, then one
    cached step per token with the lengths on the device.  Same kernels, same shapes: the logits the picks saw."""
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


@pytest.mark.parametrize('name', ['small', 'mini_k4'])
def test_generate_with_the_device_pick(name):
    model = _model(name, seed=2)
    ids = _ids(3)
    want = model.generate(ids, MAX_LENGTH, kv_cache=True, cg=True)
    got = model.generate(ids, MAX_LENGTH, kv_cache=True, cg=True, device_pick=True)
    assert got.shape == (3, MAX_LENGTH - 1) and got.dtype == ids.dtype
    assert torch.equal(got, want)
    assert torch.equal(model.generate(ids, MAX_LENGTH, kv_cache=True, device_pick=True), want)


@pytest.mark.parametrize('options', [dict(top_k=10, temperature=0.7), dict(top_p=0.9)], ids=['top_k', 'top_p'])
@pytest.mark.parametrize('name', ['small', 'mini_k4'])
def test_sample_eager_and_graph_draw_the_same_tokens(name, options):
    model = _model(name, seed=2)
    ids = _ids(3)
    eager = model.sample(ids, MAX_LENGTH, kv_cache=True, rng_state=_state(), **options)
    graph = model.sample(ids, MAX_LENGTH, kv_cache=True, cg=True, rng_state=_state(), **options)
    assert eager.shape == (3, MAX_LENGTH - 1) and torch.equal(eager[:, :PROMPT], ids)
    assert torch.equal(eager, graph)
    assert ((eager >= 0) & (eager < model.config.vocab_size)).all()
    other = model.sample(ids, MAX_LENGTH, kv_cache=True, cg=True, rng_state=_state(offset=OFFSET + 1), **options)
    assert not torch.equal(other, eager)
    if name != 'small':
        return
    temperature, top_k, top_p = options.get('temperature', 1.0), options.get('top_k', 0), options.get('top_p', 1.0)
    logits = _teacher_forced_logits(model, eager)
    eps = R.epsilon(logits[PROMPT].shape[1])
    for t in range(PROMPT, MAX_LENGTH - 1):
        x = _host(logits[t])
        for b in range(3):
            z = R.scaled(x[b], temperature)
            R.assert_draw(int(eager[b, t]), z, R.kept_set(z, top_k, top_p), R.uniform(SEED, OFFSET, b, t), eps, what=(t, b))


def test_intervened_wrapper_takes_the_pick_options():
    from src.models.intervened_models import WeightedBackpackLMHeadModel
    model = _model('small', seed=4)
    cfg = model.config
    cw = (torch.rand(model.lm_head.weight.shape[0], cfg.num_content_vectors, generator=torch.Generator().manual_seed(11)) * 3)
    wrapper = WeightedBackpackLMHeadModel(model, cw.to(DEV), None, 0.1, anneal=False, upweight_nearby=True).eval()
    ids = _ids(2)
    want = wrapper.generate(ids, MAX_LENGTH, kv_cache=True, cg=True)
    assert torch.equal(wrapper.generate(ids, MAX_LENGTH, kv_cache=True, cg=True, device_pick=True), want)
    a = wrapper.sample(ids, MAX_LENGTH, kv_cache=True, cg=True, rng_state=_state(), top_k=10, temperature=0.7)
    b = wrapper.sample(ids, MAX_LENGTH, kv_cache=True, rng_state=_state(), top_k=10, temperature=0.7)
    assert a.shape == (2, MAX_LENGTH - 1) and torch.equal(a[:, :PROMPT], ids) and torch.equal(a, b)
    assert ((a >= 0) & (a < cfg.vocab_size)).all()
