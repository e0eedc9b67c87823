"""GPU: bp_pick_report (csrc/pick_report.hip) through the C ABI, every record a view inside a NaN-filled buffer whose guard rows,
gap columns AND the record columns the call does not own must keep their bits (tests/rowwise_exact.py:Guarded), the logits a
strided view that starts any number of elements behind a 16-byte boundary; then the generation loops that call it.

  exact        rows of -128 with one 0 (tests/score_ref.py:spike_rows): entropy 0, logprob 0 / -128, every rank, every top column
               and top log-probability in closed form, bit for bit; the spike and the token walk the head / body / tail seams and
               the lane / wave seams of the row reader; mixed counters per row, so every call also checks its neighbours
  comparisons  rank and top_idx equal the numpy restatement (tests/pick_report_ref.py) entry for entry on 16-bit vocabulary rows
               (thousands of ties) and fp32 rows, NaN and signed-zero rows included; top_idx equals bp_row_extremes' top end on
               NaN-free rows without -0, and its first entry bp_hip.pick_token's greedy token on every row
  drawn rows   logprob / entropy / top_logprob against float64 within 4x the worst error of the fp32 CPU twin (_eager_report) on
               the same inputs, in the units of tests/score_ref.py -- the rule of tests/test_gpu_score_rows.py; both are printed
  columns      counters outside [0, rec_cols) leave the row's record alone
  repeatable   two calls give identical bits; the Python wrapper agrees with the raw ABI; every error code comes with no launch
  generation   small and mini_k4: the cg=True record is bit-identical to the cg=False one, which equals bp_hip.pick_report applied
               to the logits a recording wrapper kept; the weighted wrapper's table-form step too; sequences with and without the
               options are identical under one rng_state; a call without the options makes the calls it made

Measured on the MI355X (the tests print every figure, -s), in the units of tests/score_ref.py, kernel / twin: worst logprob 1.23 / 0.67,
entropy 1.28 / 0.71, top_logprob 1.55 / 0.94, all on 24 x 50264 fp32 rows of scale 0.05 (every term weighs the same); largest ratio 3.35
of the 4 allowed (fp16 logprob, same shape: 1.01 / 0.30); at scale 3 about 0.48 / 0.33.  Every spike case holds bit for bit.
"""
import ctypes
from unittest import mock

import numpy as np
import pytest
import torch

import pick_report_ref as P
import rowwise_exact as X
import score_ref as R
from decode_support import VOCAB, _model

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
F32 = torch.float32
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
PER16 = {'bf16': 8, 'fp16': 8, 'fp32': 4}
NAN_BITS = 0x7fc00000                                             # what Guarded fills with, as an int32
WAVES = 16


def _lib():
    import bp_hip
    return bp_hip.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:                                  # a GPU fault: nothing more may run on this device
        pytest.exit(f'{what}: {err}', returncode=3)


def report(x, tokens, counters, rec_cols, n_top, stride=None, offset=0, rec_stride=None, want=P.RECORDS, expect=0):
    """bp_pick_report on x (rows, vocab) torch tensor (its dtype) placed `offset` elements behind a 16-byte boundary with row
    stride `stride`; tokens, counters numpy (rows,).  Records: (rows, rec_cols) views of row stride rec_stride inside NaN
    buffers.  Returns (dict of numpy records -- what was not written holds NaN / NAN_BITS --, list of guard failures)."""
    rows, vocab = x.shape
    rec_stride = rec_stride or rec_cols
    logits = X.guarded_like(x.to(DEV), x.dtype, stride, offset)
    tbuf = torch.full((rows, 3), 12345, dtype=torch.int64, device=DEV)
    tbuf[:, 0] = torch.from_numpy(np.asarray(tokens, dtype=np.int64)).to(DEV)
    cbuf = torch.from_numpy(np.asarray(counters, dtype=np.int32)).to(DEV)
    out = {}
    for n in P.RECORDS:
        last = n_top if n.startswith('top_') else 1
        if n in want and last:
            out[n] = X.Guarded(rows, rec_cols * last, F32, DEV, stride=rec_stride * last)
    rc = _lib().bp_pick_report(logits.ptr(), tbuf.data_ptr(), cbuf.data_ptr(), *[out[n].ptr() if n in out else None for n in P.RECORDS],
                               rows, vocab, logits.view.stride(0), 3, rec_cols, rec_stride, n_top, X.DTYPE_CODE[x.dtype], _stream())
    _sync('bp_pick_report')
    assert rc == expect, rc
    bad = logits.failures('logits')
    assert torch.equal(tbuf[:, 1:], torch.full((rows, 2), 12345, dtype=torch.int64, device=DEV))
    assert torch.equal(cbuf.cpu(), torch.from_numpy(np.asarray(counters, dtype=np.int32)))
    res = {}
    for n, g in out.items():
        bad += g.failures(n)
        view = g.view.contiguous()
        view = view.view(torch.int32) if n in ('rank', 'top_idx') else view
        res[n] = view.cpu().numpy().reshape((rows, rec_cols, n_top) if n.startswith('top_') else (rows, rec_cols))
    return res, bad


def untouched(rows, rec_cols, n_top, names=P.RECORDS):
    """Records as Guarded leaves them: NaN, which reads NAN_BITS as an int32."""
    return {n: np.full((rows, rec_cols, n_top) if n.startswith('top_') else (rows, rec_cols),
                       NAN_BITS if n in ('rank', 'top_idx') else np.nan, dtype=P.DTYPES[n])
            for n in names if n_top or not n.startswith('top_')}


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _bits_equal(got, want):
    """got: the kernel's fp32 / int32 records; want: float64 / int64 arrays whose values are fp32 / int32 numbers."""
    return [n for n in got if not _same_bits(got[n], want[n].astype(np.int32 if n in ('rank', 'top_idx') else np.float32))]


# ---- exact ------------------------------------------------------------------------------------------------------------------------

def seam_columns(vocab, per16):
    """Columns worth a spike or a token: score_ref's (ends, head / body / tail seams) and the seams of vocab_row.h's RowView --
    wave w owns the chunks [w cpw, (w + 1) cpw), lane l of step s the chunk 64 s + l of them -- for every row alignment."""
    picks = set()
    for head in range(per16):
        picks.update(R.boundary_columns(vocab, (per16 - head) % per16, per16))
        nch = (vocab + head + per16 - 1) // per16
        cpw = (nch + WAVES - 1) // WAVES
        for chunk in (0, 1, 63, 64, 65, cpw - 1, cpw, cpw + 1, cpw + 64, 2 * cpw, (WAVES - 1) * cpw - 1, (WAVES - 1) * cpw, nch - 1):
            for inner in (0, per16 - 1):
                picks.add(chunk * per16 - head + inner)
    return sorted(p for p in picks if 0 <= p < vocab)


def spike_top(spikes, vocab, n):
    """Closed form of the top end of spike rows: the spike, then the other columns in ascending order; their log-probabilities."""
    idx = np.empty((len(spikes), n), dtype=np.int64)
    for r, s in enumerate(spikes):
        idx[r] = ([s] + [c for c in range(min(vocab, n + 1)) if c != s])[:n]
    return idx, np.where(np.arange(n)[None, :] == 0, 0.0, -128.0) * np.ones((len(spikes), 1))


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('vocab', [1, 2, 7, 8, 9, 15, 16, 17, 255, 256, 257, 2047, 2048, 2049, 8191, 8193, 50257, 50264])
def test_spike_rows_are_exact(vocab, dtype):
    per16 = PER16[dtype]
    picks = seam_columns(vocab, per16)
    odd = vocab + 1 + vocab % 2                                    # an odd row stride: 64 rows start at every alignment
    bad = []
    for rows, stride, offset, n_top in ((1, vocab, 0, min(16, vocab)), (3, vocab + 3, 1, min(5, vocab)), (64, odd, per16 - 1, min(2, vocab)),
                                        (64, vocab + 2 * per16, 3 % per16, min(1, vocab)), (3, vocab, 2, 0)):
        tag = f'{rows}x{vocab} stride {stride} offset {offset} n_top {n_top}'
        x, spikes = R.spike_rows(rows, vocab, picks[rows % 3:] + picks[:rows % 3])
        walk = np.array([picks[(5 * r + 1) % len(picks)] for r in range(rows)])
        choice = np.stack([spikes, walk, (spikes + 5) % vocab, np.full_like(spikes, -100), np.full_like(spikes, vocab),
                           (spikes * 7 + 1) % vocab], axis=1)
        tokens = choice[np.arange(rows), np.arange(rows) % 6]
        rec_cols, rec_stride = 3, 5
        counters = (np.arange(rows) * 2 + 1) % rec_cols
        got, fails = report(torch.from_numpy(x).to(DTYPES[dtype]), tokens, counters, rec_cols, n_top, stride, offset, rec_stride)
        bad += [f'{tag}: {f}' for f in fails]
        closed = R.spike_expected(spikes, tokens[:, None], vocab)
        want = untouched(rows, rec_cols, n_top)
        at = (np.arange(rows), counters)
        want['logprob'][at], want['rank'][at], want['entropy'][at] = closed['logprob'][:, 0], closed['rank'][:, 0], 0.0
        if n_top:
            want['top_idx'][at], want['top_logprob'][at] = spike_top(spikes, vocab, n_top)
        bad += [f'{tag}: {n}' for n in _bits_equal(got, want)]
    assert not bad, '; '.join(bad[:10])


# ---- comparisons ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def vocab_rows():
    """24 x 50264 fp32 draws with NaN, infinite and signed-zero rows, and a token per row."""
    x = R.drawn_rows(24, 50264, seed=21)
    x[3, [40000, 17]] = np.nan
    x[9, 50263] = np.nan
    x[15, 0], x[15, 1] = np.nan, np.inf
    x[5, x[5] > 0] = -1.0
    x[5, [30, 7000, 50000]] = [0.0, -0.0, 0.0]                     # the maximum is a zero at three columns
    x[6, 100:30000] = x[6, 100]
    tokens = R.drawn_targets(24, 50264, 1, seed=22)[:, 0]
    tokens[3], tokens[5], tokens[6], tokens[9] = 17, 7000, 15000, 5
    return x, tokens


@pytest.mark.parametrize('dtype', sorted(DTYPES))
def test_ranks_and_top_columns_equal_the_restatement_row_extremes_and_the_greedy_pick(vocab_rows, dtype):
    import bp_hip
    x32, tokens = vocab_rows
    x = torch.from_numpy(x32).to(DTYPES[dtype])
    x64 = x.double().numpy()
    rows, n = x.shape[0], 16
    if dtype != 'fp32':
        assert len(np.unique(x64[0])) < 50264 // 4                # 16-bit rows: thousands of ties by construction
    counters = np.zeros(rows, dtype=np.int64)
    got, bad = report(x, tokens, counters, 1, n, 50264 + 3, 1, want=('rank', 'top_idx'))
    want = P.pick_report(x64, tokens, counters, untouched(rows, 1, n, ('rank', 'top_idx')))
    assert np.array_equal(got['rank'], want['rank']) and np.array_equal(got['top_idx'], want['top_idx'])
    assert want['top_idx'][3, 0, :2].tolist() == [17, 40000] and want['top_idx'][15, 0, :2].tolist() == [0, 1]
    assert want['top_idx'][5, 0, :3].tolist() == [30, 7000, 50000] and want['rank'][5, 0] == 1
    plain = ~np.isnan(x64).any(axis=1) & ~((x64 == 0) & np.signbit(x64)).any(axis=1)
    assert plain.sum() >= 19
    ext = bp_hip.row_extremes(x.to(DEV), n, smallest=False)[1].cpu().numpy()
    assert np.array_equal(got['top_idx'][plain, 0], ext[plain])
    greedy = bp_hip.pick_token(x.to(DEV)).cpu().numpy()
    assert np.array_equal(got['top_idx'][:, 0, 0], greedy)
    # the token at top position i has rank i (NaN-free rows)
    nan_free = ~np.isnan(x64).any(axis=1)
    for i in (0, 1, 7, 15):
        again, fails = report(x, got['top_idx'][:, 0, i], counters, 1, 0, 50264 + 3, 1, want=('rank',))
        bad += fails
        assert (again['rank'][nan_free, 0] == i).all(), i
    assert not bad, '; '.join(bad[:10])


# ---- drawn rows -------------------------------------------------------------------------------------------------------------------

def _twin(x, tokens, counters, rec_cols, n_top):
    from src.utils.generation import _eager_report
    rows = x.shape[0]
    recs = {n: torch.zeros((rows, rec_cols, n_top) if n.startswith('top_') else (rows, rec_cols),
                           dtype=torch.int32 if n in ('rank', 'top_idx') else torch.float32) for n in P.RECORDS}
    _eager_report(x.cpu(), torch.from_numpy(tokens), torch.from_numpy(counters).int(), **recs)
    return {n: v.numpy() for n, v in recs.items()}


def _worst(rec, want, x64):
    """Worst errors of logprob, entropy and top_logprob at column 0, in the units of tests/score_ref.py."""
    with np.errstate(invalid='ignore'):
        res = R.worst_errors({'logprob': rec['logprob'], 'entropy': rec['entropy'][:, 0]},
                             {'logprob': want['logprob'], 'entropy': want['entropy'][:, 0]}, x64)
        res['top_logprob'] = R.worst_errors({'logprob': rec['top_logprob'][:, 0]}, {'logprob': want['top_logprob'][:, 0]}, x64)['logprob']
    return res


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('rows,vocab,scale', [(24, 50264, 3.0), (24, 50264, 0.05), (64, 2049, 12.0), (64, 257, 1.0)])
def test_drawn_rows_stay_within_four_times_the_twin(rows, vocab, scale, dtype):
    x = torch.from_numpy(R.drawn_rows(rows, vocab, seed=rows + vocab, scale=scale)).to(DTYPES[dtype])
    tokens = R.drawn_targets(rows, vocab, 1, seed=vocab)[:, 0]
    tokens = np.where((tokens < 0) | (tokens >= vocab), 1, tokens)
    counters = np.zeros(rows, dtype=np.int64)
    x64 = x.double().numpy()
    want = P.pick_report(x64, tokens, counters, P.new_records(rows, 1, 5))
    got, bad = report(x, tokens, counters, 1, 5, vocab + 2, 1)
    assert np.array_equal(got['rank'], want['rank']) and np.array_equal(got['top_idx'], want['top_idx'])
    mine, base = _worst(got, want, x64), _worst(_twin(x, tokens, counters, 1, 5), want, x64)
    tag = f'{dtype} {rows}x{vocab} scale {scale}'
    print(f'{tag}: error in units, kernel / twin: ' + ', '.join(f'{n} {mine[n]:.4f} / {base[n]:.4f}' for n in mine))
    for n in mine:
        assert mine[n] <= 4.0 * base[n], (tag, n, mine[n], base[n])
    assert not bad, '; '.join(bad[:10])


@pytest.mark.parametrize('dtype', sorted(DTYPES))
def test_degenerate_rows_follow_the_header(dtype):
    vocab, n = 2049, 4
    x = R.drawn_rows(6, vocab, seed=5)
    x[0, [700, 2048]] = np.nan
    x[1, [5, 1900]] = np.inf
    x[2] = -np.inf
    x[3, 11], x[3, 12] = np.inf, np.nan
    x[4, 1:] = -np.inf                                             # one finite entry: entropy 0, logprob 0
    x[5, :2040] = -np.inf
    tokens = np.array([1, 1900, 0, 11, 0, 2045])
    counters = np.zeros(6, dtype=np.int64)
    xt = torch.from_numpy(x).to(DTYPES[dtype])
    want = P.pick_report(xt.double().numpy(), tokens, counters, P.new_records(6, 1, n))
    got, bad = report(xt, tokens, counters, 1, n, vocab + 1, 1)
    assert np.array_equal(got['rank'], want['rank']) and np.array_equal(got['top_idx'], want['top_idx'])
    for name in ('logprob', 'entropy', 'top_logprob'):
        a, b = got[name].astype(np.float64), want[name]
        assert np.array_equal(np.isnan(a), np.isnan(b)), name
        inf = np.isinf(b)
        assert np.array_equal(np.isinf(a), inf) and np.array_equal(a[inf], b[inf]), name
    assert np.isnan(got['logprob'][[0, 1, 2, 3], 0]).all() and np.isnan(got['entropy'][:4, 0]).all()
    assert got['logprob'][4, 0] == 0 and got['entropy'][4, 0] == 0 and got['top_logprob'][4, 0].tolist() == [0, -np.inf, -np.inf, -np.inf]
    assert got['top_idx'][0, 0, :2].tolist() == [700, 2048] and got['top_idx'][3, 0, :2].tolist() == [12, 11]
    assert got['top_idx'][2, 0].tolist() == [0, 1, 2, 3]
    assert not bad, '; '.join(bad[:10])


# ---- columns ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_a_counter_out_of_range_leaves_the_record_alone(dtype):
    rows, vocab, rec_cols, n = 7, 4099, 4, 3
    x = torch.from_numpy(R.drawn_rows(rows, vocab, seed=31)).to(DTYPES[dtype])
    tokens = np.arange(rows) * 500
    counters = np.array([-1, rec_cols, 0, 3, -2 ** 31, 2 ** 31 - 1, 2])
    got, bad = report(x, tokens, counters, rec_cols, n, vocab + 1, 3, rec_stride=7)
    want = P.pick_report(x.double().numpy(), tokens, counters, untouched(rows, rec_cols, n))
    written = np.zeros((rows, rec_cols), dtype=bool)
    written[[2, 3, 6], [0, 3, 2]] = True
    for name in P.RECORDS:
        assert np.array_equal(np.isnan(got[name].astype(np.float64)) if name not in ('rank', 'top_idx') else got[name] == NAN_BITS,
                              np.broadcast_to(~written.reshape(written.shape + (1,) * (got[name].ndim - 2)), got[name].shape)), name
    assert np.array_equal(got['rank'], want['rank']) and np.array_equal(got['top_idx'], want['top_idx'])
    assert not bad, '; '.join(bad[:10])


# ---- repeatable, the Python wrapper, the error codes ------------------------------------------------------------------------------

def test_two_calls_agree_bit_for_bit_and_the_wrapper_agrees_with_the_abi(vocab_rows):
    import bp_hip
    x32, tokens = vocab_rows
    x = torch.from_numpy(x32).bfloat16()
    rows, rec_cols, n = x.shape[0], 3, 5
    counters = np.arange(rows) % rec_cols
    a, bad = report(x, tokens, counters, rec_cols, n, 50264 + 8, 0, rec_stride=4)
    b, _ = report(x, tokens, counters, rec_cols, n, 50264 + 8, 0, rec_stride=4)
    for name in P.RECORDS:
        assert _same_bits(a[name], b[name]), name
    nan = float('nan')
    recs = {name: torch.full((rows, 4, n) if name.startswith('top_') else (rows, 4), nan, dtype=F32, device=DEV)
            for name in P.RECORDS}
    recs['rank'], recs['top_idx'] = recs['rank'].view(torch.int32), recs['top_idx'].view(torch.int32)
    ids = torch.from_numpy(tokens).to(DEV).unsqueeze(1)            # (B, 1), as the decode step's static_ids
    bp_hip.pick_report(x.to(DEV), ids, torch.from_numpy(counters).int().to(DEV), **{k: v[:, :rec_cols] for k, v in recs.items()})
    _sync('bp_hip.pick_report')
    for name in P.RECORDS:
        assert _same_bits(recs[name][:, :rec_cols].contiguous().cpu().numpy(), a[name]), name
        assert (recs[name][:, rec_cols:].contiguous().view(torch.int32) == NAN_BITS).all(), name
    only = torch.zeros((rows, rec_cols), dtype=F32, device=DEV)
    bp_hip.pick_report(x.to(DEV), ids, torch.from_numpy(counters).int().to(DEV), entropy=only)
    at = (np.arange(rows), counters)
    assert _same_bits(only.cpu().numpy()[at], a['entropy'][at])
    assert bp_hip.pick_report_supported(x.to(DEV), 16) and not bp_hip.pick_report_supported(x.to(DEV), 17)
    with pytest.raises(RuntimeError):
        bp_hip.pick_report(x.to(DEV), ids, torch.from_numpy(counters).int().to(DEV))
    with pytest.raises(RuntimeError):                              # two widths
        bp_hip.pick_report(x.to(DEV), ids, torch.from_numpy(counters).int().to(DEV), logprob=recs['logprob'][:, :2], entropy=only)
    assert not bad, '; '.join(bad[:10])


def test_every_error_code_is_returned_before_any_launch():
    lib = _lib()
    rows, vocab, cols, n = 2, 64, 3, 2
    x = torch.zeros((rows, vocab), dtype=F32, device=DEV)
    tok = torch.zeros((rows,), dtype=torch.int64, device=DEV)
    cnt = torch.zeros((rows,), dtype=torch.int32, device=DEV)
    rec = {k: torch.full((rows, cols * (n if k.startswith('top_') else 1)), float('nan'), dtype=F32, device=DEV) for k in P.RECORDS}
    good = dict(logits=x.data_ptr(), tokens=tok.data_ptr(), counters=cnt.data_ptr(), logprob=rec['logprob'].data_ptr(),
                rank=rec['rank'].data_ptr(), entropy=rec['entropy'].data_ptr(), top_idx=rec['top_idx'].data_ptr(),
                top_logprob=rec['top_logprob'].data_ptr(), rows=rows, vocab=vocab, row_stride=vocab, tokens_stride=1, rec_cols=cols,
                rec_stride=cols, n_top=n, dtype=2)

    def call(**change):
        a = dict(good, **change)
        return lib.bp_pick_report(*[a[k] for k in good], _stream())
    DTYPE, SHAPE = -1, -3
    assert call(dtype=3) == DTYPE and call(dtype=-1) == DTYPE
    for change in (dict(rows=0), dict(rows=-1), dict(vocab=0), dict(vocab=0x7fffffff - 15), dict(row_stride=vocab - 1),
                   dict(tokens_stride=0), dict(rec_cols=0), dict(rec_stride=cols - 1), dict(n_top=-1), dict(n_top=17),
                   dict(vocab=1, row_stride=1, n_top=2), dict(top_idx=None, top_logprob=None),
                   dict(logits=None), dict(tokens=None), dict(counters=None),
                   dict(logprob=None, rank=None, entropy=None, top_idx=None, top_logprob=None, n_top=0),
                   dict(logits=x.data_ptr() + 2), dict(tokens=tok.data_ptr() + 4), dict(counters=cnt.data_ptr() + 2),
                   dict(logprob=rec['logprob'].data_ptr() + 2), dict(rank=rec['rank'].data_ptr() + 1),
                   dict(entropy=rec['entropy'].data_ptr() + 2), dict(top_idx=rec['top_idx'].data_ptr() + 2),
                   dict(top_logprob=rec['top_logprob'].data_ptr() + 3)):
        assert call(**change) == SHAPE, change
    half = x.to(torch.bfloat16)
    assert call(logits=half.data_ptr() + 1, dtype=1) == SHAPE
    _sync('bp_pick_report argument checks')
    for k, v in rec.items():
        assert torch.isnan(v).all(), f'{k} was written by a refused call'
    assert call() == 0 and call(n_top=0) == 0 and call(top_idx=None) == 0 and call(n_top=0, top_idx=None, top_logprob=None) == 0
    _sync('bp_pick_report')
    assert not torch.isnan(rec['logprob'][:, 0]).any() and torch.isnan(rec['logprob'][:, 1:]).all()


# ---- generation -------------------------------------------------------------------------------------------------------------------

PROMPT, NEW = 8, 24
FIELDS = {'logprob': 'token_logprobs', 'rank': 'token_ranks', 'entropy': 'token_entropies', 'top_idx': 'top_token_ids',
          'top_logprob': 'top_token_logprobs'}


class Recording(torch.nn.Module):
    """Keeps logits[:, -1] of every cached step (eager runs only; the prefill's pick takes what the result returns as `scores`)."""

    def __init__(self, model):
        super().__init__()
        self.model, self.steps, self.calls = model, [], 0

    def forward(self, input_ids, inference_params=None, **kw):
        out = self.model(input_ids, inference_params=inference_params, **kw)
        if self.calls:
            self.steps.append(out.logits[:, -1].detach().clone())
        self.calls += 1
        return out


def _ids(batch, seed=5):
    return torch.randint(0, VOCAB, (batch, PROMPT), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _state():
    return torch.tensor([1234, 77], dtype=torch.int64, device=DEV)


def _record_bits(out):
    return {n: getattr(out, f).contiguous().view(torch.int32).cpu() for n, f in FIELDS.items() if getattr(out, f) is not None}


def _replayed(out, step_logits, n_top):
    """bp_hip.pick_report on the kept logits of every step, into records at their initial values, then the trim."""
    import bp_hip
    seq = out.sequences
    batch, width = seq.shape
    recs = {'logprob': torch.zeros((batch, width), dtype=F32, device=DEV), 'rank': torch.full((batch, width), -1, dtype=torch.int32, device=DEV),
            'entropy': torch.zeros((batch, width), dtype=F32, device=DEV),
            'top_idx': torch.full((batch, width, n_top), -1, dtype=torch.int32, device=DEV),
            'top_logprob': torch.zeros((batch, width, n_top), dtype=F32, device=DEV)}
    ends = out.lengths if out.lengths is not None else torch.full((batch,), width, device=DEV)
    for s, lg in enumerate(step_logits):
        col = PROMPT + s
        if col >= width:
            break
        live = col < ends
        counters = torch.where(live, col, -1).to(torch.int32)     # a row past its end: no column
        bp_hip.pick_report(lg, seq[:, col].contiguous(), counters, **recs)
    return {n: v.view(torch.int32).cpu() for n, v in recs.items()}


def _check_generation(model, decode, tag):
    from src.utils import generation as G
    fn = getattr(G, {'generate': 'greedy_decode', 'sample': 'sample'}[decode])
    ids, n, n_top = _ids(3), PROMPT + NEW, 5
    kw = dict(kv_cache=True, rng_state=_state(), top_k=50) if decode == 'sample' else dict(kv_cache=True, device_pick=True)
    free = fn(ids, model, n, cg=True, **kw).sequences
    eos = int(free[0, PROMPT + 3])
    plain = fn(ids, model, n, eos_token_id=eos, **kw)
    rec = Recording(model)
    eager = fn(ids, rec, n, eos_token_id=eos, stop_check_every=1, output_logprobs=True, top_logprobs=n_top, **kw)
    graph = fn(ids, model, n, cg=True, eos_token_id=eos, stop_check_every=2, output_logprobs=True, top_logprobs=n_top, **kw)
    late = fn(ids, model, n, cg=True, eos_token_id=eos, output_logprobs=True, top_logprobs=n_top, **kw)
    _sync(tag)
    assert int(plain.lengths[0]) <= PROMPT + 4 < n - 1
    want = _replayed(eager, [eager.scores[0]] + rec.steps, n_top)
    bits = _record_bits(eager)
    assert sorted(bits) == sorted(FIELDS)
    for out in (eager, graph, late):
        assert torch.equal(out.sequences, plain.sequences) and torch.equal(out.lengths, plain.lengths), tag
        got = _record_bits(out)
        for name in FIELDS:
            assert got[name].shape[:2] == tuple(out.sequences.shape), (tag, name)
            assert torch.equal(got[name], want[name]), (tag, name)
    lp, rank = eager.token_logprobs.cpu(), eager.token_ranks.cpu()
    for b in range(3):
        end = int(eager.lengths[b])
        assert (rank[b, :PROMPT] == -1).all() and (rank[b, PROMPT:end] >= 0).all() and (rank[b, end:] == -1).all()
        assert (lp[b, :PROMPT] == 0).all() and (lp[b, PROMPT:end] < 0).all() and (lp[b, end:] == 0).all()
    if decode == 'generate':
        assert (rank[:, PROMPT:] <= 0).all()
        live = rank[:, PROMPT:] == 0
        assert torch.equal(eager.top_token_ids[:, PROMPT:, 0].cpu()[live], eager.sequences[:, PROMPT:].cpu()[live].int())


@pytest.mark.parametrize('decode', ['generate', 'sample'])
@pytest.mark.parametrize('name', ['small', 'mini_k4'])
def test_generation_records_eager_and_graphed(name, decode):
    _check_generation(_model(name, seed=2), decode, f'{name} {decode}')


def test_the_weighted_wrapper_records_its_table_form_step():
    from src.models.intervened_models import WeightedBackpackLMHeadModel
    model = _model('small', seed=4)
    cw = torch.rand(model.lm_head.weight.shape[0], model.config.num_content_vectors, generator=torch.Generator().manual_seed(11)) * 3
    wrapper = WeightedBackpackLMHeadModel(model, cw.to(DEV), None, 0.1, anneal=False, upweight_nearby=True).eval()
    _check_generation(wrapper, 'generate', 'weighted generate')
    out = wrapper.sample(_ids(2), PROMPT + 6, kv_cache=True, cg=True, rng_state=_state(), output_logprobs=True, return_dict_in_generate=True)
    assert out.token_logprobs.shape == (2, PROMPT + 5) and out.top_token_ids is None


def test_a_call_without_the_options_makes_the_calls_it_made():
    """(entry point, device) of every bp_hip._call: the record adds bp_pick_report right behind every pick and nothing else, and
    a call without the options never reaches it.  profiles/pick_report_call_sequences.txt compares the latter with the parent."""
    import bp_hip
    model = _model('small', seed=2)
    ids, n = _ids(2), PROMPT + 6
    real = bp_hip._call

    def traced(**kw):
        calls = []

        def spy(name, device, *args):
            calls.append((name, str(device)))
            return real(name, device, *args)
        with mock.patch.object(bp_hip, '_call', spy):
            model.sample(ids, n, kv_cache=True, rng_state=_state(), **kw)
        _sync('traced generation')
        return calls
    model.sample(ids, n, kv_cache=True, rng_state=_state())      # the first call of a model also builds its cached sense table
    for cg in (False, True):
        plain = traced(cg=cg)
        with_record = traced(cg=cg, output_logprobs=True, top_logprobs=3)
        assert plain and not any(name == 'bp_pick_report' for name, _ in plain)
        picks = [i for i, (name, _) in enumerate(with_record) if name.startswith('bp_pick_token')]
        assert picks and all(with_record[i + 1][0] == 'bp_pick_report' for i in picks)
        assert [c for c in with_record if c[0] != 'bp_pick_report'] == plain
        assert sum(name == 'bp_pick_report' for name, _ in with_record) == len(picks)
