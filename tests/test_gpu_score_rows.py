"""GPU: bp_score_rows (csrc/score_rows.hip) through the C ABI, every output a view inside a NaN-filled buffer whose guard rows
and gap columns must keep their bits (tests/rowwise_exact.py:Guarded), the logits a strided view that starts any number of
elements behind a 16-byte boundary.

  exact        rows of -128 with one 0 (tests/score_ref.py:spike_rows): lse = entropy = 0, logprob 0 / -128, top1 and every rank
               in closed form, bit for bit; the spike walks the head / body / tail seams and the lane, wave and workgroup seams
  comparisons  rank and top1 equal the numpy restatement entry for entry on 16-bit vocabulary rows (thousands of ties) and on
               fp32 rows; top1 equals bp_hip.pick_token's greedy token, NaN rows included
  targets      M = 1 .. 8 with repeated, tied and out-of-range targets; M = 1 and the general form agree on column 0
  specials     -inf entries, a row of -inf, +inf and NaN rows follow the rule written in include/bp_hip.h
  drawn rows   lse / logprob / entropy against float64 within 4x the worst error of the fp32 CPU twin on the same inputs, in
               the units of tests/score_ref.py (the twin's summation order is not the kernel's); both figures are printed
  repeatable   two calls give identical bits

Measured on the MI355X (the tests print every figure, -s), in the units of tests/score_ref.py, kernel / twin: worst lse 1.20 / 0.59,
logprob 1.34 / 0.88, entropy 1.28 / 0.71, all on 24 x 50264 fp32 rows of scale 0.05 (every term weighs the same; a thread's serial
sum of ~200 terms against torch's pairwise one); largest ratio 3.35 of the 4 allowed (fp16, same shape: 1.01 / 0.30); at scale 3
about 0.25 / 0.19.  v_exp_f32 beyond its range and logf(1) are exact: every spike case holds bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch

import rowwise_exact as X
import score_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
F32 = torch.float32
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
PER16 = {'bf16': 8, 'fp16': 8, 'fp32': 4}


def _lib():
    import bp_hip
    return bp_hip.lib()


def score(x, targets, stride=None, offset=0, want=R.OUTPUTS, gap=3):
    """bp_score_rows on x (rows, cols) torch tensor (its dtype) placed at `offset` elements behind a 16-byte boundary with row
    stride `stride`; targets (rows, M) int64 numpy.  Returns (dict of numpy outputs, list of guard failures)."""
    rows, cols = x.shape
    m = targets.shape[1]
    logits = X.guarded_like(x.to(DEV), x.dtype, stride, offset)
    tbuf = torch.full((rows, m + 2), 12345, dtype=torch.int64, device=DEV)
    tbuf[:, :m] = torch.from_numpy(targets).to(DEV)
    out = {'logprob': X.Guarded(rows, m, F32, DEV, stride=m + gap), 'rank': X.Guarded(rows, m, F32, DEV, stride=m + gap),
           'lse': X.Guarded(1, rows, F32, DEV), 'top1': X.Guarded(1, rows, F32, DEV), 'entropy': X.Guarded(1, rows, F32, DEV)}
    ptrs = [out[n].ptr() if n in want else None for n in R.OUTPUTS]
    rc = _lib().bp_score_rows(logits.ptr(), tbuf.data_ptr(), *ptrs, rows, cols, m, logits.view.stride(0), m + 2, m + gap,
                              X.DTYPE_CODE[x.dtype], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:                                  # a GPU fault: nothing more may run on this device
        pytest.exit(f'bp_score_rows: {err}', returncode=3)
    assert rc == 0, rc
    bad = logits.failures('logits')
    assert torch.equal(tbuf[:, m:], torch.full((rows, 2), 12345, dtype=torch.int64, device=DEV))
    res = {}
    for n in R.OUTPUTS:
        bad += out[n].failures(n)
        view = out[n].view if n in ('logprob', 'rank') else out[n].view[0]
        if n not in want:
            assert torch.isnan(view).all(), f'{n} was written though not asked for'
            continue
        res[n] = (view.contiguous().view(torch.int32) if n in ('rank', 'top1') else view).cpu().numpy()
    return res, bad


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- exact ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('cols', [1, 7, 8, 9, 2047, 2048, 2049, 4099, 50264])
def test_spike_rows_are_exact(cols, dtype):
    per16 = PER16[dtype]
    picks = sorted({c for head in range(per16) for c in R.boundary_columns(cols, head, per16)})
    bad = []
    for rows, stride, offset in ((1, cols, 0), (3, cols + 1, 1), (257, cols + per16 + 3, per16 - 1), (257, cols, 2)):
        x, spikes = R.spike_rows(rows, cols, picks[rows % 3:] + picks[:rows % 3])
        tag = f'{rows}x{cols} stride {stride} offset {offset}'
        one = spikes[:, None]
        got, fails = score(torch.from_numpy(x).to(DTYPES[dtype]), one, stride, offset)
        bad += fails
        want = R.spike_expected(spikes, one, cols)
        bad += [f'{tag} M=1 {n}' for n in R.OUTPUTS if not _same_bits(got[n], want[n])]
        many = np.stack([spikes, (spikes + 5) % cols, np.full_like(spikes, min(2, cols - 1)), np.full_like(spikes, -100),
                         (spikes * 7 + 1) % cols, np.full_like(spikes, cols)], axis=1)
        got, fails = score(torch.from_numpy(x).to(DTYPES[dtype]), many, stride, offset)
        bad += fails
        want = R.spike_expected(spikes, many, cols)
        bad += [f'{tag} M=6 {n}' for n in R.OUTPUTS if not _same_bits(got[n], want[n])]
    assert not bad, '; '.join(bad[:10])


# ---- comparisons ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def vocab_rows():
    """24 x 50264 fp32 draws, three of them with NaNs, and their int64 targets."""
    x = R.drawn_rows(24, 50264, seed=11)
    x[3, 40000] = np.nan
    x[3, 17] = np.nan
    x[9, 50263] = np.nan
    x[15, 0] = np.nan
    x[15, 1] = np.inf
    targets = R.drawn_targets(24, 50264, 8, seed=12)
    targets[3, 0], targets[9, 0] = 17, 5
    return x, targets


@pytest.mark.parametrize('dtype', sorted(DTYPES))
def test_rank_and_top1_are_exact_and_top1_is_the_greedy_pick(vocab_rows, dtype):
    import bp_hip
    x32, targets = vocab_rows
    x = torch.from_numpy(x32).to(DTYPES[dtype])
    x64 = x.double().numpy()
    if dtype != 'fp32':
        assert len(np.unique(x64[0])) < 50264 // 4                # 16-bit rows: thousands of ties by construction
    bad = []
    for m, stride, offset in ((1, 50264, 0), (8, 50264 + 3, 1)):
        tg = targets[:, :m]
        got, fails = score(x, tg, stride, offset, want=('rank', 'top1'))
        want = R.score_rows(x64, tg)
        bad += fails
        assert np.array_equal(got['rank'], want['rank']), f'M={m}: rank'
        assert np.array_equal(got['top1'], want['top1']), f'M={m}: top1'
        nan_free = ~np.isnan(x64).any(axis=1)
        assert np.array_equal((got['rank'] == 0)[nan_free], (tg == got['top1'][:, None])[nan_free])
    greedy = bp_hip.pick_token(x.to(DEV)).cpu().numpy()
    assert np.array_equal(greedy, want['top1'])
    assert want['top1'][3] == 17 and want['top1'][9] == 50263 and want['top1'][15] == 0
    assert not bad, '; '.join(bad[:10])


# ---- targets ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('m', range(1, 9))
def test_every_target_count(m, dtype):
    rows, cols = 37, 4099
    x = torch.from_numpy(R.drawn_rows(rows, cols, seed=m, minus_inf=0.05)).to(DTYPES[dtype])
    x[1, 100:3000] = x[1, 100]                                    # a run of ties across many chunks, targets inside it
    targets = R.drawn_targets(rows, cols, m, seed=100 + m)
    targets[1, :] = np.array([100, 2999, 1500, 99, 3000, 100, 0, 4098])[:m]
    x64 = x.double().numpy()
    want = R.score_rows(x64, targets)
    got, bad = score(x, targets, cols + 5, 3)
    assert np.array_equal(got['rank'], want['rank']) and np.array_equal(got['top1'], want['top1'])
    outside = (targets < 0) | (targets >= cols)
    assert outside.any() or m == 1
    assert (got['rank'][outside] == -1).all() and _same_bits(got['logprob'][outside], np.zeros(outside.sum(), np.float32))
    assert np.isfinite(got['entropy']).all() and np.isfinite(want['entropy']).all()   # -inf entries contribute 0
    twin = _twin(x, targets)
    _within_four_twins(got, twin, want, x64, f'{dtype} M={m}', ~outside)
    first, fails = score(x, targets[:, :1], cols + 5, 3)          # the M = 1 kernel against column 0 of the general form
    bad += fails
    for n in ('lse', 'top1', 'entropy'):
        assert _same_bits(first[n], got[n]), n
    assert _same_bits(first['logprob'][:, 0], got['logprob'][:, 0]) and np.array_equal(first['rank'][:, 0], got['rank'][:, 0])
    assert not bad, '; '.join(bad[:10])


# ---- specials ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', sorted(DTYPES))
def test_degenerate_rows_follow_the_header(dtype):
    cols = 2049
    x = R.drawn_rows(7, cols, seed=5)
    x[0, 700] = np.nan
    x[0, 2048] = np.nan
    x[1, 5] = np.inf
    x[1, 1900] = np.inf
    x[2] = -np.inf
    x[3, 11] = np.inf
    x[3, 12] = np.nan
    x[4, 1:] = -np.inf                                            # one finite entry: entropy 0, lse = x, logprob 0
    x[5, :2040] = -np.inf                                         # only the tail is finite
    x[6, 3] = -0.0
    x[6, 2047] = 0.0
    x[6, x[6] > 0] = -1.0                                         # the maximum is a zero at two columns: the lower one wins
    targets = np.array([[700, 1], [5, 1], [0, 2048], [11, 12], [0, 1], [2045, 3], [2047, 3]], dtype=np.int64)
    xt = torch.from_numpy(x).to(DTYPES[dtype])
    x64 = xt.double().numpy()
    want = R.score_rows(x64, targets)
    got, bad = score(xt, targets, cols + 1, 1)
    assert np.array_equal(got['rank'], want['rank']) and np.array_equal(got['top1'], want['top1'])
    assert got['top1'].tolist() == [700, 5, 0, 12, 0, int(np.argmax(x64[5])), 3]
    assert got['rank'][0, 0] == 0 and got['rank'][3, 1] == 0      # the rank of a NaN target is 0
    assert got['rank'][6].tolist() == [1, 0]
    for n in ('lse', 'entropy', 'logprob'):
        a, b = got[n].astype(np.float64), want[n]
        assert np.array_equal(np.isnan(a), np.isnan(b)), n
        inf = np.isinf(b)
        assert np.array_equal(np.isinf(a), inf) and np.array_equal(np.sign(a[inf]), np.sign(b[inf])), n
    assert np.isnan(got['lse'][[0, 3]]).all() and np.isnan(got['entropy'][:4]).all() and np.isnan(got['logprob'][[0, 2, 3]]).all()
    assert got['lse'][1] == np.inf and np.isnan(got['logprob'][1, 0]) and got['logprob'][1, 1] == -np.inf
    assert got['lse'][2] == -np.inf
    assert got['lse'][4] == x64[4, 0] and got['entropy'][4] == 0 and got['logprob'][4, 0] == 0 and got['logprob'][4, 1] == -np.inf
    assert not bad, '; '.join(bad[:10])


# ---- drawn rows -------------------------------------------------------------------------------------------------------------------

def _twin(x, targets):
    from src.utils.scoring import _eager_score_rows
    res = _eager_score_rows(x.cpu(), torch.from_numpy(targets))
    return {n: v.numpy() for n, v in res.items()}


def _within_four_twins(got, twin, want, x64, tag, scored=None):
    """The project's rule for row-wise kernels: the kernel's worst error against float64 is at most 4x that of the fp32
    evaluation of the same formulas on the CPU (the twin), per output, in the units of tests/score_ref.py."""
    real = ('lse', 'logprob', 'entropy')
    with np.errstate(invalid='ignore'):
        mine = R.worst_errors({n: got[n] for n in real}, want, x64, scored)
        base = R.worst_errors({n: twin[n] for n in real}, want, x64, scored)
    print(f'{tag}: error in units, kernel / twin: ' + ', '.join(f'{n} {mine[n]:.4f} / {base[n]:.4f}' for n in real))
    for n in real:
        assert mine[n] <= 4.0 * base[n], (tag, n, mine[n], base[n])


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('rows,cols,scale', [(24, 50264, 3.0), (24, 50264, 0.05), (64, 2049, 12.0), (64, 257, 1.0)])
def test_drawn_rows_stay_within_four_times_the_twin(rows, cols, scale, dtype):
    x = torch.from_numpy(R.drawn_rows(rows, cols, seed=rows + cols, scale=scale)).to(DTYPES[dtype])
    targets = R.drawn_targets(rows, cols, 2, seed=cols)
    x64 = x.double().numpy()
    want = R.score_rows(x64, targets)
    got, bad = score(x, targets, cols + 2, 1)
    assert np.array_equal(got['rank'], want['rank']) and np.array_equal(got['top1'], want['top1'])
    _within_four_twins(got, _twin(x, targets), want, x64, f'{dtype} {rows}x{cols} scale {scale}', want['rank'] >= 0)
    assert not bad, '; '.join(bad[:10])


# ---- repeatable, and the Python wrapper -------------------------------------------------------------------------------------------

def test_two_calls_agree_bit_for_bit_and_the_wrapper_agrees_with_the_abi(vocab_rows):
    import bp_hip
    x32, targets = vocab_rows
    x = torch.from_numpy(x32).bfloat16()
    a, bad = score(x, targets[:, :3], 50264 + 8, 0)
    b, _ = score(x, targets[:, :3], 50264 + 8, 0)
    for n in R.OUTPUTS:
        assert _same_bits(a[n], b[n]), n
    res = bp_hip.score_rows(x.to(DEV), torch.from_numpy(targets[:, :3]).to(DEV))
    for n in R.OUTPUTS:
        assert _same_bits(res[n].cpu().numpy(), a[n]), n
    flat = bp_hip.score_rows(x.to(DEV), torch.from_numpy(targets[:, 0].copy()).to(DEV), want=('logprob', 'top1'))
    assert sorted(flat) == ['logprob', 'top1'] and flat['logprob'].shape == (24,)
    assert _same_bits(flat['logprob'].cpu().numpy(), np.ascontiguousarray(a['logprob'][:, 0]))
    assert not bad, '; '.join(bad[:10])
