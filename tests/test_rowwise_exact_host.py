"""CPU: the inputs of tests/test_gpu_rowwise_exact.py (tests/rowwise_exact.py) do what that file relies on.  For every case
the GPU file runs: the inputs and the expected outputs are representable as claimed (integers and powers of two, exact in bf16
and fp16, partial sums below 2^24, fp64 expectations that are fp32 numbers), a plain fp32 torch evaluation of the operation
meets every criterion, and named mutants of that evaluation do NOT -- the proof that the GPU tests can fail:

  column sums      a row dropped; a row counted twice; row r taking the `pre` of row r + 1
  bias + GELU      the bias of the neighbouring column
  cross-entropy    the last tail element dropped from the log-sum-exp; the head's last element written by the vector path
  LayerNorm fwd    the spike left out of the mean, left out of the variance, counted twice (>= 100x the fp32 bound, every width)
  LayerNorm bwd    the second grid-stride trip dropped from, or counted twice in, the column sums
  softmax bwd      the last live column left out of the row sum

It also measures the two recorded bounds (rowwise_exact.LN_FWD_F32_BOUND, LN_BWD_BOUND) and asserts that each is 4x the worst
error of the fp32 evaluation, and pins the tiling arithmetic (trips of the unrolled loops, CH tables) the cases aim at."""
import os

import pytest
import torch

import rowwise_exact as R

DTYPES = (torch.bfloat16, torch.float16)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'backpacks-flash-attn_amd', 'csrc')


def _representable(x64, dtype, tag):
    assert torch.equal(x64.to(dtype).double(), x64), f'{tag}: not representable in {dtype}'


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_guard_sees_a_stray_write():
    for dtype in (torch.bfloat16, torch.float32):
        g = R.Guarded(3, 5, dtype, 'cpu', stride=7, offset=1)
        g.view.fill_(1.0)
        assert g.failures('x') == [] and g.ptr() % 16 == g.view.element_size()
        g.buf[g.geometry[2] + 5] = 0.0                       # a gap column
        assert g.failures('x')
        g = R.Guarded(3, 8, dtype, 'cpu')
        g.buf.view(R.BITS[dtype])[g.geometry[2] - 1] = g.nan_bits ^ 1      # another NaN is another bit pattern
        g.buf[g.geometry[2] + 24] = 1.0
        assert '2 wrong' in g.failures('x')[0]


# ---- 1. column sums and the GELU backward ------------------------------------------------------------------------------------

def test_tiling_constants_are_the_sources():
    """The constants this module restates, where the library exposes none."""
    gelu = _source('bias_gelu.hip')
    assert f'if (wgs > {R.GELU_FWD_MAX_WG}) wgs = {R.GELU_FWD_MAX_WG};' in gelu
    assert 'constexpr int kGeluBwdRows = 4;' in gelu and 'bias_gelu_bwd_kernel<ET, false, 8>' in gelu
    assert f'kBiasGeluMaxSlices = {R.BIAS_GELU_MAX_SLICES};' in _source('bp_kernels.h')
    ln = _source('add_layer_norm.hip')
    assert 'with_bound<%s>(chunks, hipErrorInvalidValue' % ', '.join(map(str, R.LN_CH_LIST)) in ln
    assert 'with_bound<%s>(chunks, hipErrorNotSupported' % ', '.join(map(str, R.LN_BWD_CH_LIST)) in ln
    assert 'with_bound<1, 2, 4, 8>((p.s + 511) / 512' in _source('softmax_bwd.hip')


@pytest.mark.parametrize('shape', list(R.COLSUM_CASES), ids=lambda s: 'x'.join(map(str, s)))
def test_column_sums(shape):
    rows, cols = shape
    slices = R.bias_gelu_slices(rows, cols)
    for u, want in R.COLSUM_CASES[shape].items():
        assert R.trip_summary(rows, slices, u) == want
    for u, shapes in R.COLSUM_MAIN_AND_TAIL.items():
        if shape in shapes:
            main, tail = R.unrolled_trips(rows, slices, u)
            assert main.max() >= 1 and tail.max() >= 1
    prob = R.colsum_problem(rows, cols, 'cpu')
    assert prob['g'].abs().min() >= 1 and prob['g'].abs().sum(0).max() < 2 ** 24
    for dtype in DTYPES:
        for k in ('g', 'pre', 'dpre'):
            _representable(prob[k], dtype, k)

        def evaluate(g, pre, weight=None):
            dpre = (g.float() * R.gelu_grad32(pre.float())).to(dtype)
            terms = dpre.float() if weight is None else dpre.float() * weight[:, None]
            plain = g.float() if weight is None else g.float() * weight[:, None]
            return dpre, terms.sum(0), plain.sum(0)

        def failures(dpre, dbias, colsum, out):
            return (R.exact_failures(dpre, prob['dpre'], dtype, 'dpre') + R.exact_failures(dbias.to(out), prob['dbias'], out, 'dbias')
                    + R.exact_failures(colsum.to(out), prob['colsum'], out, 'colsum'))

        for out in (torch.float32, dtype):
            assert failures(*evaluate(prob['g'], prob['pre']), out) == []
        if dtype != torch.bfloat16:
            continue
        for factor in (0.0, 2.0):                            # a row dropped, a row counted twice
            weight = torch.ones(rows)
            weight[rows // 2] = factor
            bad = failures(*evaluate(prob['g'], prob['pre'], weight), torch.float32)
            assert any('dbias' in b for b in bad) and any('colsum' in b for b in bad)
        if rows > 1:
            bad = failures(*evaluate(prob['g'], prob['pre'].roll(-1, 0)), torch.float32)
            assert any('dpre' in b for b in bad)


# ---- 2. bias + GELU forward --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', R.GELU_FWD_CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_bias_gelu_forward(shape):
    rows, cols = shape
    assert R.gelu_fwd_trips(rows, cols) == {(3, 8): (0, 1), (257, 1032): (0, 1), (4100, 4096): (1, 2)}[shape]
    for with_bias in (False, True):
        prob = R.gelu_fwd_problem(rows, cols, 'cpu', with_bias)
        assert prob['pre'].abs().min() >= 8 and prob['pre'].abs().max() <= 120
        for dtype in DTYPES:
            for k in ('x', 'pre', 'y') + (('bias',) if with_bias else ()):
                _representable(prob[k], dtype, k)
            bias = prob['bias'] if with_bias else torch.zeros(cols, dtype=torch.float64)
            pre = (prob['x'].float() + bias.float()).to(dtype)
            assert R.exact_failures(pre, prob['pre'], dtype, 'pre') == []
            assert R.exact_failures(R.gelu_fwd32(pre.float()).to(dtype), prob['y'], dtype, 'y') == []
            if with_bias and dtype == torch.bfloat16:
                wrong = (prob['x'].float() + bias.float().roll(1)).to(dtype)
                assert R.exact_failures(R.gelu_fwd32(wrong.float()).to(dtype), prob['y'], dtype, 'y')


# ---- 3. cross-entropy --------------------------------------------------------------------------------------------------------

def _xent_reference(x, y, g, drop_last_tail=None):
    """Plain fp32: lse, loss, and dx with lse = 0 handed in.  drop_last_tail: (tail0 per row) -> the mutant whose log-sum-exp
    misses column cols - 1 of every row that has a tail."""
    x = x.float()
    cols = x.shape[1]
    seen = x.clone()
    if drop_last_tail is not None:
        seen[drop_last_tail < cols, cols - 1] = -float('inf')
    lse = torch.logsumexp(seen, 1)
    inside = (y >= 0) & (y < cols)
    loss = torch.where(inside, lse - x[torch.arange(x.shape[0]), y.clamp(0, cols - 1)], torch.zeros_like(lse))
    hit = torch.zeros_like(x)
    hit[torch.arange(x.shape[0])[inside], y[inside]] = 1
    return lse, loss, g[:, None] * (torch.exp(x) - hit)


def _vector_path_takes_the_head(dx, nhead, tail0):
    """Mutant: the vector stores start one element early, over the head's last element."""
    out = dx.clone()
    for r in range(dx.shape[0]):
        h, t = int(nhead[r]), int(tail0[r])
        if h >= 1 and t > h:
            out[r, h - 1:t - 1] = dx[r, h:t]
    return out


@pytest.mark.parametrize('dtype', R.XENT_DTYPES, ids=['bf16', 'fp16', 'fp32'])
@pytest.mark.parametrize('cols', R.XENT_SMALL + R.XENT_BIG)
def test_cross_entropy(cols, dtype):
    eb = 4 if dtype == torch.float32 else 2
    tail_mutant_seen = False
    for stride in (cols, R.odd_above(cols)):
        for offset in ((0, 1) if cols in R.XENT_SMALL else (0,)):
            rows = cols if cols in R.XENT_SMALL else R.XENT_BIG_ROWS
            addr = (offset + torch.arange(rows) * stride) * eb                  # behind a 16-byte boundary
            nhead, tail0 = R.xent_split(addr, cols, dtype)
            j = R.xent_small_needles(cols) if cols in R.XENT_SMALL else R.xent_big_needles(cols, nhead, tail0)
            assert j.min() >= 0 and j.max() < cols
            if cols in R.XENT_BIG:
                assert {0, cols - 1, 2047, 2049, 49151, 49153} <= set(j.tolist())
                if stride % 2:
                    assert set(nhead[:8].tolist()) == set(range(16 // eb))          # one row per phase and kind
                    assert (j[16:24] == nhead[16:24] - 1).sum() >= 16 // eb - 1 and (j[40:48] == tail0[40:48].clamp(max=cols - 1)).all()
            if offset and cols < 16 // eb:
                assert (nhead == cols).any()                                    # the whole row is head
            y, g = R.xent_labels(j, cols), R.xent_grads(rows)
            x = torch.empty(rows, cols, dtype=torch.float64)
            R.xent_fill(x, j)
            _representable(x, dtype, 'logits')
            want_dx = R.xent_want_dx(j, y, g, cols)
            _representable(want_dx, dtype, 'dx')
            lse, loss, dx = _xent_reference(x, y, g)
            assert R.xent_fwd_failures(loss, lse, j, y, cols, 'ref') == []
            assert R.exact_failures(dx.to(dtype), want_dx, dtype, 'dx') == []
            if ((tail0 < cols) & (j == cols - 1)).any() and cols > 1:        # a row whose needle is its last tail element
                lse, loss, _ = _xent_reference(x, y, g, drop_last_tail=tail0)
                assert R.xent_fwd_failures(loss, lse, j, y, cols, 'mutant')
                tail_mutant_seen = True
            if ((nhead >= 1) & (tail0 > nhead)).any() and cols in R.XENT_SMALL:
                assert R.exact_failures(_vector_path_takes_the_head(dx, nhead, tail0).to(dtype), want_dx, dtype, 'dx')
    assert tail_mutant_seen or cols == 1


def test_cross_entropy_smoothing_bounds():
    """The bounds the GPU test applies: 4x the error of the fp32 evaluation of the kernel's formulas (printed; -s shows)."""
    _, bounds = R.smooth_bounds()
    print('smoothing bounds (lse, loss, dx):', ' '.join(f'{b:.3e}' for b in bounds))
    assert all(0 < b < 1e-4 for b in bounds)


# ---- 4. add + LayerNorm forward ----------------------------------------------------------------------------------------------

def _ln_fwd_cases():
    for cols in R.LN_FWD_CH:
        yield cols, R.ln_spike_columns(cols)
    for cols, rows in R.LN_FWD_FEW_ROWS.items():
        yield cols, R.ln_spike_columns(cols, rows)


def test_layer_norm_forward():
    worst = 0.0
    for cols, js in _ln_fwd_cases():
        assert R.ln_ch(cols) == R.LN_FWD_CH[cols]
        if cols > 1540 and js.numel() > 5:
            assert {0, 255, 256, cols - 1} <= set(js.tolist())
        for residual in (False, True):
            prob = R.ln_fwd_problem(cols, js, residual)
            for dtype in DTYPES:
                for k in ('x0', 'gamma', 'beta'):
                    _representable(prob[k], dtype, k)
            assert prob['x'].abs().sum(1).max() < 2 ** 24
            want, scale = R.ln_fwd_closed_form(prob)
            assert torch.allclose(want, R.ln_fwd_eval(prob, torch.float64), rtol=1e-12, atol=1e-12)   # the closed form IS LayerNorm
            z = R.ln_fwd_eval(prob)
            worst = max(worst, float(((z.double() - want).abs() / scale).max()))
            assert R.ln_fwd_failures(z, prob, torch.float32, f'{cols}') == []
            for dtype in DTYPES:
                assert R.ln_fwd_failures(z.to(dtype), prob, dtype, f'{cols} {dtype}') == []
            some = R.ln_fwd_problem(cols, js[::8] if js.numel() > 64 else js, residual)     # every eighth spike column
            want, scale = R.ln_fwd_closed_form(some)
            for mean_w, var_w in ((0.0, 1.0), (1.0, 0.0), (2.0, 2.0)):
                err = (R.ln_fwd_eval(some, mean_weight=mean_w, var_weight=var_w).double() - want).abs() / scale
                least = float(err.max(1).values.min())           # every ROW of every width
                assert least >= R.LN_FWD_MUTANT_FACTOR * R.LN_FWD_F32_BOUND, (cols, residual, mean_w, var_w, least)
    print(f'LayerNorm forward: worst fp32 evaluation error {worst:.3e} scales; bound {R.LN_FWD_F32_BOUND:.3e}')
    assert 4 * worst <= R.LN_FWD_F32_BOUND <= 8 * worst
    with pytest.raises(StopIteration):
        R.ln_ch(8196)


# ---- 5. add + LayerNorm backward ---------------------------------------------------------------------------------------------

def test_layer_norm_backward():
    cap = 1024
    assert 'BP_LN_BWD_WS_ROWS %d' % cap in open(os.path.join(os.path.dirname(CSRC), '..', 'include', 'bp_hip.h')).read()
    worst = {}
    seen = set()
    for cols, rows, dx_in, dx1, colscale in R.ln_bwd_cases():
        assert R.ln_ch(cols, R.LN_BWD_CH_LIST) in R.LN_BWD_CH_LIST
        assert R.ln_bwd_trips(rows, cap) == R.LN_BWD_TRIPS[rows]
        n_wg = R.ln_bwd_nwg(rows, cap)
        prob = R.ln_bwd_problem(rows, cols, 'cpu', colscale)
        for dtype in DTYPES:
            for k in ('dz', 'x', 'dx_in', 'x0', 'gamma') + (('cs',) if colscale else ()):
                _representable(prob[k], dtype, k)
        assert prob['dz'].abs().sum(0).max() < 2 ** 24
        ref = R.ln_bwd_eval(prob, torch.float64, n_wg, dx_in)
        got = R.ln_bwd_eval(prob, torch.float32, n_wg, dx_in)
        assert R.ln_bwd_exact_failures(got, prob, dx_in, torch.float32, 'fp32') == []
        assert R.ln_bwd_bound_failures(got, ref, 'fp32') == []
        for k, v in R.ln_bwd_ratios(got, ref).items():
            worst[k] = max(worst.get(k, 0.0), v)
        for dtype in DTYPES:                                     # 16-bit weights: dbeta rounded once
            assert R.exact_failures(got['dbeta'].to(dtype), prob['dz'].sum(0), dtype, 'dbeta') == []
        if R.LN_BWD_TRIPS[rows][1] >= 2:
            for weight in (0, 2):
                mutant = R.ln_bwd_eval(prob, torch.float32, n_wg, dx_in, {1: weight})
                assert any('dbeta' in b for b in R.ln_bwd_exact_failures(mutant, prob, dx_in, torch.float32, 'm'))
                bad = R.ln_bwd_bound_failures(mutant, ref, 'm')
                assert any('dgamma' in b for b in bad) and (not colscale or any('dcolscale' in b for b in bad))
        seen.add((rows > 4096, dx_in, dx1, colscale))
    assert len(seen) == 16                                       # every option on and off, below and beyond the first trip
    print('LayerNorm backward: worst fp32 evaluation error in scales:', {k: f'{v:.3e}' for k, v in worst.items()})
    for k, v in worst.items():
        assert 4 * v <= R.LN_BWD_BOUND[k] <= 8 * v, (k, v)


# ---- 6. causal softmax backward ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('s', list(R.SOFTMAX_CASES))
def test_softmax_backward(s):
    assert R.softmax_ch(s) == R.SOFTMAX_CASES[s]
    with pytest.raises(StopIteration):
        R.softmax_ch(4104)
    n = R.softmax_matrices(s)
    prob = R.softmax_problem(s, n, 'cpu')
    alpha, da = prob['alpha'], prob['da']
    assert torch.equal(alpha.sum(-1), torch.ones(n, s, dtype=torch.float64))
    assert (torch.triu(alpha[0], 1) == 0).all() and (torch.triu(da[0], 1) == R.SOFTMAX_POISON)[torch.triu(torch.ones(s, s), 1) > 0].all()
    for dtype in DTYPES:
        _representable(alpha, dtype, 'alpha')
        _representable(torch.tril(da), dtype, 'dA')             # 777 above the diagonal is poison: any value
    a32, d32 = alpha.float(), da.float()
    below = torch.tril(torch.ones(s, s, dtype=torch.bool))

    def evaluate(skip_last_live=False):
        prod = a32 * torch.where(below, d32, torch.zeros(()))
        if skip_last_live:
            last = (alpha[0] > 0).sum(-1) - 1                      # last column with probability mass
            prod[:, torch.arange(s), last] = 0
        acc = prod.sum(-1, keepdim=True)
        return torch.where(below, torch.tensor(R.SOFTMAX_SCALE) * a32 * (d32 - acc), torch.zeros(()))

    out = evaluate()
    assert torch.equal(out.double(), prob['want'])               # exact in fp32
    for dtype in DTYPES:
        assert R.exact_failures(out.to(dtype), prob['want'], dtype, 'dS') == []
        assert R.exact_failures(evaluate(True).to(dtype), prob['want'], dtype, 'dS')
