"""GPU: WHICH rows and columns the row-wise kernels (csrc/add_layer_norm.hip, bias_gelu.hip, xentropy.hip, softmax_bwd.hip) own,
checked exactly -- what tests/test_gpu_prefill_needles.py does for the attention kernels.  The 2x parity tests
(tests/test_gpu_fused_ops.py and the module-level ones) cannot see one row dropped from a column sum of a few thousand random
rows, or one logit dropped from a 50257-wide log-sum-exp; here either changes bits.

Inputs, expected results and criteria: tests/rowwise_exact.py; tests/test_rowwise_exact_host.py proves on the CPU that a plain
fp32 evaluation meets every criterion on every case below and that named mutants of it do not.  Every call goes through the C
ABI (bp_hip.lib()), so that every output and workspace is a view inside a NaN-filled buffer whose guard rows and gap columns
must keep their bits.

  column sums, dGELU   dpre, dbias and bp_column_sum == the fp64 value rounded once, bit for bit; the trips of the U-unrolled
                       main loop and of its tail are computed from the slice count the library reports
  bias + GELU fwd      y and pre bit for bit; 4100 x 4096 gives some threads a second grid-stride trip
  cross-entropy        |lse| <= 2^-20, loss within 2^-20 of 0 / 128, exactly 0 for a label out of range; dx bit for bit, gap
                       columns untouched; head 0..7 (0..3 in fp32) by odd row strides and a base one element off; the backward
                       out of place, in place, and with a gradient stride of the other parity (the element-wise path)
  add + LayerNorm fwd  residual out bit for bit; 16-bit z within one ulp of the rounded closed form; fp32 z within
                       LN_FWD_F32_BOUND; every CH of the launcher, cols = 8196 refused
  add + LayerNorm bwd  dbeta == sum of dz exactly through all grid-stride trips and the workspace fold; rows with dz = 0 pass
                       dx_in through bit for bit; dgamma, dcolscale, dx within LN_BWD_BOUND in the all-fp32 mode
  softmax backward     bit for bit, zero above the diagonal, CH = 1, 2, 4, 8; S = 4104 and 12 refused

Measured bounds (not derived), all against an fp32 evaluation of the same formulas on the CPU, 4x its own worst error versus
fp64 (tests/rowwise_exact.py), and what the MI355X reached (the tests print it, -s):
  LayerNorm forward, fp32 z     bound 4.5e-6 scales (evaluation 1.12e-6)       kernel 1.23e-6 (cols = 6144)
  LayerNorm backward, dx        bound 3.15e-6 scales (evaluation 7.75e-7)      kernel 7.86e-7 (4096 x 2048)
                      dgamma    bound 1.03e-6 (2.54e-7)                        kernel 2.99e-7 (2 x 2048)
                      dcolscale bound 8.2e-7 (1.89e-7)                         kernel 2.56e-7 (5 x 2048)
  smoothing s = 0.1             lse 3.7e-6, loss 5.8e-6, dx 8.0e-7 absolute    kernel 9.9e-7, 1.9e-6, 2.0e-7
The LayerNorm forward's evaluation follows the kernel's summation order (rowwise_exact.wave_row_sum): the lane that holds the
spike's square absorbs the small squares it adds afterwards, which costs the row's rstd a relative 1e-6 in the kernel and in
the evaluation alike; against torch.sum (2.3e-7) the first version of the bound, 9.2e-7, failed at cols = 6144 for that reason.
v_rcp_f32 at 1 and 2, v_exp_f32 at 0 and beyond both ends of its range and v_log_f32 at 1 are exact on the MI355X: every GELU
and cross-entropy case holds bit for bit, no fallback bound was needed.

The issue's table lists (691, 12288) as "some waves take a main-loop trip of the U = 4 loop, others only the tail"; with the 43
slices the library reports every wave takes one trip there.  The shape stays, with what it does asserted, and (603, 12288) is
the shape that has both kinds of wave.

Mutation run (single-line mutants, arithmetic only -- no address, bound or launch shape changed; built as two variant libraries
with one mutant per kernel each and run once against this file; number = failing cases of 214):

  #  mutant                                                                           killed here by
  1  bias_gelu.hip: the U-unrolled main loop adds its row u = 2 twice                 12: column sums, every shape with a
                                                                                          main-loop trip
  2  add_layer_norm.hip, backward: db not accumulated when row >= n_wg * 4            26: every case of 4097 rows and more
  3  xentropy.hip, forward: the first tail element is left out of the sum of exp      30: every width, vocabulary rows, smoothing
  4  add_layer_norm.hip, forward: CH = 6 skips c = 5 in the variance                  5: cols = 1536, all five modes (at 1028 and
                                                                                          1280 chunk 5 holds no column)
  5  softmax_bwd.hip: acc skips c = 7                                                 2: S = 4096 (at 2056 chunk 7 is never live)
  6  xentropy.hip, backward: the element-wise pass misses the label when x and dx     24: the gradient stride of the other parity,
     differ in phase                                                                      every width but 1 (one row: same phase)
  7  bias_gelu.hip, forward: 0 instead of GELU on the second grid-stride trip         2: 4100 x 4096
  8  add_layer_norm.hip, backward: dg not accumulated when row >= n_wg * 8            10: 8195 and 12291 rows (dgamma, fp32 mode)
  9  bias_gelu.hip, colsum_finish_kernel: partial row 5 skipped                       12: column sums with more than 5 slices
"""
import ctypes

import pytest
import torch

import rowwise_exact as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
F32 = torch.float32
DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ['bf16', 'fp16']


def _lib():
    import bp_hip
    return bp_hip.lib()


def _call(name, *args):
    rc = getattr(_lib(), name)(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:                                  # a GPU fault: nothing more may run on this device
        pytest.exit(f'{name}: {err}', returncode=3)
    return rc


def _ok(bad, tag):
    assert not bad, f'{tag}: ' + '; '.join(bad)


def _ids(shape):
    return 'x'.join(map(str, shape))


# ---- 1. column sums and the GELU backward ------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', list(R.COLSUM_CASES), ids=_ids)
def test_column_sums_and_gelu_backward(shape, dtype):
    """bp_column_sum (U = 8) and bp_bias_gelu_bwd (U = 4) with fp32 and 16-bit dbias, then in place and with dbias == NULL."""
    rows, cols = shape
    ws_floats = _lib().bp_bias_grad_ws_floats(rows, cols)
    slices = ws_floats // cols
    assert ws_floats == slices * cols
    for u, want in R.COLSUM_CASES[shape].items():                # the trips this shape claims, from the library's slice count
        assert R.trip_summary(rows, slices, u) == want, (u, R.trip_summary(rows, slices, u))
        if shape in R.COLSUM_MAIN_AND_TAIL[u]:
            assert want[1] >= 1 and want[3] >= 1                 # at least one main-loop trip and one tail trip
    prob = R.colsum_problem(rows, cols, DEV)
    g, pre, code = prob['g'].to(dtype), prob['pre'].to(dtype), R.DTYPE_CODE[dtype]
    bad = []
    for out in (F32, dtype):
        tag = f'dbias {out}'
        dbias, ws = R.Guarded(1, cols, out, DEV), R.Guarded(slices, cols, F32, DEV)
        assert _call('bp_column_sum', g.data_ptr(), dbias.ptr(), ws.ptr(), rows, cols, code, int(out == F32)) == 0
        bad += R.exact_failures(dbias.view[0], prob['colsum'], out, f'column sum, {tag}') + dbias.failures(tag) + ws.failures('ws')
        dpre, dbias, ws = R.Guarded(rows, cols, dtype, DEV), R.Guarded(1, cols, out, DEV), R.Guarded(slices, cols, F32, DEV)
        assert _call('bp_bias_gelu_bwd', g.data_ptr(), pre.data_ptr(), dpre.ptr(), dbias.ptr(), ws.ptr(), rows, cols, code,
                     int(out == F32)) == 0
        bad += (R.exact_failures(dpre.view, prob['dpre'], dtype, f'dpre, {tag}') + R.exact_failures(dbias.view[0], prob['dbias'], out, tag)
                + dpre.failures('dpre') + dbias.failures(tag) + ws.failures('ws'))
    inplace, dbias, ws = R.guarded_like(prob['g'], dtype), R.Guarded(1, cols, F32, DEV), R.Guarded(slices, cols, F32, DEV)
    assert _call('bp_bias_gelu_bwd', inplace.ptr(), pre.data_ptr(), inplace.ptr(), dbias.ptr(), ws.ptr(), rows, cols, code, 1) == 0
    bad += (R.exact_failures(inplace.view, prob['dpre'], dtype, 'dpre in place') + R.exact_failures(dbias.view[0], prob['dbias'], F32, 'dbias in place')
            + inplace.failures('in place') + dbias.failures('dbias in place') + ws.failures('ws in place'))
    dpre, ws = R.Guarded(rows, cols, dtype, DEV), R.Guarded(slices, cols, F32, DEV)
    assert _call('bp_bias_gelu_bwd', g.data_ptr(), pre.data_ptr(), dpre.ptr(), None, ws.ptr(), rows, cols, code, 1) == 0
    bad += R.exact_failures(dpre.view, prob['dpre'], dtype, 'dpre without dbias') + dpre.failures('dpre without dbias') + ws.failures('ws')
    assert torch.isnan(ws.view).all(), 'dbias == NULL: the workspace was written'
    _ok(bad, f'{shape} {dtype}')


# ---- 2. bias + GELU forward --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', R.GELU_FWD_CASES, ids=_ids)
def test_bias_gelu_forward(shape, dtype):
    rows, cols = shape
    if shape == R.GELU_FWD_CASES[-1]:
        assert R.gelu_fwd_trips(rows, cols) == (1, 2)           # some threads take a second grid-stride trip
    code = R.DTYPE_CODE[dtype]
    bad = []
    for variant in R.GELU_FWD_VARIANTS:
        prob = R.gelu_fwd_problem(rows, cols, DEV, 'nobias' not in variant)
        bias = prob['bias'].to(dtype) if prob['bias'] is not None else None
        x = R.guarded_like(prob['x'], dtype)
        y = x if 'inplace' in variant else R.Guarded(rows, cols, dtype, DEV)
        pre = R.Guarded(rows, cols, dtype, DEV) if 'pre' in variant else None
        assert _call('bp_bias_gelu_fwd', x.ptr(), bias.data_ptr() if bias is not None else None,
                     pre.ptr() if pre is not None else None, y.ptr(), rows, cols, code) == 0
        bad += R.exact_failures(y.view, prob['y'], dtype, f'{variant}: y') + y.failures(f'{variant}: y') + x.failures(f'{variant}: x')
        if pre is not None:
            bad += R.exact_failures(pre.view, prob['pre'], dtype, f'{variant}: pre') + pre.failures(f'{variant}: pre')
        if 'inplace' not in variant:
            bad += R.exact_failures(x.view, prob['x'], dtype, f'{variant}: x was written')
    _ok(bad, f'{shape} {dtype}')


# ---- 3. cross-entropy --------------------------------------------------------------------------------------------------------

def _xent_case(cols, dtype, stride, offset, rows, want_dx_of, chain_lse=False):
    """Forward, then the three backward variants, on needle rows laid out with `stride` and `offset`."""
    code, tag = R.DTYPE_CODE[dtype], f'cols={cols} stride={stride} offset={offset}'
    logits = R.Guarded(rows, cols, dtype, DEV, stride, offset)
    nhead, tail0 = R.xent_split(R.row_addresses(logits.view), cols, dtype)
    j = R.xent_small_needles(cols) if cols in R.XENT_SMALL else R.xent_big_needles(cols, nhead, tail0)
    y, g = R.xent_labels(j, cols), R.xent_grads(rows)
    R.xent_fill(logits.view, j)
    labels, grads = y.to(DEV), g.to(DEV)
    losses, lse = R.Guarded(1, rows, F32, DEV), R.Guarded(1, rows, F32, DEV)
    assert _call('bp_xentropy_fwd', logits.ptr(), labels.data_ptr(), losses.ptr(), lse.ptr(), rows, cols, stride, 0.0, -1, code) == 0
    bad = (R.xent_fwd_failures(losses.view[0], lse.view[0], j, y, cols, f'{tag} fwd') + losses.failures('losses') + lse.failures('lse')
           + logits.failures('logits'))
    want = want_dx_of(j, y, g)
    lse0 = lse.view[0].contiguous() if chain_lse else torch.zeros(rows, device=DEV)
    x_addr = R.row_addresses(logits.view)
    for variant in ('out', 'other parity', 'in place'):
        if variant == 'in place':
            dx = logits
        else:
            dx = R.Guarded(rows, cols, dtype, DEV, stride + (variant == 'other parity'), offset)
        same_phase = ((x_addr ^ R.row_addresses(dx.view)) & 15) == 0
        assert same_phase.all() if variant != 'other parity' else (rows == 1 or not same_phase.all()), variant
        assert _call('bp_xentropy_bwd', grads.data_ptr(), logits.ptr(), lse0.data_ptr(), labels.data_ptr(), dx.ptr(), rows, cols,
                     stride, dx.view.stride(0), 0.0, -1, code) == 0
        if chain_lse:                                            # lse as the forward left it: exact where that is exactly 0
            tol = (g.double() * 2.0 ** -19)[:, None].to(DEV)
            bad += R.listing(~((dx.view.double() - want).abs() <= tol), f'{tag} {variant} (forward lse): dx')
        else:
            bad += R.exact_failures(dx.view, want, dtype, f'{tag} {variant}: dx')
        bad += dx.failures(f'{tag} {variant}: dx')
    return bad, nhead, tail0, j


@pytest.mark.parametrize('dtype', R.XENT_DTYPES, ids=DTYPE_IDS + ['fp32'])
@pytest.mark.parametrize('cols', R.XENT_SMALL)
def test_cross_entropy_every_column_is_a_needle(cols, dtype):
    """rows = cols; row stride cols and the odd value above it; base aligned and one element off (cols < head happens)."""
    want = {}

    def want_dx_of(j, y, g):
        if not want:
            want['dx'] = R.xent_want_dx(j, y, g, cols).to(DEV)
        return want['dx']

    bad, heads = [], set()
    for stride in (cols, R.odd_above(cols)):
        for offset in (0, 1):
            more, nhead, _, _ = _xent_case(cols, dtype, stride, offset, cols, want_dx_of, chain_lse=(stride == cols and offset == 0))
            bad += more
            heads |= set(nhead.tolist())
    per16 = 4 if dtype == F32 else 8
    assert heads >= set(range(min(per16, cols)))             # every head length the width allows
    if cols < per16:
        assert cols in heads                                     # a row that is all head
    _ok(bad, f'{cols} {dtype}')


@pytest.mark.parametrize('dtype', R.XENT_DTYPES, ids=DTYPE_IDS + ['fp32'])
@pytest.mark.parametrize('cols', R.XENT_BIG)
def test_cross_entropy_vocabulary_rows(cols, dtype):
    """Needles at the first and last column, at both ends of the head and of the tail (one row per 16-byte phase), at columns
    256 * 8 * k +- 1 and at 64 drawn columns."""
    bad = []
    for stride in (cols, R.odd_above(cols)):
        more, nhead, tail0, j = _xent_case(cols, dtype, stride, 0, R.XENT_BIG_ROWS, lambda j, y, g: R.xent_want_dx(j, y, g, cols).to(DEV))
        bad += more
        assert {0, cols - 1, 2047, 2049, 49151, 49153} <= set(j.tolist())
        if stride % 2:
            assert set(nhead[:8].tolist()) == set(range(4 if dtype == F32 else 8))
        assert (tail0 < cols).any() or cols % 8 == 0
    _ok(bad, f'{cols} {dtype}')


@pytest.mark.parametrize('dtype', R.XENT_DTYPES, ids=DTYPE_IDS + ['fp32'])
def test_cross_entropy_smoothing(dtype):
    """s = 0.1, 64 x 4099 logits k / 8: lse, loss and dx against fp64 within 4x the error of the fp32 evaluation of the same
    formulas on the CPU (rowwise_exact.smooth_bounds: lse 3.7e-6, loss 5.8e-6, dx 8.0e-7 here); dx in a 16-bit dtype adds its
    one rounding.  Measured on the MI355X: lse 9.9e-7, loss 1.9e-6, dx 2.0e-7 (fp32 logits)."""
    c, code = R.XENT_SMOOTH, R.DTYPE_CODE[dtype]
    x, y, g = R.smooth_problem()
    (ref_lse, ref_loss, ref_dx), (b_lse, b_loss, b_dx) = R.smooth_bounds()
    logits, labels, grads = x.to(dtype).to(DEV), y.to(DEV), g.to(DEV)
    losses, lse = R.Guarded(1, c['rows'], F32, DEV), R.Guarded(1, c['rows'], F32, DEV)
    dx = R.Guarded(c['rows'], c['cols'], dtype, DEV)
    assert _call('bp_xentropy_fwd', logits.data_ptr(), labels.data_ptr(), losses.ptr(), lse.ptr(), c['rows'], c['cols'], c['cols'],
                 c['s'], -1, code) == 0
    lse_in = lse.view[0].contiguous()
    assert _call('bp_xentropy_bwd', grads.data_ptr(), logits.data_ptr(), lse_in.data_ptr(), labels.data_ptr(), dx.ptr(), c['rows'],
                 c['cols'], c['cols'], c['cols'], c['s'], -1, code) == 0
    e_lse = (lse.view[0].double().cpu() - ref_lse).abs()
    e_loss = (losses.view[0].double().cpu() - ref_loss).abs()
    e_dx = (dx.view.double().cpu() - ref_dx).abs()
    allowed_dx = b_dx + (R.ROUNDING[dtype] * ref_dx.abs() if dtype != F32 else 0.0)
    print(f'smoothing {dtype}: lse {e_lse.max():.3e} (bound {b_lse:.3e}), loss {e_loss.max():.3e} (bound {b_loss:.3e}), '
          f'dx - rounding {(e_dx - allowed_dx + b_dx).max():.3e} (bound {b_dx:.3e})')
    _ok(R.listing(~(e_lse <= b_lse), 'lse') + R.listing(~(e_loss <= b_loss), 'loss') + R.listing(~(e_dx <= allowed_dx), 'dx')
        + losses.failures('losses') + lse.failures('lse') + dx.failures('dx'), f'smoothing {dtype}')


# ---- 4. add + LayerNorm forward ----------------------------------------------------------------------------------------------

LN_FWD_PARAMS = [(cols, None) for cols in R.LN_FWD_CH] + list(R.LN_FWD_FEW_ROWS.items())


def _ln_fwd(cols, js, mode, dtype, worst):
    x0_f32, res, x_out, w_f32 = R.LN_FWD_MODES[mode]
    prob = R.ln_fwd_problem(cols, js, res is not None)
    rows = js.numel()
    in_dtype = F32 if x0_f32 else dtype
    res_dtype = F32 if (res == 'f32' or (res is None and x0_f32)) else dtype
    w_dtype = F32 if w_f32 else dtype
    x0 = prob['x0'].to(in_dtype).to(DEV)
    x1 = prob['x1'].to(res_dtype).to(DEV) if res is not None else None
    gamma, beta = prob['gamma'].to(w_dtype).to(DEV), prob['beta'].to(w_dtype).to(DEV)
    z = R.Guarded(rows, cols, in_dtype, DEV)
    xo = R.Guarded(rows, cols, res_dtype, DEV) if x_out else None
    rc = _call('bp_dropout_add_layer_norm', x0.data_ptr(), x1.data_ptr() if x1 is not None else None, gamma.data_ptr(),
               beta.data_ptr(), z.ptr(), xo.ptr() if xo is not None else None, None, rows, cols, R.EPS, R.DTYPE_CODE[dtype],
               int(x0_f32), int(res_dtype == F32), int(res_dtype == F32), int(w_f32), 0.0, None)
    tag = f'cols={cols} rows={rows} {mode} {dtype}'
    assert rc == 0, tag
    bad = R.ln_fwd_failures(z.view, prob, in_dtype, tag) + z.failures(f'{tag}: z')
    if xo is not None:
        bad += R.exact_failures(xo.view, prob['x'].to(DEV), res_dtype, f'{tag}: residual out') + xo.failures(f'{tag}: residual out')
    if in_dtype == F32:
        want, scale = R.ln_fwd_closed_form(prob)
        worst.append(float(((z.view.double().cpu() - want).abs() / scale).max()))
    return bad


@pytest.mark.parametrize('mode', list(R.LN_FWD_MODES))
@pytest.mark.parametrize('cols,few', LN_FWD_PARAMS, ids=[f'{c}' if f is None else f'{c}x{f}' for c, f in LN_FWD_PARAMS])
def test_add_layer_norm_forward_spikes(cols, few, mode):
    """One spike per row (rowwise_exact.ln_spike_columns); CH as the issue's table says, from the launcher's own list."""
    assert R.ln_ch(cols) == R.LN_FWD_CH[cols]
    js = R.ln_spike_columns(cols, few)
    bad, worst = [], []
    for dtype in (DTYPES if not R.LN_FWD_MODES[mode][0] else DTYPES[:1]):
        bad += _ln_fwd(cols, js, mode, dtype, worst)
    if worst:
        print(f'LayerNorm forward cols={cols} {mode}: fp32 z off by {max(worst):.3e} scales (bound {R.LN_FWD_F32_BOUND:.3e})')
    _ok(bad, f'{cols} {mode}')


def test_add_layer_norm_forward_refuses_8196_columns():
    cols = 8196
    x0 = torch.ones(2, cols, device=DEV, dtype=torch.bfloat16)
    w = torch.ones(cols, device=DEV)
    z = R.Guarded(2, cols, torch.bfloat16, DEV)
    rc = _call('bp_dropout_add_layer_norm', x0.data_ptr(), None, w.data_ptr(), w.data_ptr(), z.ptr(), None, None, 2, cols, R.EPS, 1,
               0, 0, 0, 1, 0.0, None)
    assert rc != 0 and torch.isnan(z.view).all() and not z.failures('z')
    import bp_hip
    with pytest.raises(RuntimeError):
        bp_hip.add_layer_norm(x0, None, w, w, R.EPS)


# ---- 5. add + LayerNorm backward ---------------------------------------------------------------------------------------------

def _ln_bwd(prob, rows, cols, dx_in, dx1, mode, cap):
    """mode: ('f32',) all-fp32, or (16-bit dtype, residual fp32?, weights fp32?).  Returns the outputs and the guard failures."""
    if mode[0] == 'f32':
        dz_dtype = res_dtype = w_dtype = F32
        code = 1
    else:
        dz_dtype, res_dtype, w_dtype = mode[0], F32 if mode[1] else mode[0], F32 if mode[2] else mode[0]
        code = R.DTYPE_CODE[mode[0]]
    cs = prob['cs']
    dz, x, gamma = prob['dz'].to(dz_dtype), prob['x'].to(res_dtype), prob['gamma'].to(w_dtype)
    din = prob['dx_in'].to(res_dtype) if dx_in else None
    x0 = prob['x0'].to(dz_dtype) if cs is not None else None
    csw = cs.to(w_dtype) if cs is not None else None
    ws_floats = _lib().bp_ln_bwd_ws_floats(cols, int(cs is not None))
    assert ws_floats == (3 if cs is not None else 2) * cap * cols
    out = {'dx0': R.Guarded(rows, cols, dz_dtype, DEV), 'dx1': R.Guarded(rows, cols, res_dtype, DEV) if dx1 else None,
           'dgamma': R.Guarded(1, cols, w_dtype, DEV), 'dbeta': R.Guarded(1, cols, w_dtype, DEV),
           'dcolscale': R.Guarded(1, cols, w_dtype, DEV) if cs is not None else None, 'ws': R.Guarded(1, ws_floats, F32, DEV)}
    ptr = lambda t: t.data_ptr() if t is not None else None
    gptr = lambda t: t.ptr() if t is not None else None
    rc = _call('bp_dropout_add_layer_norm_scaled_bwd', dz.data_ptr(), ptr(din), x.data_ptr(), ptr(x0), gamma.data_ptr(), None,
               ptr(csw), out['dx0'].ptr(), gptr(out['dx1']), out['dgamma'].ptr(), out['dbeta'].ptr(), gptr(out['dcolscale']),
               out['ws'].ptr(), ws_floats, rows, cols, R.EPS, code, int(dz_dtype == F32), int(res_dtype == F32),
               int(w_dtype == F32), 0.0, None)
    assert rc == 0, (rows, cols, mode)
    bad = []
    for k, v in out.items():
        if v is not None:
            bad += v.failures(f'{mode}: {k}')
    got = {k: (v.view if k in ('dx0', 'dx1') else v.view[0]) if v is not None else None for k, v in out.items() if k != 'ws'}
    return got, bad, w_dtype


LN_BWD_PARAMS = R.ln_bwd_cases()


@pytest.mark.parametrize('case', LN_BWD_PARAMS, ids=[f'{c[1]}x{c[0]}' + ''.join(n for n, on in zip('irc', c[2:]) if on) for c in LN_BWD_PARAMS])
def test_add_layer_norm_backward_rows_and_trips(case):
    """(cols, rows, dx_in, dx1, colscale): all-fp32 mode against fp64 within LN_BWD_BOUND plus the exact criteria, then a 16-bit
    mode (dtype, residual dtype and weight dtype rotate) under the exact criteria alone."""
    cols, rows, dx_in, dx1, colscale = case
    cap = _lib().bp_ln_bwd_ws_floats(cols, 0) // (2 * cols)     # BP_LN_BWD_WS_ROWS, as the library reports it
    trips = R.ln_bwd_trips(rows, cap)
    assert trips == R.LN_BWD_TRIPS[rows]                         # e.g. 8195: some wave takes 2 trips and some 3
    n_wg = R.ln_bwd_nwg(rows, cap)
    prob = R.ln_bwd_problem(rows, cols, DEV, colscale)
    got, bad, _ = _ln_bwd(prob, rows, cols, dx_in, dx1, ('f32',), cap)
    ref = R.ln_bwd_eval(prob, torch.float64, n_wg, dx_in)
    bad += R.ln_bwd_exact_failures(got, prob, dx_in, F32, 'fp32') + R.ln_bwd_bound_failures(got, ref, 'fp32')
    print(f'LayerNorm backward {rows}x{cols}: off by (scales)', {k: f'{v:.2e}' for k, v in R.ln_bwd_ratios(got, ref).items()},
          'bounds', R.LN_BWD_BOUND)
    k = LN_BWD_PARAMS.index(case)
    mode = (DTYPES[k % 2], (k // 2) % 2 == 0, (k // 4) % 2 == 0)
    got, more, w_dtype = _ln_bwd(prob, rows, cols, dx_in, dx1, mode, cap)
    bad += more + R.ln_bwd_exact_failures(got, prob, dx_in, w_dtype, f'{mode}')
    _ok(bad, f'{case}')


# ---- 6. causal softmax backward ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('s', list(R.SOFTMAX_CASES))
def test_softmax_backward_is_exact(s, dtype):
    assert R.softmax_ch(s) == R.SOFTMAX_CASES[s]
    n = R.softmax_matrices(s)
    prob = R.softmax_problem(s, n, DEV)
    alpha = prob['alpha'].to(dtype)
    da = R.guarded_like(prob['da'].view(n * s, s), dtype)
    assert _call('bp_softmax_bwd_causal', alpha.data_ptr(), da.ptr(), n, s, R.SOFTMAX_SCALE, R.DTYPE_CODE[dtype]) == 0
    _ok(R.exact_failures(da.view.view(n, s, s), prob['want'], dtype, 'dS') + da.failures('dS')
        + R.listing(torch.triu(da.view.view(n, s, s), 1) != 0, 'above the diagonal'), f'S={s} {dtype}')


@pytest.mark.parametrize('s', R.SOFTMAX_REFUSED)
def test_softmax_backward_refuses(s):
    alpha = torch.zeros(s, s, device=DEV, dtype=torch.bfloat16)
    da = R.Guarded(s, s, torch.bfloat16, DEV)
    assert _call('bp_softmax_bwd_causal', alpha.data_ptr(), da.ptr(), 1, s, R.SOFTMAX_SCALE, 1) != 0
    assert torch.isnan(da.view).all() and not da.failures('dS')
