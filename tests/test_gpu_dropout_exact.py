"""GPU: the dropout mask of every kernel that draws one, and the arithmetic of the DROP bodies, checked exactly -- what
tests/test_gpu_prefill_needles.py does for key visibility.  tests/test_gpu_dropout.py holds the three attention mask
computations that are not the probability dump to "<= 2x / 4x the eager error, max-abs over the tensor", the rule that stops
seeing one wrong key a few hundred keys in; here one wrong mask bit, at any row, changes a zero into a non-zero or back.

Inputs, expected results and criteria: tests/dropout_exact.py; tests/test_dropout_exact_host.py proves on the CPU that plain
fp32 / fp64 references meet the criteria on every case below and that eight mutants of them do not.  The dropout state is
always given explicitly, (0x1234567, 99) or (-0x1234567890ABCDEF, (7 << 32) + 12345) -- the second has an offset >= 2^32, a
counter word that was zero in every earlier test -- and the expected mask comes from tests/philox_ref.py.

  read-outs    one mask bit per output entry through a one-hot operand, the four attention uses of the mask (forward, dV,
               dQ, dK), p = 0.17, 0.5, 0.9, 1e-6, both states, causal / sq != sk / ragged: exactly 0 where dropped or hidden,
               non-zero elsewhere and within 4 roundings of the fp64 value
  probs        attn_probs: sign bits == the restatement, magnitudes == the undropped dump, both dtypes, sq != sk, both states
  pairs        two tied needles per row at p = 1/2: O, dQ, dK, dV == the closed forms with the keep bits, bit for bit (flash_fwd;
               flash_bwd from the closed-form O and LSE; chained; sq != sk; ragged)
  LayerNorm    dmask == the restatement on all rows, widths 252 ... 8192; at p = 1/2 the residual is exactly 2 x0 where kept
               (also with power-of-two rowscale / colscale); dx0 == 0 where dropped and == (2 dx1).to(dtype) where kept

Outputs hold NaN before a call and the rows behind the call stay NaN.

No kernel had to change: all 126 cases pass on the library as it stood.

Mutation run (single-line mutants, arithmetic only -- no address, loop bound, launch or synchronisation changes --, each built as
a variant library outside the tree and run once against this file, 126 cases, and once against tests/test_gpu_dropout.py, 644
cases; number = failing cases):

  #  mutant                                                                       here                            old file
  1  flash_fwd_dma.hip: key tiles >= 2 take the keep bits of col0 + 4             27: fwd read-outs, pair fwd,    72 (qkvpacked)
                                                                                      the chain
  2  flash_bwd.hip, dQ: the edge body takes kbase of the previous tile for the    32: dq read-outs, every pair    102 (qkvpacked)
     mask                                                                             backward
  3  bp_philox.h: dropout_keep_collane reads halfword j ^ 1                       46: dv and dk read-outs, every  120 (qkvpacked)
                                                                                      pair backward
  4  flash_bwd.hip, dK/dV: de = pv * z * (dp + dneg)                              18: every pair backward (the    118 (qkvpacked)
                                                                                      read-outs have D = 0)
  5  add_layer_norm.hip, backward: the last 256-column chunk takes (col >> 2) + 1 12: every LayerNorm backward    256 (LayerNorm
                                                                                                                      training)
  6  flash_fwd_dma.hip: key tiles >= 3, second half, register 5 takes register    22: fwd read-outs from S = 257  47 (qkvpacked,
     4's keep bit                                                                     on, pair fwd, the chain         S = 256, 512)
  7  flash_bwd.hip, dQ: the same one bit per row and key tile                     26                              43 (S = 256, 512)
  8  flash_bwd.hip, dK/dV: query tiles >= 3, second sub-block, register 5 takes   30                              48 (S = 256, 512)
     register 4's keep bit

Eight of eight are killed here -- and the old file lets none of them through either: its oracle is handed the restated mask, and
on its random data (S <= 512, scores of order 1) one wrong mask bit moves an entry by 0.26 where 4x the eager error is 0.01.  So
the gap this file closes is not a mutant of this list; it is what the old file never launches or never compares: the DROP
kernels with sq != sk, a ragged batch with an empty sequence, attention at p = 0.5, 0.9 and 1e-6 (the clamped threshold), fp16
through the probability dump, the LayerNorm mask on rows >= 64 and at widths > 768 -- and every result as bits, not as a ratio
of errors.
"""
import pytest
import torch

import dropout_exact as X
import prefill_needles as P
import rowwise_exact as W

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ['bf16', 'fp16']
NAN = float('nan')
TAIL = 16


def _bp():
    import bp_hip
    return bp_hip


def _ok(bad, tag):
    assert not bad, f'{tag}: ' + '; '.join(bad)


def _rng(state):
    return X.state_tensor(state, DEV)


def _behind(x, dtype, poison, whole):
    """x (n, ...) as the head of a buffer with TAIL more rows of `poison`; `whole`: hand the buffer itself to the call (a
    cu_seqlens call, which takes the row count from cu_seqlens), else the view of the n rows -> (buffer, argument)."""
    buf = torch.full((x.shape[0] + TAIL,) + tuple(x.shape[1:]), poison, device=DEV, dtype=dtype)
    buf[:x.shape[0]] = x.to(DEV, dtype)
    return buf, (buf if whole else buf[:x.shape[0]])


def _untouched(bufs, rows, tag):
    for buf in bufs:
        assert torch.isnan(buf[rows:]).all(), f'{tag}: rows behind the call were written'


# ---- A. read-outs -------------------------------------------------------------------------------------------------------------

_PROBLEMS = {}


def _readout_problem(case, kind):
    """Built once on the CPU (fp64 probabilities) and shared by the dtypes, the states and the values of p."""
    key = (X.case_id(case), kind)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = X.readout_problem(case, kind)
    return _PROBLEMS[key]


def _readout(bp, prob, dtype, state, p, tag):
    kind, ragged = prob['kind'], prob['ragged']
    cu = prob['cu'].to(DEV) if ragged else None
    tq, tk = prob['q'].shape[0], prob['k'].shape[0]
    (_, q), (_, k), (_, v), (_, dout) = (_behind(prob[x], dtype, 8.0, ragged) for x in ('q', 'k', 'v', 'dout'))
    if kind == 'fwd':
        buf, out = _behind(torch.full_like(prob['q'], NAN), dtype, NAN, ragged)
        lse = bp.flash_fwd(q, k, v, out, cu, cu, prob['max_q'], prob['max_k'], prob['scale'], prob['causal'], p, _rng(state))
        got, rows, bufs = buf[:tq], tq, [buf]
        for n, s in enumerate(prob['seqs']):
            if s is not None:
                _ok(P.lse_failures(lse[n, :, :s['lq']].cpu(), s['lse']), f'{tag} LSE of sequence {n}')
    else:
        zeros = torch.zeros(q.shape, device=DEV, dtype=dtype)
        (bq, dq), (bk, dk), (bv, dv) = (_behind(torch.full_like(prob[x], NAN), dtype, NAN, ragged) for x in ('q', 'k', 'v'))
        bp.flash_bwd(dout, q, k, v, zeros, X.readout_lse(prob, DEV), dq, dk, dv, cu, cu, prob['max_q'], prob['max_k'],
                     prob['scale'], prob['causal'], p, _rng(state))
        got = {'dv': bv[:tk], 'dq': bq[:tq], 'dk': bk[:tk]}[kind]
        _untouched([bq], tq, tag)
        _untouched([bk, bv], tk, tag)
        assert not torch.isnan(torch.cat([bq[:tq].flatten(), bk[:tk].flatten(), bv[:tk].flatten()])).any(), f'{tag}: NaN in a gradient'
        rows, bufs = 0, []
    _untouched(bufs, rows, tag)
    _ok(X.readout_failures(got.cpu(), X.readout_want(prob, state, p), dtype, kind), tag)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('kind', X.KINDS)
@pytest.mark.parametrize('case', X.READ_CASES, ids=[X.case_id(c) for c in X.READ_CASES])
def test_mask_read_out_bit_by_bit(case, kind, dtype):
    """fwd: flash_fwd with V one-hot over slot n's window of keys reads the forward's mask; dv / dk: flash_bwd with dO / Q
    one-hot over a window of rows read the dK/dV kernel's lane = key mask; dq: K one-hot over a window of keys reads the dQ
    kernel's.  Every p and both states; the ragged batch takes stream sequence * h + head, rows and columns relative to the
    sequence."""
    bp = _bp()
    prob = _readout_problem(case, kind)
    for p in X.P_VALUES:
        for state in X.STATES:
            _readout(bp, prob, dtype, state, p, f'{X.case_id(case)} {kind} p={p} offset={state[1]} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', list(X.probs_shapes()), ids=lambda s: 'x'.join(map(str, s)))
def test_probability_dump_signs_are_the_mask(shape, dtype):
    """bp.attn_probs at the read-out shapes: sign bits == the restatement on every visible pair, magnitudes == the undropped
    dump, for every p and both states (p = 1e-6: the few dropped pairs of the whole matrix are all seen here)."""
    bp = _bp()
    b, h, sq, sk, d, causal = shape
    q, k = (x.to(DEV, dtype) for x in X.probs_operands(b, h, sq, sk, d))
    s = d ** -0.5 * torch.einsum('bthd,bshd->bhts', q.double(), k.double())
    visible = torch.ones(sq, sk, dtype=torch.bool, device=DEV)
    if causal:
        visible = visible.tril()
        s = s.masked_fill(~visible, float('-inf'))
    lse = torch.full((b, h, -(-sq // 16) * 16), NAN, device=DEV)
    lse[:, :, :sq] = torch.logsumexp(s, -1).float()
    plain = bp.attn_probs(q, k, lse, d ** -0.5, causal)
    assert (plain[..., visible] > 0).all() and (plain[..., ~visible] == 0).all()
    for p in X.P_VALUES:
        for state in X.STATES:
            probs = bp.attn_probs(q, k, lse, d ** -0.5, causal, p, _rng(state))
            want = X.keep_mask(state, b * h, sq, sk, p).view(b, h, sq, sk).to(DEV)
            got = ~torch.signbit(probs.float())
            tag = f'{shape} p={p} offset={state[1]} {dtype}'
            assert torch.equal(got[..., visible], want[..., visible]), f'{tag}: sign bits differ from the restatement'
            assert torch.equal(probs.abs(), plain), f'{tag}: magnitudes differ from the undropped dump'


# ---- B. pair problems under p = 1/2 -------------------------------------------------------------------------------------------

def _exact_in(dtype, *tensors):
    for t in tensors:
        assert torch.equal(t.to(dtype).double(), t.double()), f'expected result not representable in {dtype}'


def _rows_lse_in(lse):
    b, g, s = lse.shape
    buf = torch.full((b, g, -(-s // 16) * 16), NAN, device=DEV)
    buf[:, :, :s] = lse.float()
    return buf


def _pair_fwd(bp, prob, dtype, causal, state, tag):
    b, sq, h, d = prob['q'].shape
    sk = prob['k'].shape[1]
    q, k, v = (prob[x].to(dtype).reshape(-1, h, d) for x in ('q', 'k', 'v'))
    buf, out = _behind(torch.full_like(q, NAN), dtype, NAN, False)
    lse = bp.flash_fwd(q, k, v, out, None, None, sq, sk, prob['scale'], causal, X.PAIR_P, _rng(state))
    _exact_in(dtype, prob['want'])
    _ok(P.exact_failures(out.view(b, sq, h, d), prob['want'], dtype, 'out', prob['zero_out']) + P.lse_failures(lse[:, :, :sq], prob['lse']),
        tag + ' (forward)')
    _untouched([buf], q.shape[0], tag)
    return out, lse


def _pair_bwd(bp, prob, dtype, causal, state, tag, chain=False):
    b, sq, h, d = prob['q'].shape
    sk = prob['k'].shape[1]
    q, k, v, dout = (prob[x].to(dtype).reshape(-1, h, d) for x in ('q', 'k', 'v', 'dout'))
    if chain:
        out, lse = _pair_fwd(bp, prob, dtype, causal, state, tag)
    else:
        out, lse = prob['want'].to(dtype).reshape(-1, h, d), _rows_lse_in(prob['lse'])
    (bq, dq), (bk, dk), (bv, dv) = (_behind(torch.full_like(x, NAN), dtype, NAN, False) for x in (q, k, v))
    bp.flash_bwd(dout, q, k, v, out, lse, dq, dk, dv, None, None, sq, sk, prob['scale'], causal, X.PAIR_P, _rng(state))
    _exact_in(dtype, prob['want_dq'], prob['want_dk'], prob['want_dv'])
    _ok(P.exact_failures(dq.view(b, sq, h, d), prob['want_dq'], dtype, 'dq', prob['zero_dq'])
        + P.exact_failures(dk.view(b, sk, h, d), prob['want_dk'], dtype, 'dk', prob['zero_dk'])
        + P.exact_failures(dv.view(b, sk, h, d), prob['want_dv'], dtype, 'dv'), tag)
    _untouched([bq], q.shape[0], tag)
    _untouched([bk, bv], k.shape[0], tag)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', P.PAIR_BWD_CASES, ids=[f"d{c['d']}" for c in P.PAIR_BWD_CASES])
def test_pair_flash_fwd_under_dropout_is_its_closed_form(case, dtype):
    """flash_fwd with p = 1/2 on the fixed-length pair cases: out == k1 V[j1] + k2 V[j2] (2 k V[j1] for a row without a
    partner) bit for bit -- the row sum runs over the unrounded, undropped P -- and the LSE is the one without dropout."""
    bp = _bp()
    for tag, prob in X.pair_fixed_problems(dtype, DEV, cases=[case]):
        _pair_fwd(bp, prob, dtype, True, X.PAIR_STATE['fixed'], f'{tag} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', P.PAIR_BWD_CASES, ids=[f"d{c['d']}" for c in P.PAIR_BWD_CASES])
def test_pair_flash_bwd_under_dropout_is_its_closed_form(case, dtype):
    """flash_bwd with p = 1/2, the closed-form O and per-row LSE handed in: D = k1 dP1 + k2 dP2, dS1 = k1 dP1 - D / 2, dS2 =
    k2 dP2 - D / 2, dQ = scale (dS1 K[j1] + dS2 K[j2]), dK = scale sum dS Q_i, dV = sum k dO_i, bit for bit where not 0; where
    0, the bounds of the pair tests without dropout.  bf16 without dropout_exact.PAIR_BF16_LEFT_OUT."""
    bp = _bp()
    for tag, prob in X.pair_fixed_problems(dtype, DEV, cases=[case]):
        _pair_bwd(bp, prob, dtype, True, X.PAIR_STATE['fixed'], f'{tag} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_pair_flash_bwd_under_dropout_chained_to_the_forward(dtype):
    """O and LSE as the dropout forward returns them, then the same exact gradients from the same state."""
    c = P.PAIR_CHAIN
    for tag, prob in X.pair_fixed_problems(dtype, DEV, cases=[dict(d=c['d'], seqlens=[c['s']])]):
        _pair_bwd(_bp(), prob, dtype, True, X.PAIR_STATE['chain'], f'chained {tag} {dtype}', chain=True)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_pair_flash_bwd_under_dropout_cross_lengths(dtype):
    """Not causal, sq = 150, sk = 333, the second state."""
    for tag, prob in X.pair_cross_problems(dtype, DEV):
        _pair_bwd(_bp(), prob, dtype, False, X.PAIR_STATE['cross'], f'{tag} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_pair_flash_bwd_under_dropout_ragged_batch(dtype):
    """The ragged batch with its empty sequence, the second state: stream sequence * h + head, mask rows and columns relative
    to the sequence; LSE entries behind each sequence are NaN, rows behind the batch poison in every input and NaN in every
    output."""
    bp = _bp()
    c = P.FLASH_BWD_RAGGED
    for tag, prob in X.pair_ragged_problems(dtype, DEV):
        total, top = prob['q'].shape[0], max(c['lens'])
        (_, q), (_, k), (_, v), (_, dout), (_, out) = (_behind(prob[x], dtype, 8.0, True) for x in ('q', 'k', 'v', 'dout', 'want'))
        lse = torch.full((len(c['lens']), c['h'], -(-top // 16) * 16), NAN, device=DEV)
        for n, length in enumerate(c['lens']):
            if length:
                lse[n, :, :length] = prob['lse'][n].float()
        dq, dk, dv = torch.full_like(q, NAN), torch.full_like(k, NAN), torch.full_like(v, NAN)
        bp.flash_bwd(dout, q, k, v, out, lse, dq, dk, dv, prob['cu'], prob['cu'], top, top, prob['scale'], True, X.PAIR_P,
                     _rng(X.PAIR_STATE['ragged']))
        _exact_in(dtype, prob['want_dq'], prob['want_dk'], prob['want_dv'])
        _ok(P.exact_failures(dq[:total], prob['want_dq'], dtype, 'dq', prob['zero_dq'])
            + P.exact_failures(dk[:total], prob['want_dk'], dtype, 'dk', prob['zero_dk'])
            + P.exact_failures(dv[:total], prob['want_dv'], dtype, 'dv'), f'{tag} {dtype}')
        _untouched([dq, dk, dv], total, tag)


# ---- C. LayerNorm ---------------------------------------------------------------------------------------------------------------

EPS = 1e-5


def _ln_weights(cols):
    gamma, beta = (x.float().to(DEV) for x in W.ln_weights(cols))
    return gamma, beta


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('cols', X.LN_FWD_COLS)
def test_layer_norm_forward_mask_and_residual(cols, dtype):
    """add_layer_norm with dropout, integer x0, no x1, an fp32 residual: dmask == rows_keep_mask on ALL rows (70 and 257), both
    states, p = 1/2 and 0.17; at p = 1/2 the residual is exactly 2 x0 where kept and 0 where dropped, also with power-of-two
    rowscale and colscale."""
    bp = _bp()
    gamma, beta = _ln_weights(cols)
    for rows in X.LN_ROWS:
        x0 = X.ln_x0(rows, cols, DEV)
        rs, cs = X.ln_scales(rows, cols, DEV)
        for state in X.STATES:
            for p in X.LN_P:
                keep = X.ln_keep(state, rows, cols, p).to(DEV)
                for scaled in (False, True):
                    tag = f'rows={rows} cols={cols} p={p} offset={state[1]} scaled={scaled} {dtype}'
                    z, xo, dmask = bp.add_layer_norm(x0.to(dtype), None, gamma, beta, EPS, residual_dtype=torch.float32, dropout_p=p,
                                                     rng_state=_rng(state), return_dropout_mask=True,
                                                     rowscale=rs.to(dtype) if scaled else None, colscale=cs if scaled else None)
                    assert torch.equal(dmask.bool(), keep) and int(dmask.max()) <= 1, f'{tag}: dmask differs from the restatement'
                    assert torch.isfinite(z.float()).all(), tag
                    if p == 0.5:
                        want = 2 * x0 * keep
                        if scaled:
                            want = want * rs[:, None] * cs
                        assert torch.equal(xo, want), f'{tag}: residual is not 2 x0 where kept, 0 where dropped'
                    else:
                        assert torch.equal(xo == 0, ~keep), f'{tag}: zero pattern of the residual'


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('cols', X.LN_BWD_COLS)
def test_layer_norm_backward_passes_the_forward_mask(cols, dtype):
    """add_layer_norm_bwd with the forward's state and want_dx1, an fp32 stream: dx0 is exactly 0 where dropped; where kept, at
    p = 1/2, dx0 == (2 dx1).to(dtype) bit for bit (the mask enters only the product dx * drop_scale); at p = 0.17 within one
    rounding of dx1 / (1 - p) (2 u allowed: the rounding, and the fp32 scale)."""
    bp = _bp()
    assert bp.add_layer_norm_bwd_supported(dtype, cols)
    gamma, beta = _ln_weights(cols)
    for rows in X.LN_ROWS:
        x0 = X.ln_x0(rows, cols, DEV)
        dz = X.ln_dz(rows, cols, DEV).to(dtype)
        dx_in = X.ln_dz(rows, cols, DEV).flip(0).contiguous() / 4
        for state in X.STATES:
            for p in X.LN_P:
                tag = f'rows={rows} cols={cols} p={p} offset={state[1]} {dtype}'
                keep = X.ln_keep(state, rows, cols, p).to(DEV)
                _, xo = bp.add_layer_norm(x0.to(dtype), None, gamma, beta, EPS, residual_dtype=torch.float32, dropout_p=p,
                                          rng_state=_rng(state))
                dx0, dx1, _, _ = bp.add_layer_norm_bwd(dz, dx_in, xo, gamma, EPS, True, p, _rng(state))
                assert dx1.dtype == torch.float32 and torch.isfinite(dx1).all(), tag
                assert (dx0[~keep] == 0).all(), f'{tag}: dx0 is not 0 where the forward dropped'
                if p == 0.5:
                    assert torch.equal(dx0[keep], (2 * dx1).to(dtype)[keep]), f'{tag}: dx0 != (2 dx1).to(dtype) where kept'
                else:
                    want = dx1.double() / (1 - p)
                    off = (dx0.double() - want).abs()[keep]
                    assert (off <= 2 * X.ROUNDING[dtype] * (want.abs()[keep] + X.SMALLEST_NORMAL[dtype])).all(), f'{tag}: dx0 off where kept'
