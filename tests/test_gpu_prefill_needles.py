"""GPU: WHICH keys the prefill forward (csrc/flash_fwd*.hip, attn_probs.hip, sense_mix*.hip, sense_wide*.hip) and the
backward (csrc/flash_bwd.hip, sense_mix_bwd.hip) let a row see, checked exactly -- what tests/test_gpu_decode_edges.py
section A does for the decode kernels.  The whole-tensor 2x rule of the parity tests is set by the early rows and notices a
key lost by late rows only while the error stays above it (a few hundred keys in); here a dropped, duplicated or
misattributed key changes bits at any row.

Inputs, expected results and criteria: tests/prefill_needles.py; tests/test_prefill_needles_host.py proves on the CPU that
the fp32 / fp64 references meet the criteria on every case below and that three mutants of them do not.

  forward      out == V[j*] (sum over senses: sum_l C[j*_l]) bit for bit, LSE within the decode tolerance
  probs        exactly 1.0 at the needle, exactly 0 where masked, <= 2e-21 elsewhere; the LSE is handed in (needle score)
  dV, dC       == the sum of the dO rows whose needle the key is, bit for bit; <= 1e-12 for a key that is nobody's needle
  dQ, dK       <= 1e-6 (out = V[j*] and lse = needle score handed in; once both taken from bp.flash_fwd)
  dqk          within prefill_needles.dqk_bounds (below)

Outputs the caller allocates hold NaN before the call; what a call must not read is poisoned: rows past cu_seqlens and
LSE entries past a sequence (NaN / magnitude 8), the odd rows of the gather table, the columns behind a narrower view.

NOT tested here: the non-zero arithmetic of dQ, dK and dqk (the 2x tests of tests/test_gpu_backward.py keep that job),
dropout, and a row taking another row's LSE (every row of a call has the same LSE; another row's D is seen).

Two places where the kernels' own arithmetic is not exact on these inputs, each with a derived bound instead:
  * flash_fwd_dma.hip:282-285 and 484: the LSE is the logarithm of the sum of ROUNDED p.  In the stale-reference case that
    sum is one bf16 number, e^18 rounded: prefill_needles.STALE_LSE_TOL adds half a bf16 ulp to the decode tolerance.  The
    output bits are exact all the same (the same rounded p normalises and multiplies V).
  * sense_mix_bwd.hip:380-386, 416-420, 463-466: dq = scale (A1 - (D - r) A2) rounds g_n = P_n (dP_n - r) to 16 bit for
    A1 but not inside D, and the rebuilt P_n is 1 - e with e ~ 1e-5 (fl(scale log2e) * width and fl(lse log2e) round
    apart).  What that leaves is bounded in prefill_needles.dqk_bounds, an fp64 model the host test checks; a row with
    another row's D is 4 (bf16) or 32 (fp16) times that bound away per unit of D.

Mutation run (single-line mutants, arithmetic only, each built as a variant library and run once against this file; number =
failing cases of 103):

  #  mutant                                                                         killed here by
  1  flash_fwd_dma.hip: wave 2 skips key tile 3 when the pass has >= 6 key tiles    22: flash fwd (S = 385, 641), the mixes
                                                                                        with S >= 641 through their LSE pre-pass
  2  flash_fwd_dma.hip: l_run takes key tile 2's row sum twice (fast entry)         34: flash fwd from S = 129 on, ragged, mixes
                                                                                        (LSE), the chained backward
  3  flash_bwd.hip, dK/dV: query tile 3, sub-block 1, register 5 has P = 0          14: dV of the fixed, chained and ragged cases
  4  flash_bwd.hip, dQ: a row takes the D of its neighbouring lane                  18: dQ bound, every backward case
  5  mix_ring.h, mix_x_block: register 11 of the second half has P = 0              16: the ring mixes, gather, dC
  6  sense_mix_bwd.hip, dq: a row takes D - r of its neighbouring lane              6: every sense_dqk case
  7  flash_fwd_dma.hip: l_run takes a KEPT steady-state tile's row sum twice         1 of the 23 forward cases: the stale-reference
                                                                                        one (elsewhere a kept tile weighs 1e-21)
"""
import pytest
import torch

import prefill_needles as P

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ['bf16', 'fp16']
NAN = float('nan')


def _bp():
    import bp_hip
    return bp_hip


def _ok(bad, tag):
    assert not bad, f'{tag}: ' + '; '.join(bad)


def _exact_in(dtype, *tensors):
    for t in tensors:
        assert torch.equal(t.to(dtype).double(), t.double()), f'expected result not representable in {dtype}'


def _lse_in(value, b, g, s):
    """The hand-built (b, g, roundup(s, 16)) LSE: the needle score in the rows of the call, NaN behind them."""
    lse = torch.full((b, g, -(-s // 16) * 16), NAN, device=DEV)
    lse[:, :, :s] = value
    return lse


# ---- flash forward ---------------------------------------------------------------------------------------------------------

def _flash_fwd(bp, prob, dtype, causal, tag, lse_tol=P.LSE_TOL):
    b, sq, h, d = prob['q'].shape
    sk = prob['k'].shape[1]
    q, k, v = (prob[x].to(dtype).reshape(-1, h, d) for x in ('q', 'k', 'v'))
    out = torch.full_like(q, NAN)
    lse = bp.flash_fwd(q, k, v, out, None, None, sq, sk, prob['scale'], causal)
    _exact_in(dtype, prob['want'])
    _ok(P.flash_failures(out.view(b, sq, h, d), lse[:, :, :sq], prob, dtype, lse_tol), tag)
    return out, lse


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', P.FLASH_FWD_CASES, ids=[f"d{c['d']}" for c in P.FLASH_FWD_CASES])
def test_flash_fwd_rows_are_their_needles(case, dtype):
    """Causal, fixed length, three (sample, head) slots with a map each, every map of FWD_MAPS in three calls: S = 129 ...
    256 is the paired pass of two query tiles, 257 ... 384 leaves the middle tile unpaired, from 257 on the 2-slot ring
    wraps twice; d = 36 takes the register-staged kernel."""
    bp = _bp()
    for s in case['seqlens']:
        b, h = P.bh_of(s)
        for rot in P.rotations(P.FWD_MAPS, 3):
            prob = P.attn_problem(P.slot_maps(P.FWD_MAPS, 3, rot), b, h, s, s, case['d'], DEV)
            _flash_fwd(bp, prob, dtype, True, f"d={case['d']} S={s} maps from {rot} {dtype}")


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_flash_fwd_nine_pairs(dtype):
    """b * h = 9: the (sample, head) -> XCD mapping with a count that is no multiple of 8."""
    c = P.FLASH_BH9
    prob = P.attn_problem(P.slot_maps(P.FWD_MAPS, 9, 0), c['b'], c['h'], c['s'], c['s'], c['d'], DEV)
    _flash_fwd(_bp(), prob, dtype, True, f'nine pairs {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('causal', [False, True])
def test_flash_fwd_cross_lengths(causal, dtype):
    """sq = 150, sk = 333; not causal: also needles behind the row (mirror, last)."""
    c = P.FLASH_CROSS
    maps = P.FWD_MAPS if causal else P.CROSS_MAPS + P.FWD_MAPS
    for rot in P.rotations(maps, 3):
        prob = P.attn_problem(P.slot_maps(maps, 3, rot), c['b'], c['h'], c['sq'], c['sk'], c['d'], DEV)
        _flash_fwd(_bp(), prob, dtype, causal, f'cross causal={causal} maps from {rot} {dtype}')


def _ragged_buffers(prob, dtype, names, pad=64):
    """(total + pad, h, d) buffers of a ragged problem, the rows behind cu_seqlens[-1] poisoned with magnitude 8."""
    total = prob['q'].shape[0]
    bufs = []
    for n, x in enumerate(names):
        buf = torch.full((total + pad,) + tuple(prob[x].shape[1:]), 8.0 * (-1) ** n, device=DEV, dtype=dtype)
        buf[:total] = prob[x].to(dtype)
        bufs.append(buf)
    return bufs


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_flash_fwd_ragged_batch(dtype):
    """cu_seqlens with sequences that start inside a tile ([70, 1, 130, 257, 5]): a key of the neighbouring sequence has
    the same position code and another value id; the rows behind the batch are poison and their outputs stay NaN."""
    bp = _bp()
    c = P.FLASH_RAGGED
    for rot in P.rotations(P.FWD_MAPS, c['h']):
        prob = P.ragged_problem(c['lens'], c['h'], c['d'], P.FWD_MAPS, rot, DEV)
        total = prob['q'].shape[0]
        q, k, v = _ragged_buffers(prob, dtype, ('q', 'k', 'v'))
        out = torch.full_like(q, NAN)
        lse = bp.flash_fwd(q, k, v, out, prob['cu'], prob['cu'], max(c['lens']), max(c['lens']), prob['scale'], True)
        _ok(P.flash_failures(out[:total], None, prob, dtype), f'ragged maps from {rot} {dtype}')
        assert torch.isnan(out[total:]).all(), 'rows behind cu_seqlens[-1] were written'
        for n, length in enumerate(c['lens']):
            torch.testing.assert_close(lse[n, :, :length], torch.full_like(lse[n, :, :length], prob['lse']), **P.LSE_TOL)


def test_flash_fwd_stale_reference_body():
    """softmax_scale = 9 / reps, bf16, S = 641: rows >= 128 meet their needle in key tile 1, e^18 ~ 2^26 above the reference
    their first tile set -- under the 2^30 limit, so the steady-state body of csrc/flash_fwd_dma.hip keeps the stale reference
    (with the default scale every late needle is e^48 above it and takes the retry, the other body).  LSE: STALE_LSE_TOL."""
    c = P.FLASH_STALE
    prob = P.attn_problem([P.STALE_MAP] * 3, c['b'], c['h'], c['s'], c['s'], c['d'], DEV, scale_num=c['scale_num'])
    _flash_fwd(_bp(), prob, torch.bfloat16, True, 'stale reference', P.STALE_LSE_TOL)


# ---- probabilities ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('d', P.PROBS_D)
def test_attn_probs_from_a_given_lse(d, causal, dtype):
    """bp.attn_probs on its own: sk = 64 and 200 store 16 bytes, 204 eight, 333 single elements (p_vec16 / p_vec of
    bp_attn_probs_dropout); square and sq = 150."""
    bp = _bp()
    maps = P.FWD_MAPS if causal else P.CROSS_MAPS + P.FWD_MAPS
    for sk in P.PROBS_SK:
        for sq in (sk, P.PROBS_CROSS_SQ):
            prob = P.attn_problem(P.slot_maps(maps, 3, sk + sq), 1, 3, sq, sk, d, DEV, cols=8)
            p = bp.attn_probs(prob['q'].to(dtype), prob['k'].to(dtype), _lse_in(prob['lse'], 1, 3, sq), prob['scale'], causal)
            _ok(P.probs_failures(p, prob['js'], causal, f'd={d} sq={sq} sk={sk} causal={causal} {dtype}'), 'attn_probs')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', P.ALPHA_CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_sense_alpha_from_a_given_lse(shape, dtype):
    s, k, dk = shape
    prob = P.sense_problem(s, k, dk, 8, device=DEV)
    alpha = _bp().sense_alpha(prob['qk'].to(dtype), prob['scale'], lse=_lse_in(prob['lse'], 2, k, s))
    _ok(P.probs_failures(alpha, prob['js'], True, f'{shape} {dtype}'), 'sense_alpha')


# ---- sense LSE and mix -------------------------------------------------------------------------------------------------------

def _behind_a_view(x, dtype, extra=8, offset=0, poison=8.0):
    """x as a view of a buffer with `extra` more columns (poison), starting at column `offset`."""
    buf = torch.full(tuple(x.shape[:-1]) + (x.shape[-1] + extra,), poison, device=DEV, dtype=dtype)
    view = buf[..., offset:offset + x.shape[-1]]
    view.copy_(x)
    return buf, view


def _mix(bp, prob, dtype, tag, offset=0, gather=False):
    b, s, _, k, _ = prob['qk'].shape
    _, qk = _behind_a_view(prob['qk'], dtype)
    lse = bp.sense_lse(qk, prob['scale'])
    torch.testing.assert_close(lse[:, :, :s], torch.full_like(lse[:, :, :s], prob['lse']), **P.LSE_TOL)
    out_buf, out = _behind_a_view(torch.full_like(prob['want'], NAN), dtype, poison=NAN)
    if gather:
        table = prob['table'].to(dtype)
        table[1::2] = -8.0
        bp.sense_mix_gather(qk, table, prob['rows'], prob['scale'], out=out, lse=lse)
    else:
        _, content = _behind_a_view(prob['content'], dtype, offset=offset)
        bp.sense_mix(qk, content, prob['scale'], out=out, lse=lse, key_weight=prob['key_weight'])
    _exact_in(dtype, prob['want'])
    _ok(P.flash_failures(out, None, prob, dtype), tag)
    assert torch.isnan(out_buf[..., out.shape[-1]:]).all(), f'{tag}: columns behind the output view were written'


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', P.MIX_NARROW + P.MIX_WIDE, ids=lambda s: 'x'.join(map(str, s)))
def test_sense_mix_rows_are_the_sums_of_their_needles(shape, dtype):
    """Every sense has a map of its own (FWD_MAPS rotated by sense and sample).  qk, content and out are views of buffers
    eight columns wider (poison behind them; d_k = 10: the zero-padded width); the narrow shapes take the LDS-DMA ring, the
    wide ones (d_k = 160, 640) theirs, S = 333 the staged wide kernel."""
    _mix(_bp(), P.sense_problem(*shape, device=DEV), dtype, f'{shape} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_sense_mix_staged_route(dtype):
    """Content viewed at a 2-byte offset (as test_operands_as_awkward_views): the register-staged csrc/sense_mix.hip."""
    _mix(_bp(), P.sense_problem(*P.MIX_STAGED, device=DEV), dtype, f'staged {dtype}', offset=1)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', P.MIX_GATHER, ids=lambda s: 'x'.join(map(str, s)))
def test_sense_mix_gather_rows_are_the_sums_of_their_needles(shape, dtype):
    """Content rows through a 1024-row table whose odd rows (never named) hold -8."""
    _mix(_bp(), P.sense_problem(*shape, device=DEV, form='gather'), dtype, f'gather {shape} {dtype}', gather=True)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_sense_mix_key_weights(dtype):
    """key_weight in {0.5, 1, 2}, a hash of (sample, sense, key): out = sum_l w[l, j*_l] C[j*_l, l], still exact."""
    _mix(_bp(), P.sense_problem(*P.MIX_WEIGHTED, device=DEV, weighted=True), dtype, f'weighted {dtype}')


# ---- flash backward ------------------------------------------------------------------------------------------------------------

def _flash_bwd(bp, prob, dtype, causal, tag, chain=False):
    b, sq, h, d = prob['q'].shape
    sk = prob['k'].shape[1]
    q, k, v, dout = (prob[x].to(dtype).reshape(-1, h, d) for x in ('q', 'k', 'v', 'dout'))
    if chain:
        out = torch.full_like(q, NAN)
        lse = bp.flash_fwd(q, k, v, out, None, None, sq, sk, prob['scale'], causal)
    else:
        out, lse = prob['want'].to(dtype).reshape(-1, h, d), _lse_in(prob['lse'], b, h, sq)
    dq, dk, dv = torch.full_like(q, NAN), torch.full_like(k, NAN), torch.full_like(v, NAN)
    bp.flash_bwd(dout, q, k, v, out, lse, dq, dk, dv, None, None, sq, sk, prob['scale'], causal)
    _exact_in(dtype, prob['want_dv'])
    _ok(P.grad_failures(dv.view(b, sk, h, d), prob['want_dv'], prob['fan'], dtype, 'dv')
        + P.dust_failures(dq, P.GRAD_DUST, 'dq') + P.dust_failures(dk, P.GRAD_DUST, 'dk'), tag)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', P.FLASH_BWD_CASES, ids=[f"d{c['d']}" for c in P.FLASH_BWD_CASES])
def test_flash_bwd_dv_is_the_sum_of_its_rows(case, dtype):
    """Causal, fixed length, out = V[j*] and lse = the needle score handed in (NaN behind the rows), dO in {1, 2}: dV bit
    for bit, dQ and dK dust.  d = 64 and 128 are the FULLD instantiations."""
    bp = _bp()
    for s in case['seqlens']:
        b, h = P.bh_of(s)
        for rot in P.rotations(P.BWD_MAPS, 3):
            prob = P.attn_problem(P.slot_maps(P.BWD_MAPS, 3, rot), b, h, s, s, case['d'], DEV)
            _flash_bwd(bp, prob, dtype, True, f"d={case['d']} S={s} maps from {rot} {dtype}")


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_flash_bwd_chained_to_the_forward(dtype):
    """out and lse as bp.flash_fwd returns them."""
    prob = P.attn_problem(P.slot_maps(P.BWD_MAPS, 3, 0), 1, 3, 385, 385, 64, DEV)
    _flash_bwd(_bp(), prob, dtype, True, f'chained {dtype}', chain=True)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_flash_bwd_cross_lengths(dtype):
    """Not causal, sq = 150, sk = 333 (most keys are nobody's needle)."""
    c = P.FLASH_CROSS
    maps = P.CROSS_MAPS + P.BWD_MAPS
    for rot in P.rotations(maps, 3):
        prob = P.attn_problem(P.slot_maps(maps, 3, rot), c['b'], c['h'], c['sq'], c['sk'], c['d'], DEV)
        _flash_bwd(_bp(), prob, dtype, False, f'cross maps from {rot} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_flash_bwd_ragged_batch(dtype):
    """The ragged batch with a zero-length sequence; LSE entries behind each sequence are NaN, rows behind the batch poison
    in every input and NaN (unwritten) in every output."""
    bp = _bp()
    c = P.FLASH_BWD_RAGGED
    for rot in P.rotations(P.BWD_MAPS, c['h']):
        prob = P.ragged_problem(c['lens'], c['h'], c['d'], P.BWD_MAPS, rot, DEV)
        total, top = prob['q'].shape[0], max(c['lens'])
        q, k, v, dout, out = _ragged_buffers(prob, dtype, ('q', 'k', 'v', 'dout', 'want'))
        lse = _lse_in(NAN, len(c['lens']), c['h'], top)
        for n, length in enumerate(c['lens']):
            lse[n, :, :length] = prob['lse']
        dq, dk, dv = torch.full_like(q, NAN), torch.full_like(k, NAN), torch.full_like(v, NAN)
        bp.flash_bwd(dout, q, k, v, out, lse, dq, dk, dv, prob['cu'], prob['cu'], top, top, prob['scale'], True)
        _exact_in(dtype, prob['want_dv'])
        _ok(P.grad_failures(dv[:total], prob['want_dv'], prob['fan'], dtype, 'dv')
            + P.dust_failures(dq[:total], P.GRAD_DUST, 'dq') + P.dust_failures(dk[:total], P.GRAD_DUST, 'dk'),
            f'ragged maps from {rot} {dtype}')
        for g in (dq, dk, dv):
            assert torch.isnan(g[total:]).all(), 'rows behind cu_seqlens[-1] were written'


# ---- sense backward ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', P.MIX_DC, ids=lambda s: 'x'.join(map(str, s)))
def test_sense_mix_dc_is_the_sum_of_its_rows(shape, dtype):
    """dC[s, l, :] = sum of dout[t, :] over {t : j*_l(t) = s}, dense dout in {1, 2}, lse = the needle score (NaN behind S)."""
    s, k, dk, d = shape
    prob = P.sense_problem(*shape, device=DEV, maps=P.BWD_MAPS, pad=True)
    like = torch.empty(1, 1, 1, d, device=DEV, dtype=dtype)
    dc = _bp().sense_mix_dc(prob['qk'].to(dtype), prob['dout'].to(dtype), _lse_in(prob['lse'], 2, k, s), prob['scale'], like)
    _exact_in(dtype, prob['want_dc'])
    _ok(P.grad_failures(dc, prob['want_dc'], prob['fan'], dtype, 'dc'), f'{shape} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', P.MIX_DQK, ids=lambda s: 'x'.join(map(str, s)))
def test_sense_dqk_vanishes_within_its_rounding(shape, dtype):
    """Sparse dout (at most four non-zero columns, 1 or 2): dP = dout . C is an integer <= 64, exact in the 16-bit slab;
    dq and dk stay within prefill_needles.dqk_bounds (module docstring).  S = 257 and 641: slabs that start at 128 ... 640."""
    s, k, dk, d = shape
    prob = P.sense_problem(*shape, device=DEV, maps=P.BWD_MAPS, sparse=True, pad=True)
    dqk = _bp().sense_dqk(prob['qk'].to(dtype), prob['content'].to(dtype), prob['dout'].to(dtype),
                          _lse_in(prob['lse'], 2, k, s), prob['scale'])
    bound_q, bound_k = P.dqk_bounds(prob, dtype)
    print(f'{shape} {dtype}: |dq| {dqk[:, :, 0].abs().max().item():.3e} (bound {bound_q:.3e}), '
          f'|dk| {dqk[:, :, 1].abs().max().item():.3e} (largest bound {bound_k.max().item():.3e})')
    _ok(P.dust_failures(dqk[:, :, 0], bound_q, 'dq') + P.dust_failures(dqk[:, :, 1], bound_k, 'dk'), f'{shape} {dtype}')
