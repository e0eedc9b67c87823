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
  (single needles; the pair problems further down give dQ, dK and dqk their non-zero values)

Outputs the caller allocates hold NaN before the call; what a call must not read is poisoned: rows past cu_seqlens and
LSE entries past a sequence (NaN / magnitude 8), the odd rows of the gather table, the columns behind a narrower view.

The non-zero arithmetic of dQ, dK and dqk, which a single needle cannot reach (P = 1 makes dS vanish), is tested by the PAIR
problems at the end of this file: two needles per row with bit-equal scores, P = 1/2 each, closed forms for everything
(tests/prefill_needles.py, second half):

  forward      out == (V[j1] + V[j2]) / 2 (sum over senses) bit for bit, LSE = score + ln 2 within the decode tolerance
  dQ, dK, dV   flash_bwd: == scale (n / 4) (K[j1] - K[j2]), scale sum +- (n / 4) Q_i, sum P dO_i bit for bit where not 0;
               where 0: 1e-6 / 1e-12, plus FP32_SUM (2^-22) of the terms where non-zero terms cancel (bf16: the matrix unit
               leaves -2^-24 of a group's largest product next to the others' -1e-21; fp16 gives exact zeros)
  dC           sense_mix_dc: bit for bit
  dqk          sense_dqk: within prefill_needles.pair_dqk_bounds (< scale / 8; one wrong term moves an entry by >= scale / 2);
               dq bit for bit on the rows whose needles both lie in the first 32 keys (exact row reference).  dk is NOT held to
               bit equality: its D = sum P dP carries the rebuilt P's error e ~ 1e-5, a row with n = 0 leaves e mean dP / 2
               in 16 bit, and fp16 shows the sum of those next to a non-zero entry (measured 3.9e-3 = one fp16 ulp at 6)
  wide route   sense_mix_autograd at d_k = 160 (_sense_mix_backward_rebuild): bit for bit, as its host model predicts

First finding of the pair tests, fixed in csrc/flash_fwd_dma.hip: a masked (diagonal / last) tile rescaled O and l by
exp2(m c2 - fl(m c2)), the rounding error of the product, when the tile did not raise the row's maximum -- 1 + 2e-5 instead
of 1 at m c2 ~ 500, which left 3e-5 where (V[j1] + V[j2]) / 2 = 0 with the needles in different tiles (d = 64, 128).

Dropout in the forward and the backward is tested exactly in tests/test_gpu_dropout_exact.py.
NOT tested here: key_weight in the fused sense backward (it has none), and a paired row taking
another paired row's LSE (they share one; row 0, with one needle, has another, and another row's D is seen).  A live key tile
that holds no needle (mutant 7 below) is the subject of tests/test_gpu_tie_blocks.py: rows whose weight lies on 16 ... 2048 keys
tied bit for bit, where that mutant fails every forward case of the LDS-DMA kernel.  Non-unit rescale factors between live tiles
stay parity-only there as well: score steps between tiles are not exact powers of two under fl(scale log2e).

Two places where the kernels' own arithmetic is not exact on these inputs, each with a derived bound instead:
  * flash_fwd_dma.hip:282-285 and 487: the LSE is the logarithm of the sum of ROUNDED p.  In the stale-reference case that
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


# ---- two needles per row: the non-zero arithmetic of dQ, dK and dqk ----------------------------------------------------------

def _rows_lse_in(lse, tail=NAN):
    """Per-row LSEs (b, g, s) -> the (b, g, roundup(s, 16)) fp32 buffer, NaN behind the rows."""
    b, g, s = lse.shape
    buf = torch.full((b, g, -(-s // 16) * 16), tail, device=DEV)
    buf[:, :, :s] = lse.float()
    return buf


def _with_tail(x, rows=16):
    """x (n, ...) as the head of a buffer with `rows` more rows of NaN -> (buffer, view)."""
    buf = torch.full((x.shape[0] + rows,) + tuple(x.shape[1:]), NAN, device=DEV, dtype=x.dtype)
    return buf, buf[:x.shape[0]]


def _pair_flash_fwd(bp, prob, dtype, causal, tag):
    b, sq, h, d = prob['q'].shape
    sk = prob['k'].shape[1]
    q, k, v = (prob[x].to(dtype).reshape(-1, h, d) for x in ('q', 'k', 'v'))
    out = torch.full_like(q, NAN)
    lse = bp.flash_fwd(q, k, v, out, None, None, sq, sk, prob['scale'], causal)
    _exact_in(dtype, prob['want'])
    _ok(P.exact_failures(out.view(b, sq, h, d), prob['want'], dtype, 'out', prob['zero_out']) + P.lse_failures(lse[:, :, :sq], prob['lse']), tag)
    return out, lse


def _pair_flash_bwd(bp, prob, dtype, causal, tag, chain=False):
    b, sq, h, d = prob['q'].shape
    sk = prob['k'].shape[1]
    q, k, v, dout = (prob[x].to(dtype).reshape(-1, h, d) for x in ('q', 'k', 'v', 'dout'))
    if chain:
        out, lse = _pair_flash_fwd(bp, prob, dtype, causal, tag + ' (forward)')
    else:
        out, lse = prob['want'].to(dtype).reshape(-1, h, d), _rows_lse_in(prob['lse'])
    bufs, (dq, dk, dv) = zip(*(_with_tail(x) for x in (q, k, v)))
    bp.flash_bwd(dout, q, k, v, out, lse, dq, dk, dv, None, None, sq, sk, prob['scale'], causal)
    _exact_in(dtype, prob['want_dq'], prob['want_dk'], prob['want_dv'])
    _ok(P.exact_failures(dq.view(b, sq, h, d), prob['want_dq'], dtype, 'dq', prob['zero_dq'])
        + P.exact_failures(dk.view(b, sk, h, d), prob['want_dk'], dtype, 'dk', prob['zero_dk'])
        + P.exact_failures(dv.view(b, sk, h, d), prob['want_dv'], dtype, 'dv'), tag)
    for buf, g in zip(bufs, (dq, dk, dv)):
        assert torch.isnan(buf[g.shape[0]:]).all(), f'{tag}: rows behind the call were written'


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', P.PAIR_BWD_CASES, ids=[f"d{c['d']}" for c in P.PAIR_BWD_CASES])
def test_pair_flash_bwd_gradients_are_their_closed_forms(case, dtype):
    """Causal, fixed length, S = 65 ... 641, the exact O = (V[j1] + V[j2]) / 2 and the per-row closed-form LSE handed in (NaN
    behind the rows): dQ = scale (n / 4) (K[j1] - K[j2]), dK = scale sum +- (n / 4) Q_i and dV = sum P dO_i bit for bit where
    they are not 0; where they are, dust (1e-6, 1e-12), plus prefill_needles.FP32_SUM of the terms where non-zero terms cancel.  Per dtype the value magnitudes of prefill_needles.PAIR_MAGS and, in
    bf16, without the (map, d, S) of PAIR_BF16_LEFT_OUT."""
    bp = _bp()
    for tag, prob in P.pair_fixed_problems(dtype, DEV, cases=[case]):
        _pair_flash_bwd(bp, prob, dtype, True, f'{tag} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_pair_flash_bwd_chained_to_the_forward(dtype):
    """O and LSE as bp.flash_fwd returns them on the pair problem: O bit for bit, the LSE within the decode tolerance, then
    the same exact gradients."""
    c = P.PAIR_CHAIN
    for tag, prob in P.pair_fixed_problems(dtype, DEV, cases=[dict(d=c['d'], seqlens=[c['s']])]):
        _pair_flash_bwd(_bp(), prob, dtype, True, f'chained {tag} {dtype}', chain=True)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_pair_flash_bwd_cross_lengths(dtype):
    """Not causal, sq = 150, sk = 333: the partner may lie behind the row."""
    for tag, prob in P.pair_cross_problems(dtype, DEV):
        _pair_flash_bwd(_bp(), prob, dtype, False, f'{tag} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_pair_flash_bwd_ragged_batch(dtype):
    """The ragged batch with its empty sequence: per-row LSEs of each sequence, NaN behind it; rows behind the batch poison
    in every input and NaN (unwritten) in every output."""
    bp = _bp()
    c = P.FLASH_BWD_RAGGED
    for tag, prob in P.pair_ragged_problems(dtype, DEV):
        total, top = prob['q'].shape[0], max(c['lens'])
        q, k, v, dout, out = _ragged_buffers(prob, dtype, ('q', 'k', 'v', 'dout', 'want'))
        lse = _lse_in(NAN, len(c['lens']), c['h'], top)
        for n, length in enumerate(c['lens']):
            if length:
                lse[n, :, :length] = prob['lse'][n].float()
        dq, dk, dv = torch.full_like(q, NAN), torch.full_like(k, NAN), torch.full_like(v, NAN)
        bp.flash_bwd(dout, q, k, v, out, lse, dq, dk, dv, prob['cu'], prob['cu'], top, top, prob['scale'], True)
        _exact_in(dtype, prob['want_dq'], prob['want_dk'], prob['want_dv'])
        _ok(P.exact_failures(dq[:total], prob['want_dq'], dtype, 'dq', prob['zero_dq'])
            + P.exact_failures(dk[:total], prob['want_dk'], dtype, 'dk', prob['zero_dk'])
            + P.exact_failures(dv[:total], prob['want_dv'], dtype, 'dv'), f'{tag} {dtype}')
        for g in (dq, dk, dv):
            assert torch.isnan(g[total:]).all(), 'rows behind cu_seqlens[-1] were written'


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', P.PAIR_FWD_CASES, ids=[f"d{c['d']}" for c in P.PAIR_FWD_CASES])
def test_pair_flash_fwd_rows_are_the_means_of_their_needles(case, dtype):
    """Two tied keys, 20 to 60 % of them in different 64-key tiles: out == (V[j1] + V[j2]) / 2 bit for bit needs the first
    tile's partial rescaled by exactly 1; LSE = score + ln 2 (row 0: its single needle's score)."""
    bp = _bp()
    for tag, prob in P.pair_fixed_problems(dtype, DEV, cases=[case], mags=P.PAIR_FWD_MAGS):
        _pair_flash_fwd(bp, prob, dtype, True, f'{tag} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', P.PAIR_MIX_FWD, ids=lambda s: 'x'.join(map(str, s)))
def test_pair_sense_mix_rows_are_the_sums_of_their_means(shape, dtype):
    """bp.sense_lse + bp.sense_mix on a pair problem (the narrow ring and the wide one): out == sum_l (C[j1_l] + C[j2_l]) / 2."""
    bp = _bp()
    s = shape[0]
    prob = P.pair_sense_problem(*shape, device=DEV, maps=P.FWD_MAPS, **P.PAIR_FWD_MAGS)
    qk, content = prob['qk'].to(dtype), prob['content'].to(dtype)
    lse = bp.sense_lse(qk, prob['scale'])
    out = torch.full_like(prob['want'], NAN, dtype=dtype)
    bp.sense_mix(qk, content, prob['scale'], out=out, lse=lse)
    _exact_in(dtype, prob['want'])
    _ok(P.lse_failures(lse[:, :, :s], prob['lse']) + P.exact_failures(out, prob['want'], dtype, 'out', prob['zero_out']), f'{shape} {dtype}')


def _pair_sense(shape, dtype):
    prob = P.pair_sense_problem(*shape, device=DEV, maps=P.pair_sense_maps(shape, dtype), pad=True, **P.PAIR_SENSE_MAGS[dtype])
    _exact_in(dtype, prob['want_dqk'], prob['want_dc'])
    return prob


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', P.PAIR_MIX_DQK, ids=lambda s: 'x'.join(map(str, s)))
def test_pair_sense_mix_dc_is_the_weighted_sum_of_its_rows(shape, dtype):
    """dC[s, l, :] = sum of P dout[t, :] over the rows that have s as a needle of sense l, P = 1/2 (1 for row 0): bit for bit."""
    prob = _pair_sense(shape, dtype)
    like = torch.empty(1, 1, 1, shape[3], device=DEV, dtype=dtype)
    dc = _bp().sense_mix_dc(prob['qk'].to(dtype), prob['dout'].to(dtype), _rows_lse_in(prob['lse']), prob['scale'], like)
    _ok(P.exact_failures(dc, prob['want_dc'], dtype, 'dc'), f'{shape} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', P.PAIR_MIX_DQK, ids=lambda s: 'x'.join(map(str, s)))
def test_pair_sense_dqk_is_its_closed_form_within_its_rounding(shape, dtype):
    """bp.sense_dqk with the closed-form per-row LSE: dq and dk within prefill_needles.pair_dqk_bounds of scale (n / 4)
    (K[j1] - K[j2]) and scale sum +- (n / 4) Q_i -- bounds under scale / 8, a quarter of what one wrong term moves; S = 257 and
    641 make slabs start at 128 ... 640 and dk_acc sum over up to six launches.  The rows whose two needles both lie in the
    first 32 keys have an exact row reference (the host model shows it: r = (dP_1 + dP_2) / 2), so their dq is bit for bit
    where it is not 0."""
    prob = _pair_sense(shape, dtype)
    dqk = _bp().sense_dqk(prob['qk'].to(dtype), prob['content'].to(dtype), prob['dout'].to(dtype), _rows_lse_in(prob['lse']),
                          prob['scale'])
    bound_q, bound_k = P.pair_dqk_bounds(prob, dtype)
    assert float(bound_q.max()) < prob['scale'] / 8 and float(bound_k.max()) < prob['scale'] / 8
    want_q, want_k = prob['want_dqk'][:, :, 0], prob['want_dqk'][:, :, 1]
    print(f'{shape} {dtype}: |dq - closed form| {(dqk[:, :, 0].double() - want_q).abs().max().item():.3e} (largest bound '
          f'{bound_q.max().item():.3e}), |dk - closed form| {(dqk[:, :, 1].double() - want_k).abs().max().item():.3e} (largest bound '
          f'{bound_k.max().item():.3e})')
    js, js2 = prob['js'], prob['js2']
    low = ((js2 != js) & (js < 32) & (js2 < 32)).permute(0, 2, 1)[..., None]
    _ok(P.near_failures(dqk[:, :, 0], want_q, bound_q, 'dq') + P.near_failures(dqk[:, :, 1], want_k, bound_k, 'dk')
        + P.exact_failures(torch.where(low, dqk[:, :, 0].double(), want_q), want_q, dtype, 'dq below key 32', bound_q), f'{shape} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_pair_wide_senses_through_the_alpha_rebuilding_route(dtype):
    """d_k = 160 (scale 2) through bp.sense_mix_autograd: the forward's own LSE, then _sense_mix_backward_rebuild (sense_alpha,
    BLAS products, softmax_bwd_causal_).  Its host model (16-bit alpha = 1/2, 16-bit integer dP, fp32 row sum) predicts bit
    equality, so dqk and dcontent are held to the exact criterion."""
    bp = _bp()
    prob = _pair_sense(P.PAIR_MIX_WIDE, dtype)
    assert prob['scale'] == 2.0
    qk, content = prob['qk'].to(dtype).requires_grad_(), prob['content'].to(dtype).requires_grad_()
    out = bp.sense_mix_autograd(qk, content, prob['scale'])
    out.backward(prob['dout'].to(dtype))
    _exact_in(dtype, prob['want'])
    _ok(P.exact_failures(out.detach(), prob['want'], dtype, 'out', prob['zero_out']) + P.exact_failures(qk.grad, prob['want_dqk'], dtype, 'dqk', prob['zero_dqk'])
        + P.exact_failures(content.grad, prob['want_dc'], dtype, 'dcontent'), f'wide {dtype}')
