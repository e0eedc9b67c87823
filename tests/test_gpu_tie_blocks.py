"""GPU: the softmax kernels on rows whose weight lies on MANY keys, equal bit for bit -- what the needle and pair tests of
tests/test_gpu_prefill_needles.py cannot see: there every key tile but the needle's weighs 1e-21, here every live tile, every
16-key group of it and every query tile's term counts, at any row.

Inputs, expected results and criteria: tests/tie_blocks.py (tie queries of order m over the +-1 position codes: full blocks
with P = 2^-m on 2^m keys, m = 4, 6 across two key tiles, 7 = two whole tiles; own blocks with P = 1 / r, r = 1 ... 64, on the
masked diagonal tile; flat rows with P = 1 / (i + 1)).  tests/test_tie_blocks_host.py proves on the CPU, for the same case
lists, that an fp32 model of the kernels' order and fp64 autograd meet the criteria and that the named mutants do not.

  forward      flash_fwd: full-block rows == the block mean (representable) bit for bit; 1 / n rows == the 16-bit rounding of
               sum / n bit for bit unless that rounding depends on the 2^-21 an fp32 sum * (1 / l) may be off by (then one of the
               two neighbours; <= 10 % of a call's rows, counted on the host); an exact 0 within DUST + FP32_SUM of the terms;
               LSE = score + ln n within the decode tolerance, which is < ln(1 + 1 / n) / 2 on every row
  probs        attn_probs from the forward's LSE and from the closed-form LSE: the 16-bit rounding of 1 / n bit for bit (2^-m
               always; 1 / n unless within tie_blocks.row_p_error of a rounding tie), exactly 0 where masked, <= 2e-21 elsewhere
  dV           flash_bwd on full blocks: == the ONE 16-bit rounding of the exact fp32 sum of 2^-m dO, bit for bit (no entry excused)
  dQ, dK       within tie_blocks.grad_bounds of the fp64 closed forms: the rebuilt P's error, ONE 16-bit rounding of dS, fp32
               sums -- a bound relative to sum |dS| |k| of the entry, 2^-8 (bf16) of it; a query tile's term missing is 1 / 10 of it
               or more (the host test shows both mutants outside).  Bit for bit where every intermediate is representable: a dO
               with a single 1 per row, orders m <= 3 in fp16 and m <= 2 (3 at the short lengths) in bf16
               (tie_blocks.exact_grad_slots; above that a sum over 2^m keys of (m + 2)-bit terms outgrows the dtype)
  sense        sense_lse + sense_mix (dense, gather, varlen, key_weight in {0, 1/2, 1, 2}, the staged and the wide routes), every
               sense with a full-block map of its own: out == the rounding of the exact sum over senses of the block means, bit
               for bit (positive content: the other keys' 1e-21 only add and an fp32 sum absorbs them); sense_alpha as attn_probs;
               dC of sense_mix_dc and dcontent of the alpha-rebuilding route (d_k = 160) bit for bit, its dqk within
               tie_blocks.rebuild_dqk_bounds; sense_dqk, full-block and 1 / n senses, within the bounds of tie_blocks.dqk_forms
               (the model of prefill_needles.pair_dqk_bounds on many live keys)
  decode       flash_decode (64 / 8 / 1 splits) and sense_decode (table, cache, weighted), L = 63 ... 4096: every tie count a
               power of two (tie_blocks.decode_maps), so every split weight and product is exact: out bit for bit, LSE, the
               appended row, NaN behind it; flat rows and cut blocks with any other count within tie_blocks.decode_bound
  1 / n rows   own-block and flat rows where a kernel rebuilds P from an LSE and ROUNDS it (the mix in every form, dC, dV): within
               tie_blocks.mix_bound, the full-block senses / slots next to them still bit for bit; dQ, dK within grad_bounds

Outputs hold NaN before the call; rows behind cu_seqlens and LSE entries behind a sequence are poison, as in the needle file.

NOT covered: dropout.  key_weight in the fused sense backward (it has none) and non-unit rescale factors between live tiles stay parity-only:
score steps between tiles are not exact powers of two under fl(scale log2e).

No criterion failed on the unmodified kernels: there is no finding to report and no kernel changed.

Mutation run.  Single mutants of the kernels' arithmetic, never an address or a bound; each built as a variant library, selected
with BP_HIP_LIB.  The "here" counts are over 78 cases of this file: the forward, probability, test_flash_bwd_on_full_blocks /
chained / cross / ragged, full-block sense (mix, staged, gather, key_weight on the narrow ring, varlen, alpha, dC, the wide route's out and dcontent)
and test_flash_decode_rows_are_the_means_of_their_tied_keys tests.  The other tests of this file -- sense_decode, sense_dqk, the
wide route's dqk, the 1 / n rows of the mix, dC and flash_bwd, the exact dQ / dK slots, decode rows with any tie count -- have
faced no kernel mutant on the GPU but 7: only the host models of the mutants in tests/test_tie_blocks_host.py stand behind them (c would
reach sense_decode and the flat decode rows, d the mixed dC).  "needles" = tests/test_gpu_prefill_needles.py, 151 cases.  Number =
failing cases; "-" = no such run (the needle file launches no decode kernel, so c cannot fail there).  No variant is committed.

  mutant                                                                        here   needles   killed here by
  7' flash_fwd_dma.hip: l_run takes the row sum of EVERY kept steady-state       34      11      every flash_fwd case of the LDS-DMA
     tile twice (l_run += (fast_entry && !exact) ? 2 rs : rs)                                    kernel (d = 8, 64, 128, cross, ragged),
                                                                                                 the mixes through their LSE pre-pass,
                                                                                                 sense_alpha's sense_lse, chained bwd
  k  flash_fwd_dma.hip: accumulate_packed skips the second 16-key step of        16       9      every flash_fwd case of that kernel,
     every kept steady-state tile                                                                attn_probs from its LSE, chained bwd
  2  flash_fwd_dma.hip: l_run takes key tile 2's row sum twice (fast entry)      32      42      flash_fwd from three key tiles on, the
                                                                                                 mixes and sense_alpha through the LSE
  5  mix_ring.h, mix_x_block: register 11 of the second half has P = 0          10      20      the ring mixes (dense, gather, varlen)
                                                                                                 and dC at S = 641
  c  decode_core.h, decode_combine_kernel: split 1 takes split 0's weight         8       -      flash_decode, 64 and 8 splits (one
                                                                                                 split has no split 1)
  b  flash_bwd.hip, dK/dV: the second 32-query sub-block of the clean query       6      22      dV and dK at S = 641 and 385 (fixed,
     tiles 256 rows or more below the key tile is dropped                                        chained)
  d  sense_mix_bwd.hip, dC: register 5 of query half 0 has P = 0 in a clean       2       -      dC at S = 641 (the shorter dC cases have
     (non-diagonal) step                                                                         no clean step: one 256-key workgroup)

  7  flash_fwd_dma.hip: l_run takes the row sum of ONE kept steady-state         40*     11      every flash_fwd case of the LDS-DMA
     tile, key tile 1, twice (... && kb == 1)                                                    kernel with three or more key tiles (d =
                                                                                                 8, 64, 128, cross, ragged), attn_probs
                                                                                                 from its LSE, the chained backward, the
                                                                                                 narrow mixes and sense_alpha through the
                                                                                                 LSE pre-pass, the mixed mix tests
  * of all 128 cases of this file (the only mutant run against all of them).

Mutant 7 is the needle file's mutant 7 ("a KEPT steady-state tile", 1 of 23 forward cases there when it was written; 11 of 151 now,
all pair or stale-reference cases: a pair across two tiles keeps the second one).  7' doubles every kept tile and is louder.
Both, and k, fail every forward case with three or more key tiles here except d = 36, which runs the register-staged
csrc/flash_fwd.hip, not the mutated file; the host's 'sum2' mutant is the model of 7.
"""
import pytest
import torch

import prefill_needles as P
import tie_blocks as T

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


def _rows_lse_in(lse, tail=NAN):
    """Per-row LSEs (b, g, s) -> the (b, g, roundup(s, 16)) fp32 buffer, NaN behind the rows."""
    b, g, s = lse.shape
    buf = torch.full((b, g, -(-s // 16) * 16), tail, device=DEV)
    buf[:, :, :s] = lse.float()
    return buf


def _flash_fwd(bp, prob, dtype, tag):
    b, sq, h, d = prob['q'].shape
    sk = prob['k'].shape[1]
    q, k, v = (prob[x].to(dtype).reshape(-1, h, d) for x in ('q', 'k', 'v'))
    out = torch.full_like(q, NAN)
    lse = bp.flash_fwd(q, k, v, out, None, None, sq, sk, prob['scale'], prob['causal'])
    _ok(T.mean_failures(out.view(b, sq, h, d), prob['want'], dtype, 'out', T.zero_out(prob))
        + T.lse_failures(lse[:, :, :sq], prob['lse']), tag)
    return out, lse


# ---- forward ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', T.FLASH_FWD_CASES, ids=[f"d{c['d']}" for c in T.FLASH_FWD_CASES])
def test_flash_fwd_rows_are_the_means_of_their_tied_keys(case, dtype):
    """Causal, fixed length, S = 129 ... 641 (d = 8: up to 223 + the offset), three (sample, head) slots with a map each, the
    nine maps of tie_blocks.FWD_MAPS in three calls; d = 36 takes the register-staged kernel."""
    bp = _bp()
    for tag, prob in T.fixed_problems(case, T.FWD_MAPS, dtype, DEV):
        _flash_fwd(bp, prob, dtype, f'{tag} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('c', T.FLASH_CROSS, ids=lambda c: f"sk{c['sk']}")
def test_flash_fwd_cross_lengths(c, dtype):
    """Not causal, sq = 150: blocks anywhere among the keys; a flat row weighs all Sk keys alike, 2^-8 exactly at Sk = 256."""
    for tag, prob in T.cross_problems(c, dtype, DEV):
        _flash_fwd(_bp(), prob, dtype, f'{tag} {dtype}')


def _ragged_buffers(prob, dtype, names, pad=64):
    total = prob['q'].shape[0]
    bufs = []
    for n, x in enumerate(names):
        buf = torch.full((total + pad,) + tuple(prob[x].shape[1:]), 8.0 * (-1) ** n, device=DEV, dtype=dtype)
        buf[:total] = prob[x].to(dtype)
        bufs.append(buf)
    return bufs


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_flash_fwd_ragged_batch(dtype):
    """cu_seqlens with sequences that start inside a tile: blocks are relative to each sequence, value ids carry its index."""
    bp = _bp()
    c = T.FLASH_RAGGED
    for tag, prob in T.ragged_problems(dtype, DEV):
        total = prob['q'].shape[0]
        q, k, v = _ragged_buffers(prob, dtype, ('q', 'k', 'v'))
        out = torch.full_like(q, NAN)
        lse = bp.flash_fwd(q, k, v, out, prob['cu'], prob['cu'], max(c['lens']), max(c['lens']), prob['scale'], True)
        bad = T.mean_failures(out[:total], prob['want'], dtype, 'out', P.DUST + P.FP32_SUM * prob['abs_want'])
        for n, (length, part) in enumerate(zip(c['lens'], prob['parts'])):
            bad += T.lse_failures(lse[n, :, :length], part['lse'][0], f'LSE of sequence {n}')
        _ok(bad, f'{tag} {dtype}')
        assert torch.isnan(out[total:]).all(), 'rows behind cu_seqlens[-1] were written'


# ---- probabilities ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('causal', [False, True])
def test_attn_probs_from_a_given_lse(causal, dtype):
    """bp.attn_probs with the closed-form per-row LSE over the store widths of PROBS_SK, d = 64: P == rnd16(1 / n)."""
    bp = _bp()
    maps = T.FWD_MAPS if causal else T.CROSS_MAPS
    for sk in T.PROBS_SK:
        prob = T.attn_problem(P.slot_maps(maps, 3, sk), 1, 3, sk, sk, 64, dtype, DEV, causal=causal, cols=8)
        p = bp.attn_probs(prob['q'].to(dtype), prob['k'].to(dtype), _rows_lse_in(prob['lse']), prob['scale'], causal)
        _ok(T.probs_failures(p, prob, dtype, f'sk={sk} causal={causal} {dtype}', T.row_p_error(prob)), 'attn_probs')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_attn_probs_from_the_forward_lse(dtype):
    """The LSE as bp.flash_fwd returns it, over the store widths of PROBS_SK, full-block slots: P = 2^-m (1 for the rows of order 0) must come out exactly.
    LSE_TOL is too wide to promise that (3e-3 at an LSE of 288), the forward's arithmetic is not: lse = (fl(m c2) + log2 l) ln 2
    (csrc/flash_fwd_dma.hip:369, 487; log2 of a power of two is exact) is three fp32 roundings of a number below 1024 log2-units,
    attn_probs' fl(lse log2e) a fourth: 4 half-ulps = 1.2e-4 in the exponent, 8.5e-5 of P (tie_blocks.lse_error), plus p_error <
    half an ulp below a power of two in either dtype."""
    bp = _bp()
    for sk in T.PROBS_SK:
        prob = T.attn_problem(P.slot_maps(T.BWD_MAPS, 3, sk), 1, 3, sk, sk, 64, dtype, DEV)
        _, lse = _flash_fwd(bp, prob, dtype, f'forward sk={sk} {dtype}')
        e = T.lse_error(prob) + T.p_error(64)
        assert e < P.HALF_ULP[dtype]
        p = bp.attn_probs(prob['q'].to(dtype), prob['k'].to(dtype), lse, prob['scale'], True)
        _ok(T.probs_failures(p, prob, dtype, f'sk={sk} {dtype}', e), 'attn_probs')


# ---- backward -------------------------------------------------------------------------------------------------------------------

def _grad_failures(dq, dk, dv, prob, dtype, d):
    bq, bk = T.grad_bounds(prob, dtype, T.p_error(d))
    return (T.mean_failures(dv, prob['want_dv'], dtype, 'dv', rel=0.0) + P.near_failures(dq, prob['want_dq'], bq, 'dq')
            + P.near_failures(dk, prob['want_dk'], bk, 'dk'))


def _flash_bwd(bp, prob, dtype, tag, chain=False):
    b, sq, h, d = prob['q'].shape
    sk = prob['k'].shape[1]
    q, k, v, dout = (prob[x].to(dtype).reshape(-1, h, d) for x in ('q', 'k', 'v', 'dout'))
    if chain:
        out, lse = _flash_fwd(bp, prob, dtype, tag + ' (forward)')
    else:
        out, lse = prob['want'].to(dtype).reshape(-1, h, d), _rows_lse_in(prob['lse'])
    dq, dk, dv = torch.full_like(q, NAN), torch.full_like(k, NAN), torch.full_like(v, NAN)
    bp.flash_bwd(dout, q, k, v, out, lse, dq, dk, dv, None, None, sq, sk, prob['scale'], prob['causal'])
    _ok(_grad_failures(dq.view(b, sq, h, d), dk.view(b, sk, h, d), dv.view(b, sk, h, d), prob, dtype, d), tag)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', T.FLASH_BWD_CASES, ids=[f"d{c['d']}" for c in T.FLASH_BWD_CASES])
def test_flash_bwd_on_full_blocks(case, dtype):
    """Causal, S = 129, 257, 641, the exact O (representable) and the closed-form LSE handed in, dense dO in {1, 2}: dV bit for
    bit, dQ and dK within their bounds of the closed forms."""
    bp = _bp()
    for tag, prob in T.fixed_problems(case, T.BWD_MAPS, dtype, DEV):
        _flash_bwd(bp, prob, dtype, f'{tag} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_flash_bwd_chained_to_the_forward(dtype):
    """O and LSE as bp.flash_fwd returns them, S = 385."""
    bp = _bp()
    for tag, prob in T.fixed_problems(dict(d=64, seqlens=[385]), T.BWD_MAPS, dtype, DEV):
        _flash_bwd(bp, prob, dtype, f'chained {tag} {dtype}', chain=True)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_flash_bwd_cross_lengths(dtype):
    """Not causal, sq = 150, sk = 333."""
    for tag, prob in T.cross_problems(T.FLASH_CROSS[1], dtype, DEV, maps=T.BWD_MAPS):
        _flash_bwd(_bp(), prob, dtype, f'{tag} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_flash_bwd_ragged_batch(dtype):
    """The ragged batch: per-row LSEs of each sequence, NaN behind it; rows behind the batch poison in every input and NaN
    (unwritten) in every output."""
    bp = _bp()
    c = T.FLASH_RAGGED
    for tag, prob in T.ragged_problems(dtype, DEV, maps=T.BWD_MAPS):
        total, top = prob['q'].shape[0], max(c['lens'])
        q, k, v, dout, out = _ragged_buffers(prob, dtype, ('q', 'k', 'v', 'dout', 'want'))
        lse = torch.full((len(c['lens']), c['h'], -(-top // 16) * 16), NAN, device=DEV)
        for n, (length, part) in enumerate(zip(c['lens'], prob['parts'])):
            lse[n, :, :length] = part['lse'][0].float()
        dq, dk, dv = torch.full_like(q, NAN), torch.full_like(k, NAN), torch.full_like(v, NAN)
        bp.flash_bwd(dout, q, k, v, out, lse, dq, dk, dv, prob['cu'], prob['cu'], top, top, prob['scale'], True)
        _ok(_grad_failures(dq[:total], dk[:total], dv[:total], prob, dtype, c['d']), f'{tag} {dtype}')
        for g in (dq, dk, dv):
            assert torch.isnan(g[total:]).all(), 'rows behind cu_seqlens[-1] were written'


# ---- sense kernels: LSE, alpha, mix --------------------------------------------------------------------------------------------

def _behind_a_view(x, dtype, extra=8, offset=0, poison=8.0):
    """x as a view of a buffer with `extra` more columns (poison), starting at column `offset`."""
    buf = torch.full(tuple(x.shape[:-1]) + (x.shape[-1] + extra,), poison, device=DEV, dtype=dtype)
    view = buf[..., offset:offset + x.shape[-1]]
    view.copy_(x)
    return buf, view


def _sum_failures(got, want, dtype, name):
    """An exact fp32 sum of positive terms, rounded once: bit for bit (tie_blocks.sense_problem); 0 (all weights 0): dust."""
    return T.mean_failures(got, want, dtype, name, rel=0.0)


def _mix(bp, prob, dtype, tag, offset=0, gather=False):
    b, s, _, k, _ = prob['qk'].shape
    _, qk = _behind_a_view(prob['qk'], dtype)
    lse = bp.sense_lse(qk, prob['scale'])
    bad = T.lse_failures(lse[:, :, :s], prob['lse'])
    out_buf, out = _behind_a_view(torch.full_like(prob['want'], NAN, dtype=torch.float32), dtype, poison=NAN)
    if gather:
        table = prob['table'].to(dtype)
        table[1::2] = -8.0
        bp.sense_mix_gather(qk, table, prob['rows'], prob['scale'], out=out, lse=lse)
    else:
        _, content = _behind_a_view(prob['content'], dtype, offset=offset)
        bp.sense_mix(qk, content, prob['scale'], out=out, lse=lse, key_weight=prob['key_weight'])
    _ok(bad + _sum_failures(out, prob['want'], dtype, 'out'), tag)
    assert torch.isnan(out_buf[..., out.shape[-1]:]).all(), f'{tag}: columns behind the output view were written'


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', T.MIX_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_sense_mix_rows_are_the_sums_of_their_block_means(shape, dtype):
    """bp.sense_lse + bp.sense_mix, every sense with a full-block map of its own (m = 4, 6 across two tiles, 7; last block and
    earlier ones): out == rnd16(sum_l 2^-m_l sum C) bit for bit, the LSE per (sense, row) within the decode tolerance.  The
    narrow ring, the zero-padded d_k = 10, the wide ring, the staged wide kernel; views eight columns wider than the operands."""
    _mix(_bp(), T.sense_problem(*shape, device=DEV), dtype, f'{shape} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_sense_mix_staged_route(dtype):
    """Content viewed at a 2-byte offset: the register-staged csrc/sense_mix.hip."""
    _mix(_bp(), T.sense_problem(*T.MIX_STAGED, device=DEV), dtype, f'staged {dtype}', offset=1)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', T.MIX_GATHER, ids=lambda s: 'x'.join(map(str, s)))
def test_sense_mix_gather(shape, dtype):
    """Content rows through a 1024-row table whose odd rows (never named) hold -8."""
    _mix(_bp(), T.sense_problem(*shape, device=DEV, form='gather'), dtype, f'gather {shape} {dtype}', gather=True)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', T.MIX_WEIGHTED, ids=lambda s: 'x'.join(map(str, s)))
def test_sense_mix_key_weights(shape, dtype):
    """key_weight in {0, 1/2, 1, 2}, a hash of (sample, sense, key), on every route of the mix: every tied key of a block with a
    weight of its own, the sum still an exact fp32 number."""
    _mix(_bp(), T.sense_problem(*shape, device=DEV, weighted=True), dtype, f'weighted {shape} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_sense_mix_varlen(dtype):
    """The packed batch [70, 1, 130, 257, 5]: blocks relative to each sequence, rows behind the batch poison / NaN."""
    bp = _bp()
    c = T.MIX_VARLEN
    prob = T.sense_varlen_problem(c['lens'], c['k'], c['dk'], c['dout'], DEV)
    total, top = prob['qk'].shape[0], max(c['lens'])
    qk = torch.full((total + 16,) + tuple(prob['qk'].shape[1:]), 8.0, device=DEV, dtype=dtype)
    content = torch.full((total + 16,) + tuple(prob['content'].shape[1:]), -8.0, device=DEV, dtype=dtype)
    qk[:total], content[:total] = prob['qk'].to(dtype), prob['content'].to(dtype)
    lse = bp.sense_lse_varlen(qk, prob['cu'], top, prob['scale'])
    out = torch.full((total + 16, c['dout']), NAN, device=DEV, dtype=dtype)
    bp.sense_mix_varlen(qk, content, prob['cu'], top, prob['scale'], out=out, lse=lse)
    bad = _sum_failures(out[:total], prob['want'], dtype, 'out')
    for n, (length, part) in enumerate(zip(c['lens'], prob['parts'])):
        bad += T.lse_failures(lse[n, :, :length], part['lse'][0], f'LSE of sequence {n}')
    _ok(bad, f'varlen {dtype}')
    assert torch.isnan(out[total:]).all(), 'rows behind cu_seqlens[-1] were written'


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', T.ALPHA_CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_sense_alpha_from_a_given_lse(shape, dtype):
    """bp.sense_alpha with the closed-form LSE, the nine maps of FWD_MAPS over the senses (own blocks and flat rows too):
    alpha == rnd16(1 / n) on the tied keys (tie_blocks.row_p_error), exactly 0 above the diagonal, <= 2e-21 elsewhere; and
    bp.sense_lse on the same problem."""
    s, k, dk = shape
    bp = _bp()
    prob = T.sense_problem(s, k, dk, 8, device=DEV, maps=T.FWD_MAPS, pad=True)
    qk = prob['qk'].to(dtype)
    _ok(T.lse_failures(bp.sense_lse(qk, prob['scale'])[:, :, :s], prob['lse']), f'{shape} {dtype}')
    alpha = bp.sense_alpha(qk, prob['scale'], lse=_rows_lse_in(prob['lse']))
    _ok(T.probs_failures(alpha, prob, dtype, f'{shape} {dtype}', T.row_p_error(prob)), 'sense_alpha')


# ---- sense backward --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', T.MIX_DC, ids=lambda s: 'x'.join(map(str, s)))
def test_sense_mix_dc_is_the_weighted_sum_of_its_rows(shape, dtype):
    """dC[s, l, :] = sum_t 2^-m_l(t) dout[t, :] over the rows whose block holds s, dense dout in {1, 2}, the closed-form LSE
    handed in: the rounding of an exact fp32 sum, bit for bit."""
    s, k, dk, d = shape
    prob = T.sense_problem(*shape, device=DEV, pad=True)
    like = torch.empty(1, 1, 1, d, device=DEV, dtype=dtype)
    dc = _bp().sense_mix_dc(prob['qk'].to(dtype), prob['dout'].to(dtype), _rows_lse_in(prob['lse']), prob['scale'], like)
    _ok(_sum_failures(dc, prob['want_dc'], dtype, 'dc'), f'{shape} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_wide_senses_through_the_alpha_rebuilding_route(dtype):
    """d_k = 160 through bp.sense_mix_autograd (the forward's own LSE, then sense_alpha and BLAS products), dense dO: out and
    dcontent bit for bit (16-bit alpha = 2^-m exactly, sums of positive multiples of 2^-7).  dqk: the next test but one."""
    bp = _bp()
    prob = T.sense_problem(*T.MIX_WIDE_AUTOGRAD, device=DEV)
    qk, content = prob['qk'].to(dtype).requires_grad_(), prob['content'].to(dtype).requires_grad_()
    out = bp.sense_mix_autograd(qk, content, prob['scale'])
    out.backward(prob['dout'].to(dtype))
    _ok(_sum_failures(out.detach(), prob['want'], dtype, 'out') + _sum_failures(content.grad, prob['want_dc'], dtype, 'dcontent'),
        f'wide {dtype}')


# ---- decode: the split kernel and its combine --------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', T.DECODE_CASES, ids=[f"d{c['d']}-{c['regime']}" for c in T.DECODE_CASES])
def test_flash_decode_rows_are_the_means_of_their_tied_keys(case, dtype):
    """bp.flash_decode at L = 63, 64, 65, 1000, 2047, 4096 in the three split regimes (64 splits, 8, 1): every (sample, head)
    row with a block of its own -- inside one split, across split borders, around the appended key -- and, where L + 1 is a
    power of two, flat rows that make all active splits weigh alike.  Every split's weight is then a power of two
    (tie_blocks.decode_maps), so out == the rounding of the exact mean bit for bit and the LSE is score + ln n; the cache rows
    behind L are NaN, row L must hold the appended key and value afterwards."""
    bp = _bp()
    b, h, d, ms = case['batch'], case['heads'], case['d'], case['max_seqlen']
    cache = torch.full((b, ms, 2, h, d), NAN, device=DEV, dtype=dtype)
    for L in T.DECODE_LENGTHS:
        prob = T.decode_problem(case, L, dtype, DEV)
        cache[:, :L, 0], cache[:, :L, 1] = prob['keys'][:, :L].to(dtype), prob['vals'][:, :L].to(dtype)
        cache[:, L:] = NAN
        k_new, v_new = prob['keys'][:, L].to(dtype).contiguous(), prob['vals'][:, L].to(dtype).contiguous()
        out = torch.full((b, h, d), NAN, device=DEV, dtype=dtype)
        seqlens = torch.full((b,), L, dtype=torch.int32, device=DEV)
        _, lse = bp.flash_decode(prob['q'].to(dtype), k_new, v_new, cache, seqlens, prob['scale'], out=out, return_lse=True)
        _ok(T.mean_failures(out, prob['want'], dtype, 'out', T.zero_out(prob), rel=0.0) + T.lse_failures(lse, prob['lse']),
            f"{case['regime']} d={d} L={L} {dtype}")
        assert torch.equal(cache[:, L, 0], k_new) and torch.equal(cache[:, L, 1], v_new), 'row L must hold the appended key and value'
        assert torch.isnan(cache[:, L + 1:]).all(), 'rows behind L were written'


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('form', ['table', 'cache', 'weighted'])
@pytest.mark.parametrize('case', T.SENSE_DECODE_CASES, ids=[f"{c['dkp']}x{c['k']}x{c['dout']}" for c in T.SENSE_DECODE_CASES])
def test_sense_decode_rows_are_the_sums_of_their_block_means(case, form, dtype):
    """bp.sense_decode (table form, cache form, and the table form with key_weight in {0, 1/2, 1, 2}: bp_sense_decode_weighted)
    at the lengths of the trunk test, every (sample, sense) with a block of its own as there: out == the rounding of the exact
    sum over senses, bit for bit.  Unnamed table rows hold -8, the key cache is NaN behind L, row L must hold the appended key
    and row afterwards."""
    bp = _bp()
    b, k, dk, ms = case['batch'], case['k'], case['dk'], case['max_seqlen']
    k_cache = torch.full((b, ms, k, dk), NAN, device=DEV, dtype=dtype)
    for L in T.DECODE_LENGTHS:
        prob = T.sense_decode_problem(case, L, 'cache' if form == 'cache' else 'table', form == 'weighted', DEV)
        table = prob['table'].to(dtype)
        if form != 'cache':
            table[1::2] = -8.0
        k_cache[:, :L] = prob['keys'][:, :L].to(dtype)
        k_cache[:, L:] = NAN
        rows = torch.ones(b, ms, dtype=torch.int32, device=DEV)               # row 1: never named (odd, or sample 0's key 1 ...)
        rows[:, :L] = prob['rows'][:, :L]
        new_row = prob['rows'][:, L].contiguous()
        k_new = prob['keys'][:, L].to(dtype).contiguous()
        kw = None
        if prob['key_weight'] is not None:
            kw = torch.full((b, k, ms), NAN, device=DEV)
            kw[:, :, :L + 1] = prob['key_weight']
        out = torch.full((b, table.shape[-1]), NAN, device=DEV, dtype=dtype)
        seqlens = torch.full((b,), L, dtype=torch.int32, device=DEV)
        bp.sense_decode(prob['q'].to(dtype), k_new, k_cache, table, rows, new_row, seqlens, prob['scale'], out=out, key_weight=kw)
        _ok(_sum_failures(out, prob['want'], dtype, 'out'), f'{form} {case} L={L} {dtype}')
        assert torch.equal(k_cache[:, L], k_new) and torch.equal(rows[:, L], new_row), 'position L must hold the appended key and row'
        assert torch.isnan(k_cache[:, L + 1:]).all(), 'rows behind L were written'


# ---- 1 / n rows where the kernel rebuilds P from an LSE and rounds it: derived bounds ------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', T.MIX_MIXED, ids=lambda s: 'x'.join(map(str, s)))
def test_sense_mix_and_dc_with_own_block_and_flat_senses(shape, dtype):
    """The nine maps of FWD_MAPS over the senses: own-block (P = 1 / r on the diagonal tile) and flat (P = 1 / (t + 1)) senses
    next to full-block ones, dense, through the gather table and with key_weight.  The mix and dC round the rebuilt P to 16 bit, so a 1 / n term
    is inexact: out and dC within tie_blocks.mix_bound, dC of the full-block senses still bit for bit, the LSE of every (sense,
    row) within the decode tolerance (it counts the keys)."""
    bp = _bp()
    s, k, dk, d = shape
    for form in ('dense', 'gather'):
        prob = T.sense_problem(*shape, device=DEV, maps=T.FWD_MAPS, form=form)
        qk = prob['qk'].to(dtype)
        lse = bp.sense_lse(qk, prob['scale'])
        out = torch.full_like(prob['want'], NAN, dtype=dtype)
        if form == 'gather':
            table = prob['table'].to(dtype)
            table[1::2] = -8.0
            bp.sense_mix_gather(qk, table, prob['rows'], prob['scale'], out=out, lse=lse)
        else:
            bp.sense_mix(qk, prob['content'].to(dtype), prob['scale'], out=out, lse=lse)
        _ok(T.lse_failures(lse[:, :, :s], prob['lse']) + P.near_failures(out, prob['want'], T.mix_bound(prob, dtype, prob['want']), 'out'),
            f'{form} {shape} {dtype}')
    prob = T.sense_problem(*shape, device=DEV, maps=T.FWD_MAPS, weighted=True)
    qk = prob['qk'].to(dtype)
    out = torch.full_like(prob['want'], NAN, dtype=dtype)
    bp.sense_mix(qk, prob['content'].to(dtype), prob['scale'], out=out, lse=bp.sense_lse(qk, prob['scale']), key_weight=prob['key_weight'])
    _ok(P.near_failures(out, prob['want'], T.mix_bound(prob, dtype, prob['want']), 'out'), f'weighted {shape} {dtype}')
    if dk > 128:                      # the fused dC takes d_k <= 128; wider senses go through the alpha-rebuilding route
        return
    like = torch.empty(1, 1, 1, d, device=DEV, dtype=dtype)
    dc = bp.sense_mix_dc(qk, prob['dout'].to(dtype), _rows_lse_in(prob['lse']), prob['scale'], like)
    full = T.full_senses(prob)[:, None, :, None]
    _ok(P.near_failures(dc, prob['want_dc'], T.mix_bound(prob, dtype, prob['want_dc'], own_lse=False), 'dc')
        + _sum_failures(torch.where(full, dc.double(), 0.0), torch.where(full, prob['want_dc'], 0.0), dtype, 'dc of the full-block senses'),
        f'dc {shape} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('d', [64, 128])
def test_flash_bwd_with_own_block_and_flat_rows(d, dtype):
    """flash_bwd on the nine maps of FWD_MAPS, S = 257 and 641: the 16-bit O handed in is the rounding of sum / n, D = dO . O
    follows it (tie_blocks.grad_bounds adds P |D16 - D|), the rebuilt P = 1 / n is rounded for dV: dV within tie_blocks.mix_bound
    (bit for bit in the slots of the full-block maps), dQ and dK within grad_bounds."""
    bp = _bp()
    for tag, prob in T.fixed_problems(dict(d=d, seqlens=[257, 641]), T.FWD_MAPS, dtype, DEV):
        b, sq, h, _ = prob['q'].shape
        q, k, v, dout = (prob[x].to(dtype).reshape(-1, h, d) for x in ('q', 'k', 'v', 'dout'))
        out, lse = prob['want'].to(dtype).reshape(-1, h, d), _rows_lse_in(prob['lse'])
        dq, dk, dv = torch.full_like(q, NAN), torch.full_like(k, NAN), torch.full_like(v, NAN)
        bp.flash_bwd(dout, q, k, v, out, lse, dq, dk, dv, None, None, sq, sq, prob['scale'], True)
        bq, bk = T.grad_bounds(prob, dtype, T.p_error(d))
        full = torch.tensor([T.parse(m)[0] in ('full', 'early') for m in prob['maps']], device=DEV).view(b, 1, h, 1)
        dv = dv.view(b, sq, h, d)
        _ok(P.near_failures(dv, prob['want_dv'], T.mix_bound(prob, dtype, prob['want_dv'], own_lse=False), 'dv')
            + T.mean_failures(torch.where(full, dv.double(), 0.0), torch.where(full, prob['want_dv'], 0.0), dtype, 'dv of the full-block slots', rel=0.0)
            + P.near_failures(dq.view(b, sq, h, d), prob['want_dq'], bq, 'dq') + P.near_failures(dk.view(b, sq, h, d), prob['want_dk'], bk, 'dk'),
            f'{tag} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_sense_mix_varlen_with_own_block_and_flat_senses(dtype):
    """The packed batch with the nine maps of FWD_MAPS over the senses: out within tie_blocks.mix_bound, every LSE."""
    bp = _bp()
    c = T.MIX_VARLEN
    prob = T.sense_varlen_problem(c['lens'], c['k'], c['dk'], c['dout'], DEV, maps=T.FWD_MAPS)
    top = max(c['lens'])
    qk, content = prob['qk'].to(dtype), prob['content'].to(dtype)
    lse = bp.sense_lse_varlen(qk, prob['cu'], top, prob['scale'])
    out = torch.full((qk.shape[0], c['dout']), NAN, device=DEV, dtype=dtype)
    bp.sense_mix_varlen(qk, content, prob['cu'], top, prob['scale'], out=out, lse=lse)
    bound = torch.cat([T.mix_bound(part, dtype, part['want'])[0] for part in prob['parts']])
    bad = P.near_failures(out, prob['want'], bound, 'out')
    for n, (length, part) in enumerate(zip(c['lens'], prob['parts'])):
        bad += T.lse_failures(lse[n, :, :length], part['lse'][0], f'LSE of sequence {n}')
    _ok(bad, f'varlen {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', T.DECODE_CASES[:2], ids=[f"d{c['d']}-{c['regime']}" for c in T.DECODE_CASES[:2]])
def test_flash_decode_flat_rows_at_any_length(case, dtype):
    """Flat rows (all active splits weigh by their key counts) and cut own blocks where the tie count is NO power of two, L = 64,
    65, 1000, 2047, 64 and 8 splits: the combine's fp32 roundings leave what tie_blocks.decode_bound derives; the LSE = ln n
    within the decode tolerance counts the keys."""
    bp = _bp()
    b, h, d, ms = case['batch'], case['heads'], case['d'], case['max_seqlen']
    nsplit = min(-(-512 // (b * h)), -(-ms // 64), 64)
    cache = torch.full((b, ms, 2, h, d), NAN, device=DEV, dtype=dtype)
    for L in T.DECODE_FLAT_LENGTHS:
        prob = T.decode_problem(case, L, dtype, DEV, maps=T.DECODE_FLAT_MAPS)
        cache[:, :L, 0], cache[:, :L, 1] = prob['keys'][:, :L].to(dtype), prob['vals'][:, :L].to(dtype)
        cache[:, L:] = NAN
        k_new, v_new = prob['keys'][:, L].to(dtype).contiguous(), prob['vals'][:, L].to(dtype).contiguous()
        seqlens = torch.full((b,), L, dtype=torch.int32, device=DEV)
        out, lse = bp.flash_decode(prob['q'].to(dtype), k_new, v_new, cache, seqlens, prob['scale'], return_lse=True)
        _ok(P.near_failures(out, prob['want'], T.decode_bound(prob, dtype, nsplit), 'out') + T.lse_failures(lse, prob['lse']),
            f"{case['regime']} L={L} {dtype}")


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('d', [64, 128])
def test_flash_bwd_exact_dq_dk_where_every_intermediate_is_representable(d, dtype):
    """Full blocks of order 1 ... 7, one per slot, and a dO with a single 1 per row, S = 129, 257, 641: dS = 2^-m (V[j, c] - O[c])
    is short, and in the slots where dS, scale dS and the closed forms of dQ and dK are representable (tie_blocks.exact_grad_slots:
    m <= 3 in fp16, m <= 2, at the short lengths 3, in bf16; beyond that a sum over 2^m keys of (m + 2)-bit terms needs more bits
    than the dtype has) dQ and dK are held bit for bit; dV bit for bit and the bounds of grad_bounds in every slot."""
    bp = _bp()
    exact = 0
    for s in (129, 257, 641):
        b, h = P.bh_of(s)
        for maps in T.EXACT_GRAD_MAPS:
            prob = T.attn_problem(maps, b, h, s, s, d, dtype, DEV, sparse=True)
            q, k, v, dout = (prob[x].to(dtype).reshape(-1, h, d) for x in ('q', 'k', 'v', 'dout'))
            out, lse = prob['want'].to(dtype).reshape(-1, h, d), _rows_lse_in(prob['lse'])
            dq, dk, dv = torch.full_like(q, NAN), torch.full_like(k, NAN), torch.full_like(v, NAN)
            bp.flash_bwd(dout, q, k, v, out, lse, dq, dk, dv, None, None, s, s, prob['scale'], True)
            dq, dk, dv = (g.view(b, s, h, d) for g in (dq, dk, dv))
            slots = T.exact_grad_slots(prob, dtype)[:, None, :, None]
            exact += int(slots.sum())
            zq, zk = (P.GRAD_DUST + P.FP32_SUM * prob[x] for x in ('abs_dq', 'abs_dk'))
            _ok(_grad_failures(dq, dk, dv, prob, dtype, d)
                + P.exact_failures(torch.where(slots, dq.double(), 0.0), torch.where(slots, prob['want_dq'], 0.0), dtype, 'dq (exact slots)', zq)
                + P.exact_failures(torch.where(slots, dk.double(), 0.0), torch.where(slots, prob['want_dk'], 0.0), dtype, 'dk (exact slots)', zk),
                f'd={d} S={s} {maps} {dtype}')
    assert exact >= 6


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('maps', [T.BWD_MAPS, T.FWD_MAPS], ids=['full', 'mixed'])
@pytest.mark.parametrize('shape', T.MIX_DQK, ids=lambda s: 'x'.join(map(str, s)))
def test_sense_dqk_is_its_closed_form_within_its_rounding(shape, maps, dtype):
    """bp.sense_dqk with the closed-form LSE and a dO with a single 1 per row (dP = a content value, exact in the 16-bit slab), on
    full-block senses and on the nine maps of FWD_MAPS (own-block and flat senses too): dq and dk within tie_blocks.dqk_forms'
    bounds of scale sum dS k and scale sum dS q, dS = P (dP - D)."""
    prob = T.sense_problem(*shape, device=DEV, maps=maps, sparse=True, pad=True)
    want, bq, bk, _ = T.dqk_forms(prob, dtype)
    dqk = _bp().sense_dqk(prob['qk'].to(dtype), prob['content'].to(dtype), prob['dout'].to(dtype), _rows_lse_in(prob['lse']), prob['scale'])
    _ok(P.near_failures(dqk[:, :, 0], want[:, :, 0], bq, 'dq') + P.near_failures(dqk[:, :, 1], want[:, :, 1], bk, 'dk'), f'{shape} {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_wide_route_dqk_is_its_closed_form_within_its_rounding(dtype):
    """dqk of bp.sense_mix_autograd at d_k = 160 (_sense_mix_backward_rebuild: sense_alpha from the forward's LSE, BLAS products,
    softmax_bwd_causal_) on full-block senses with a single 1 per dO row: within tie_blocks.rebuild_dqk_bounds of the fp64 closed
    form -- one 16-bit rounding of dS, fp32 sums, one rounding of the result; out and dcontent bit for bit as with the dense dO."""
    bp = _bp()
    prob = T.sense_problem(*T.MIX_WIDE_AUTOGRAD, device=DEV, sparse=True)
    want, bq, bk = T.rebuild_dqk_bounds(prob, dtype)
    qk, content = prob['qk'].to(dtype).requires_grad_(), prob['content'].to(dtype).requires_grad_()
    out = bp.sense_mix_autograd(qk, content, prob['scale'])
    out.backward(prob['dout'].to(dtype))
    _ok(_sum_failures(out.detach(), prob['want'], dtype, 'out') + _sum_failures(content.grad, prob['want_dc'], dtype, 'dcontent')
        + P.near_failures(qk.grad[:, :, 0], want[:, :, 0], bq, 'dq') + P.near_failures(qk.grad[:, :, 1], want[:, :, 1], bk, 'dk'), f'wide {dtype}')
