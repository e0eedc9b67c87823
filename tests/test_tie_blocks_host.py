"""CPU: the tie problems of tests/tie_blocks.py do what tests/test_gpu_tie_blocks.py relies on.  For every case that file runs
(the case lists are the same objects):

  * the construction: the fp32 scores tie bit for bit on exactly the keys of the dense P, every other visible key is 48 nats
    or more below, in both dtypes and for every map;
  * an fp32 model of the forward as the kernels order it (online softmax over 64-key tiles, P rounded to 16 bit, one division
    at the end) and plain fp64 autograd meet every criterion the GPU file applies;
  * the two conditions: a call excuses at most 10 % of its rows from bit equality (a full-block row never), and the LSE
    tolerance is at most half of ln(1 + 1 / n) on every row, so n and n +- 1 are told apart;
  * the expected full-block results are representable (out) or single roundings of exact fp32 sums (dV);
  * named mutants of the model FAIL the criteria on every call with three or more key tiles: a kept tile's row sum counted
    twice, its P V dropped, one 16-key group of it with p = 0, its value rows taken from the same positions of the next tile,
    one query tile's term missing from dV / dK, the D of the neighbouring row, and (decode) a split with another split's weight;
  * the same for the sense problems (the mix, dC, sense_dqk, sense_decode), for the 1 / n rows held to derived bounds, and for the
    slots whose dQ and dK are owed bit for bit.

Every row of every case; value columns: the first COLS.
"""
import pytest
import torch

import prefill_needles as P
import tie_blocks as T

DTYPES = (torch.bfloat16, torch.float16)
INF = float('inf')
COLS = 16                                   # value columns on the host: the eight coded ones and eight hashed ones


def _scores(prob, dt=torch.float32):
    s = prob['scale'] * torch.einsum('bthd,bshd->bhts', prob['q'].to(dt), prob['k'].to(dt))
    if prob['causal']:
        s = s.masked_fill(torch.triu(torch.ones(s.shape[-2:], dtype=torch.bool), 1), -INF)
    return s


def _tiled(prob, dtype, mutant=None, tile=1):
    """fp32 forward over 64-key tiles: running maximum, P = exp(s - m) rounded to `dtype`, l and O accumulated in fp32,
    O / l at the end -> out (b, t, h, w), lse (b, h, t).  Mutants act on key tile `tile` for the rows from 64 (tile + 1) on, for
    which it is unmasked."""
    s = _scores(prob)
    v = prob['v'].float()
    b, h, sq, sk = s.shape
    late = (torch.arange(sq) >= 64 * (tile + 1))[None, None, :]
    m = torch.full((b, h, sq), -INF)
    l = torch.zeros(b, h, sq)
    acc = torch.zeros(b, h, sq, v.shape[-1])
    for t in range(-(-sk // 64)):
        x = s[..., 64 * t:64 * t + 64]
        vt = v[:, 64 * t:64 * t + 64]
        m_new = torch.maximum(m, x.max(dim=-1).values)
        alpha = torch.where(m_new == m, 1.0, torch.exp(m - m_new)).nan_to_num(nan=0.0)
        p = torch.exp(x - m_new[..., None]).nan_to_num(nan=0.0).to(dtype).float()
        hit = late if t == tile else torch.zeros_like(late)
        if mutant == 'group0':
            p = torch.where(hit[..., None] & ((torch.arange(x.shape[-1]) // 16) == 1), 0.0, p)
        rs = p.sum(-1)
        if mutant == 'sum2':
            rs = torch.where(hit, 2 * rs, rs)
        if mutant == 'neighbour' and t == tile:
            nb = v[:, 64 * (t + 1):64 * (t + 1) + 64]
            vt_m = torch.cat([nb, vt[:, nb.shape[1]:]], dim=1)
            pv = torch.where(hit[..., None], torch.einsum('bhts,bshw->bhtw', p, vt_m), torch.einsum('bhts,bshw->bhtw', p, vt))
        else:
            pv = torch.einsum('bhts,bshw->bhtw', p, vt)
        if mutant == 'nopv':
            pv = torch.where(hit[..., None], 0.0, pv)
        l = l * alpha + rs
        acc = acc * alpha[..., None] + pv
        m = m_new
    return (acc * (1.0 / l)[..., None]).permute(0, 2, 1, 3), m + torch.log(l)


def _fwd_failures(out, lse, prob, dtype):
    return T.mean_failures(out, prob['want'], dtype, 'out', T.zero_out(prob)) + T.lse_failures(lse, prob['lse'])


def _fwd_calls(dtype, ragged=True):
    for case in T.FLASH_FWD_CASES:
        yield from T.fixed_problems(case, T.FWD_MAPS, dtype, cols=min(COLS, case['d']))
    for c in T.FLASH_CROSS:
        yield from T.cross_problems(c, dtype, cols=COLS)
    for tag, rag in T.ragged_problems(dtype, cols=COLS) if ragged else ():
        for n, part in enumerate(rag['parts']):
            yield f'{tag} sequence {n}', part


def _full_rows(prob):
    """bool (b, t, h): rows of the slots whose map is a full-block one."""
    b, h = prob['p'].shape[:2]
    full = torch.tensor([T.parse(m)[0] in ('full', 'early', 'head') for m in prob['maps']]).view(b, 1, h)
    return full.expand(b, prob['p'].shape[2], h)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_construction_ties_and_gaps(dtype):
    """Tied keys == the dense P's support, bit for bit in fp32; the best other visible key is >= 48 nats below; widths 8 ... 128
    of the cases plus the sense widths 10 (padded to 16), 24, 48, 160, 640 at S = 641 (width 8, 10: the longest they can code)."""
    calls = 0
    for tag, prob in _fwd_calls(dtype):
        s = _scores(prob)
        top = s.max(dim=-1, keepdim=True).values
        tied = s == top
        assert torch.equal(tied, prob['p'] > 0), tag
        assert torch.equal(tied.sum(-1), prob['n']), tag
        rest = s.masked_fill(tied, -INF).max(dim=-1, keepdim=True).values
        assert float((top - rest).min()) >= 48.0, tag
        calls += 1
    assert calls > 40
    for width, s in ((10, 641), (24, 641), (48, 641), (160, 641), (640, 641), (80, 641), (40, 641)):
        for name in T.FWD_MAPS:
            if s - 1 + T.parse(name)[2] > T.max_length(width):
                continue
            pos, m, base, n = T.rows_of(name, s, s, width)
            q = T.tie_query(pos, m, width, -(-width // 8) * 8)
            k = T.code(torch.arange(s) + T.parse(name)[2], width, -(-width // 8) * 8)
            sc = (q @ k.T).masked_fill(torch.triu(torch.ones(s, s, dtype=torch.bool), 1), -INF)      # integer dot products
            top = sc.max(dim=-1, keepdim=True).values
            assert torch.equal(sc == top, T.dense_p(base, n, s) > 0), (width, name)
            gap = float((top - sc.masked_fill(sc == top, -INF).max(dim=-1, keepdim=True).values).min())
            assert gap >= 2 * T.reps(width) and 2 * T.reps(width) * T.scale(width) == 48.0, (width, name)
            assert torch.equal(top[:, 0].long(), T.reps(width) * (min(width, 16) - m)), (width, name)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_forward_model_meets_the_criteria_and_the_conditions_hold(dtype):
    worst_share, worst_res = 0.0, 0.0
    for tag, prob in _fwd_calls(dtype):
        out, lse = _tiled(prob, dtype)
        assert not _fwd_failures(out, lse, prob, dtype), (tag, _fwd_failures(out, lse, prob, dtype))
        s64 = _scores(prob, torch.float64)
        out64 = torch.einsum('bhts,bshw->bthw', torch.softmax(s64, -1), prob['v'].double())
        near = ((out64 - prob['want']).abs() <= 1e-13 * (1 + prob['abs_want'])).all()
        assert near and not T.lse_failures(torch.logsumexp(s64, -1), prob['lse']), tag
        amb = T.ambiguous_rows(prob['want'], dtype)
        full = _full_rows(prob)
        assert not (amb & full).any(), f'{tag}: a full-block row is excused'
        assert torch.equal(prob['want'][full].to(dtype).double(), prob['want'][full]), f'{tag}: a block mean is not representable'
        share = float(amb.double().mean())
        assert share <= 0.10, (tag, share)
        res = T.lse_resolution(prob)
        assert res <= 0.5, (tag, res)
        worst_share, worst_res = max(worst_share, share), max(worst_res, res)
    print(f'{dtype}: largest share of excused rows {worst_share:.3f}, largest LSE tolerance / ln(1 + 1 / n) {worst_res:.3f}')


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('mutant', ['sum2', 'nopv', 'group0', 'neighbour'])
def test_forward_mutants_fail_on_every_call_with_three_key_tiles(mutant, dtype):
    """The mutant acts on key tile 1 for the rows from 128 on (a kept tile: neither their first nor their diagonal one)."""
    seen = 0
    for tag, prob in _fwd_calls(dtype, ragged=False):
        if prob['p'].shape[-1] <= 128 or (prob['causal'] and prob['p'].shape[-2] <= 128):
            continue
        out, lse = _tiled(prob, dtype, mutant)
        assert _fwd_failures(out, lse, prob, dtype), f'{tag}: mutant {mutant} passes'
        seen += 1
    assert seen > 30
    for tag, rag in T.ragged_problems(dtype, cols=COLS):             # one call: its 257-key sequence has the kept tile
        assert any(_fwd_failures(*_tiled(part, dtype, mutant), part, dtype) for part in rag['parts']), f'{tag}: mutant {mutant} passes'


# ---- backward ---------------------------------------------------------------------------------------------------------------

def _bwd_calls(dtype):
    for case in T.FLASH_BWD_CASES:
        yield from T.fixed_problems(case, T.BWD_MAPS, dtype, cols=COLS)
    yield from T.cross_problems(T.FLASH_CROSS[1], dtype, cols=COLS, maps=T.BWD_MAPS)
    for tag, rag in T.ragged_problems(dtype, cols=COLS, maps=T.BWD_MAPS):
        for n, part in enumerate(rag['parts']):
            if part is not None:
                yield f'{tag} sequence {n}', part


def _bwd_model(prob, dtype, e=0.0, drop_tile=None, shift_d=False):
    """fp64 model of the backward: P = (1 + e) 2^-m rebuilt from the LSE and rounded to `dtype` for dV, dS = P (dP - D) rounded
    to `dtype` for dQ and dK.  drop_tile: query rows 64 t ... 64 t + 63 contribute nothing to dV and dK; shift_d: row i takes the
    D of row i + 1."""
    p = prob['p'] * (1 + e)
    q, k, v, do = (prob[x].double() for x in ('q', 'k', 'v', 'dout'))
    dd = (do * prob['want'].to(dtype).double()).sum(-1).permute(0, 2, 1)
    if shift_d:
        dd = torch.cat([dd[..., 1:], dd[..., -1:]], dim=-1)
    ds = (p * (torch.einsum('bthw,bshw->bhts', do, v) - dd[..., None])).to(dtype).double()
    p16 = p.to(dtype).double()
    if drop_tile is not None:
        ds[:, :, 64 * drop_tile:64 * drop_tile + 64] = 0
        p16[:, :, 64 * drop_tile:64 * drop_tile + 64] = 0
    return (prob['scale'] * torch.einsum('bhts,bshd->bthd', ds, k), prob['scale'] * torch.einsum('bhts,bthd->bshd', ds, q),
            torch.einsum('bhts,bthw->bshw', p16, do))


def _bwd_failures(grads, prob, dtype):
    bq, bk = T.grad_bounds(prob, dtype, T.p_error(prob['q'].shape[-1]))
    return (T.mean_failures(grads[2], prob['want_dv'], dtype, 'dv', rel=0.0) + P.near_failures(grads[0], prob['want_dq'], bq, 'dq')
            + P.near_failures(grads[1], prob['want_dk'], bk, 'dk'))


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_backward_closed_forms_and_mutants(dtype):
    """fp64 autograd == the closed forms; the kernels' model with P off by +-p_error stays inside the criteria; the expected dV
    is an exact fp32 number (a multiple of 2^-7 below 2^17); a dropped query tile and a neighbour's D fail on every call with
    three or more tiles."""
    for tag, prob in _bwd_calls(dtype):
        q, k, v = (prob[x].double().requires_grad_() for x in ('q', 'k', 'v'))
        s = prob['scale'] * torch.einsum('bthd,bshd->bhts', q, k)
        if prob['causal']:
            s = s.masked_fill(torch.triu(torch.ones(s.shape[-2:], dtype=torch.bool), 1), -INF)
        out = torch.einsum('bhts,bshw->bthw', torch.softmax(s, -1), v)
        grads = torch.autograd.grad(out, (q, k, v), prob['dout'].double())
        for g, name in zip(grads, ('want_dq', 'want_dk', 'want_dv')):
            assert float((g - prob[name]).abs().max()) <= 1e-9, (tag, name)
        assert torch.equal(prob['want_dv'].float().double(), prob['want_dv']) and torch.equal(prob['want_dv'] * 128, (prob['want_dv'] * 128).round())
        e = T.p_error(prob['q'].shape[-1])
        assert e < P.HALF_ULP[torch.float16] / 2
        for err in (0.0, e, -e):
            bad = _bwd_failures(_bwd_model(prob, dtype, err), prob, dtype)
            assert not bad, (tag, err, bad)
        sq = prob['p'].shape[-2]
        if sq > 128:
            bad = _bwd_failures(_bwd_model(prob, dtype, drop_tile=2), prob, dtype)
            assert any(x.startswith('dv') for x in bad) and any(x.startswith('dk') for x in bad), (tag, bad)
            bad = _bwd_failures(_bwd_model(prob, dtype, shift_d=True), prob, dtype)
            assert any(x.startswith('dq') for x in bad), (tag, bad)


def test_probability_criterion():
    """1 / n rounded from (1 +- p_error) / n: a power of two is never ambiguous; of 641 flat rows few are (the issue measured 4 in
    bf16, 44 in fp16 at 2e-5); a probability matrix rolled by one key fails."""
    for dtype in DTYPES:
        prob = T.attn_problem(('flat', 'full7', 'own6'), 1, 3, 641, 641, 64, dtype, cols=8)
        e = T.p_error(64)
        assert e < P.HALF_ULP[torch.float16] / 2
        assert float(T.row_p_error(prob).max()) <= e
        lo, hi = T.candidates(prob['p'], dtype, T.row_p_error(prob))
        amb = (lo != hi).any(-1)
        assert not amb[0, 1].any() and float(amb.double().mean()) <= 0.10      # of the call's 3 * 641 rows
        p16 = prob['p'].to(dtype)
        assert not T.probs_failures(p16, prob, dtype, 'ref', T.row_p_error(prob))
        assert T.probs_failures(p16.roll(1, dims=-1), prob, dtype, 'ref', T.row_p_error(prob))
        for causal, maps in ((True, T.FWD_MAPS), (False, T.CROSS_MAPS)):               # the calls of test_attn_probs_from_a_given_lse
            for sk in T.PROBS_SK:
                prob = T.attn_problem(P.slot_maps(maps, 3, sk), 1, 3, sk, sk, 64, dtype, causal=causal, cols=8)
                lo, hi = T.candidates(prob['p'], dtype, T.row_p_error(prob))
                assert float((lo != hi).any(-1).double().mean()) <= 0.10, (sk, causal)
                assert not T.probs_failures(prob['p'].to(dtype), prob, dtype, 'ref', T.row_p_error(prob))


# ---- decode -------------------------------------------------------------------------------------------------------------------

def _split_combine(prob, nsplit, mutant=None):
    """fp32 model of csrc/decode_core.h: per split m, l = sum exp2(x - m), acc = sum p v; combine with w_s = exp2(m_s - M) / lsum.
    mutants: 'first': split 1 takes the weight of split 0; 'shift': every split that of its predecessor."""
    s = (prob['scale'] * P.LOG2E) * torch.einsum('bhd,bshd->bhs', prob['q'], prob['keys'])
    n = s.shape[-1]
    chunk = -(-n // nsplit)
    nact = -(-n // chunk)
    s = torch.nn.functional.pad(s, (0, nact * chunk - n), value=-INF).view(*s.shape[:2], nact, chunk)
    v = torch.nn.functional.pad(prob['vals'].permute(0, 2, 1, 3), (0, 0, 0, nact * chunk - n)).reshape(*s.shape[:2], nact, chunk, -1)
    m = s.max(-1).values
    p = torch.exp2(s - m[..., None])
    l, acc = p.sum(-1), torch.einsum('bhcs,bhcsw->bhcw', p, v)
    big = m.max(-1, keepdim=True).values
    e = torch.exp2(m - big)
    lsum = (l * e).sum(-1, keepdim=True)
    w = e * (1.0 / lsum)
    if mutant == 'first' and nact > 1:
        w[..., 1] = w[..., 0]
    if mutant == 'shift' and nact > 1:
        w = w.roll(1, dims=-1)
    return (w[..., None] * acc).sum(-2), (big[..., 0] + torch.log2(lsum[..., 0])) * P.LN2


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_decode_model_meets_the_criterion_and_a_wrong_split_weight_does_not(dtype):
    """Every case of the GPU test: construction, the fp32 split-and-combine model bit for bit, nothing excused (rel = 0), LSE
    resolution, every expected result one rounding of an exact fp32 number; split 1 with split 0's weight, and every split with
    its predecessor's, fail at every length in the regimes that have a second split (the 'head0' row keeps all its weight in
    split 0)."""
    for case in T.DECODE_CASES:
        nsplit = min(-(-512 // (case['batch'] * case['heads'])), -(-case['max_seqlen'] // 64), 64)
        for L in T.DECODE_LENGTHS:
            prob = T.decode_problem(case, L, dtype, cols=COLS)
            s = prob['scale'] * torch.einsum('bhd,bshd->bhs', prob['q'], prob['keys'])
            top = s.max(-1, keepdim=True).values
            assert torch.equal(s == top, prob['p'] > 0) and float((top - s.masked_fill(s == top, -INF).max(-1, keepdim=True).values).min()) >= 48.0
            assert T.lse_resolution(prob) <= 0.5
            assert torch.equal(prob['want'].float().double(), prob['want'])
            assert ((prob['n'] & (prob['n'] - 1)) == 0).all(), 'a tie count that is no power of two'
            out, lse = _split_combine(prob, nsplit)
            bad = T.mean_failures(out, prob['want'], dtype, 'out', T.zero_out(prob), rel=0.0) + T.lse_failures(lse, prob['lse'])
            assert not bad, (case['regime'], L, bad)
            for mutant in ('first', 'shift') if nsplit > 1 else ():
                out, lse = _split_combine(prob, nsplit, mutant=mutant)
                assert T.mean_failures(out, prob['want'], dtype, 'out', T.zero_out(prob), rel=0.0), (case['regime'], L, mutant, 'passes')


# ---- sense kernels ------------------------------------------------------------------------------------------------------------

def _sense_model(prob, dtype, zero=None):
    """fp32 model of the mix and of dC: P = exp2(s c2 - fl(lse log2e)) from the fp32 LSE of the scores, rounded to `dtype`;
    out = sum_l P_l (w C_l), dC_l = P_l^T dout.  zero: (tile, key in tile) whose P is 0 for the rows behind that tile (a register
    of the accumulating step) -> out (b, t, w), dc (b, s, k, w), lse (b, k, t)."""
    q, k = prob['qk'][:, :, 0].float(), prob['qk'][:, :, 1].float()
    s = torch.einsum('btld,bsld->blts', q, k)
    n = s.shape[-1]
    mask = torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
    lse = torch.logsumexp((prob['scale'] * s).masked_fill(mask, -INF), dim=-1)
    c2 = torch.tensor(prob['scale'], dtype=torch.float32) * torch.tensor(P.LOG2E, dtype=torch.float32)
    pr = torch.exp2(s * c2 - (lse * torch.tensor(P.LOG2E, dtype=torch.float32))[..., None]).masked_fill(mask, 0.0).to(dtype).float()
    if zero is not None:
        pr[:, :, 64 * (zero[0] + 1):, 64 * zero[0] + zero[1]] = 0.0
    content = prob['content'].float()
    pw = pr if prob['key_weight'] is None else pr * prob['key_weight'][:, :, None, :]
    return torch.einsum('blts,bslw->btw', pw, content), torch.einsum('blts,btw->bslw', pr, prob['dout'].float()), lse


def _sense_calls():
    for shape in T.MIX_SHAPES + [T.MIX_STAGED] + T.MIX_DC + [T.MIX_WIDE_AUTOGRAD]:
        yield str(shape), T.sense_problem(*shape, cols=COLS, pad=True)
    for shape in T.MIX_GATHER:
        yield f'gather {shape}', T.sense_problem(*shape, cols=COLS, form='gather')
    for shape in T.MIX_WEIGHTED:
        yield f'weighted {shape}', T.sense_problem(*shape, cols=COLS, weighted=True, pad=True)
    c = T.MIX_VARLEN
    for n, part in enumerate(T.sense_varlen_problem(c['lens'], c['k'], c['dk'], c['dout'], cols=COLS)['parts']):
        yield f'varlen sequence {n}', part


def _sum(got, want, dtype, name):
    return T.mean_failures(got, want, dtype, name, rel=0.0)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_sense_model_meets_the_criteria_and_a_zeroed_register_does_not(dtype):
    """Every full-block sense case of the GPU file (the same list objects): all tie counts powers of two; want and want_dc exact
    fp32 numbers, multiples of 2^-8 -- with key_weight = 1/2 too --, so nothing is excused; the LSE tolerance resolves n; the
    fp32 model gives the expected bits for out and dC and an LSE inside the tolerance; with one key of tile 1 at P = 0 for the
    rows from 128 on, out and dC fail wherever the problem has such rows."""
    for tag, prob in _sense_calls():
        assert T.full_senses(prob).all(), tag
        for name in ('want', 'want_dc'):
            assert torch.equal(prob[name].float().double(), prob[name]) and torch.equal(prob[name] * 256, (prob[name] * 256).round()), (tag, name)
        assert T.lse_resolution(prob) <= 0.5, tag
        assert T.lse_error(prob) + float(T.row_p_error(prob).max()) < P.HALF_ULP[dtype], tag
        out, dc, lse = _sense_model(prob, dtype)
        bad = _sum(out, prob['want'], dtype, 'out') + _sum(dc, prob['want_dc'], dtype, 'dc') + T.lse_failures(lse, prob['lse'])
        assert not bad, (tag, bad)
        if prob['p'].shape[-1] > 128:
            live = prob['p'][:, :, 128:, 64 + 43] > 0                              # (b, k, rows) that weigh the zeroed key
            out, dc, _ = _sense_model(prob, dtype, zero=(1, 43))
            if live.any():
                assert _sum(dc, prob['want_dc'], dtype, 'dc'), (tag, 'the zeroed register passes dC')
                kw = prob['key_weight']
                if kw is None or (live & (kw[:, :, 64 + 43] > 0)[..., None]).any():   # (a key of weight 0 is legitimately unseen)
                    assert _sum(out, prob['want'], dtype, 'out'), (tag, 'the zeroed register passes the mix')


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_mixed_sense_model_stays_inside_its_bound(dtype):
    """MIX_MIXED and ALPHA_CASES (own-block and flat senses next to full-block ones): the fp32 model inside tie_blocks.mix_bound
    for out and dC, the full-block senses' dC bit for bit, the LSE condition, at most 10 % of the alpha rows excused; a flat
    sense's key zeroed fails dC where its row is short enough for the bound (the docstring of mix_bound says how short)."""
    for shape in T.MIX_MIXED:
        prob = T.sense_problem(*shape, cols=COLS, maps=T.FWD_MAPS)
        assert not T.full_senses(prob).all() and T.full_senses(prob).any() and T.lse_resolution(prob) <= 0.5
        out, dc, lse = _sense_model(prob, dtype)
        full = T.full_senses(prob)[:, None, :, None]
        bad = (P.near_failures(out, prob['want'], T.mix_bound(prob, dtype, prob['want']), 'out')
               + P.near_failures(dc, prob['want_dc'], T.mix_bound(prob, dtype, prob['want_dc']), 'dc')
               + _sum(torch.where(full, dc.double(), 0.0), torch.where(full, prob['want_dc'], 0.0), dtype, 'dc of the full-block senses')
               + T.lse_failures(lse, prob['lse']))
        assert not bad, (shape, bad)
        out, dc, _ = _sense_model(prob, dtype, zero=(1, 43))
        assert P.near_failures(dc, prob['want_dc'], T.mix_bound(prob, dtype, prob['want_dc']), 'dc'), (shape, 'mutant passes')
    for s, k, dk in T.ALPHA_CASES:
        prob = T.sense_problem(s, k, dk, 8, maps=T.FWD_MAPS, pad=True)
        lo, hi = T.candidates(prob['p'], dtype, T.row_p_error(prob))
        assert float((lo != hi).any(-1).double().mean()) <= 0.10 and T.lse_resolution(prob) <= 0.5, (s, k, dk)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_sense_decode_model(dtype):
    """Every sense_decode case, table and cache form, weighted: ties, power-of-two counts, an exact fp32 want, and the fp32
    split-and-combine model (senses as heads, summed) bit for bit; split 1 with split 0's weight fails."""
    for case in T.SENSE_DECODE_CASES:
        nsplit = min(-(-512 // (case['batch'] * case['k'])), -(-case['max_seqlen'] // 64), 64)
        for L in T.DECODE_LENGTHS:
            for form in ('table', 'cache'):
                prob = T.sense_decode_problem(case, L, form, weighted=(form == 'table'), cols=COLS)
                s = prob['scale'] * torch.einsum('bld,bsld->bls', prob['q'], prob['keys'])
                assert torch.equal(s == s.max(-1, keepdim=True).values, prob['p'] > 0) and ((prob['n'] & (prob['n'] - 1)) == 0).all()
                assert torch.equal(prob['want'].float().double(), prob['want'])
                model = dict(q=prob['q'], keys=prob['keys'], vals=prob['vals'], scale=prob['scale'])
                out, _ = _split_combine(model, nsplit)
                assert not _sum(out.sum(1), prob['want'], dtype, 'out'), (case, L, form)
                chunk = -(-(L + 1) // nsplit)
                kw = prob['key_weight']
                # the 'head0' sense keeps its weight on key 0: seen unless that key, or all of split 1 for that sense, has weight 0
                head = [r for r in range(case['batch'] * case['k']) if prob['maps'][r % len(prob['maps'])] == 'head0']
                seen = kw is None or any(kw[r // case['k'], r % case['k'], 0] > 0 and (kw[r // case['k'], r % case['k'], chunk:2 * chunk] > 0).any()
                                         for r in head)
                if seen and L + 1 > chunk:
                    out, _ = _split_combine(model, nsplit, mutant='first')
                    assert _sum(out.sum(1), prob['want'], dtype, 'out'), (case, L, form, 'mutant passes')


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_backward_model_with_own_block_and_flat_rows(dtype):
    """test_flash_bwd_with_own_block_and_flat_rows: the model (P off by +-p_error and rounded for dV, D from the 16-bit O, dS
    rounded) inside mix_bound for dV and grad_bounds for dQ, dK, bit for bit on dV in the full-block slots; a dropped query tile
    fails dV and dK, a neighbour's D fails dQ."""
    for d in (64, 128):
        for tag, prob in T.fixed_problems(dict(d=d, seqlens=[257, 641]), T.FWD_MAPS, dtype, cols=COLS):
            b, h = prob['p'].shape[:2]
            full = torch.tensor([T.parse(m)[0] in ('full', 'early') for m in prob['maps']]).view(b, 1, h, 1)
            bq, bk = T.grad_bounds(prob, dtype, T.p_error(d))
            bv = T.mix_bound(prob, dtype, prob['want_dv'], own_lse=False)

            def failures(g):
                return (P.near_failures(g[2], prob['want_dv'], bv, 'dv')
                        + T.mean_failures(torch.where(full, g[2], 0.0), torch.where(full, prob['want_dv'], 0.0), dtype, 'dv full', rel=0.0)
                        + P.near_failures(g[0], prob['want_dq'], bq, 'dq') + P.near_failures(g[1], prob['want_dk'], bk, 'dk'))
            e = T.p_error(d)
            for err in (0.0, e, -e):
                assert not failures(_bwd_model(prob, dtype, err)), (tag, err, failures(_bwd_model(prob, dtype, err)))
            bad = failures(_bwd_model(prob, dtype, drop_tile=2))
            assert any(x.startswith('dv') for x in bad) and any(x.startswith('dk') for x in bad), (tag, bad)
            assert any(x.startswith('dq') for x in failures(_bwd_model(prob, dtype, shift_d=True))), tag


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_decode_flat_rows_at_any_length(dtype):
    """test_flash_decode_flat_rows_at_any_length: the fp32 split-and-combine model inside decode_bound, the LSE condition, and
    split 1 with split 0's weight outside the bound wherever a full-block row keeps the two apart (L >= 1000)."""
    for case in T.DECODE_CASES[:2]:
        nsplit = min(-(-512 // (case['batch'] * case['heads'])), -(-case['max_seqlen'] // 64), 64)
        for L in T.DECODE_FLAT_LENGTHS:
            prob = T.decode_problem(case, L, dtype, cols=COLS, maps=T.DECODE_FLAT_MAPS)
            assert T.lse_resolution(prob) <= 0.5
            out, lse = _split_combine(prob, nsplit)
            bound = T.decode_bound(prob, dtype, nsplit)
            assert not P.near_failures(out, prob['want'], bound, 'out') + T.lse_failures(lse, prob['lse']), (case['regime'], L)
            out, _ = _split_combine(prob, nsplit, mutant='shift')
            assert P.near_failures(out, prob['want'], bound, 'out'), (case['regime'], L, 'mutant passes')


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_exact_grad_slots(dtype):
    """test_flash_bwd_exact_dq_dk_where_every_intermediate_is_representable: in the slots exact_grad_slots names the kernels'
    model (P off by +-p_error, dS rounded once) returns the closed forms of dQ and dK bit for bit; orders 1 and 2 are always
    among them, no order above 3 ever; a neighbour's D fails there."""
    for d in (64, 128):
        for s in (129, 257, 641):
            b, h = P.bh_of(s)
            for maps in T.EXACT_GRAD_MAPS:
                prob = T.attn_problem(maps, b, h, s, s, d, dtype, sparse=True)
                slots = T.exact_grad_slots(prob, dtype)
                orders = [T.parse(m)[1] for m in maps]
                for ok, m in zip(slots.flatten().tolist(), orders):
                    assert ok or m > 2, (d, s, m)
                    assert not ok or m <= 3, (d, s, m)
                sl = slots[:, None, :, None]

                def failures(g):
                    return (P.exact_failures(torch.where(sl, g[0], 0.0), torch.where(sl, prob['want_dq'], 0.0), dtype, 'dq', P.GRAD_DUST)
                            + P.exact_failures(torch.where(sl, g[1], 0.0), torch.where(sl, prob['want_dk'], 0.0), dtype, 'dk', P.GRAD_DUST)
                            + _bwd_failures(g, prob, dtype))
                e = T.p_error(d)
                for err in (0.0, e, -e):
                    assert not failures(_bwd_model(prob, dtype, err)), (d, s, maps, err)
                if slots.any():
                    assert any(x.startswith('dq') for x in failures(_bwd_model(prob, dtype, shift_d=True))), (d, s, maps)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_sense_dqk_forms_and_bounds(dtype):
    """MIX_DQK, full-block senses and the nine maps of FWD_MAPS: the closed forms == fp64 autograd of the mix; a model with P off by +-E, D = (1 +- E) sum P dP and dS rounded to
    16 bit stays inside the bounds; row t with the D of row t + 1 does not (dq and dk)."""
    for shape, maps in [(shape, maps) for shape in T.MIX_DQK for maps in (T.BWD_MAPS, T.FWD_MAPS)]:
        prob = T.sense_problem(*shape, maps=maps, sparse=True, pad=True)
        want, bq, bk, ds = T.dqk_forms(prob, dtype)
        qk = prob['qk'].double().requires_grad_()
        s = prob['scale'] * torch.einsum('btld,bsld->blts', qk[:, :, 0], qk[:, :, 1])
        s = s.masked_fill(torch.triu(torch.ones(s.shape[-2:], dtype=torch.bool), 1), -INF)
        out = torch.einsum('blts,bslw->btw', torch.softmax(s, -1), prob['content'].double())
        grad, = torch.autograd.grad(out, qk, prob['dout'].double())
        assert float((grad - want).abs().max()) <= 1e-9, shape
        e = float(T.row_p_error(prob).max())
        q, key, p = prob['qk'][:, :, 0].double(), prob['qk'][:, :, 1].double(), prob['p']
        dp = torch.einsum('btw,bslw->blts', prob['dout'].double(), prob['content'].double())

        def model(pe, de, shift=False):
            dd = (p * dp).sum(-1) * (1 + de)
            if shift:
                dd = torch.cat([dd[..., 1:], dd[..., -1:]], dim=-1)
            d16 = (p * (1 + pe) * (dp - dd[..., None])).to(dtype).double()
            return (prob['scale'] * torch.einsum('blts,bsld->btld', d16, key)).to(dtype), (prob['scale'] * torch.einsum('blts,btld->bsld', d16, q)).to(dtype)
        for pe in (0.0, e, -e):
            for de in (0.0, e, -e):
                dq, dk = model(pe, de)
                bad = P.near_failures(dq, want[:, :, 0], bq, 'dq') + P.near_failures(dk, want[:, :, 1], bk, 'dk')
                assert not bad, (shape, pe, de, bad)
        dq, dk = model(0.0, 0.0, shift=True)
        assert P.near_failures(dq, want[:, :, 0], bq, 'dq') and P.near_failures(dk, want[:, :, 1], bk, 'dk'), (shape, 'mutant passes')


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_rebuild_route_dqk_bounds(dtype):
    """test_wide_route_dqk_is_its_closed_form_within_its_rounding: alpha rebuilt from the forward's own LSE rounds to 2^-m; the
    route's model in its own order -- 16-bit alpha and dalpha, fp32 D, dS = fl(fl(scale) alpha (dalpha - D)) rounded to 16 bit,
    fp32 products with k and q, 16-bit results -- stays inside rebuild_dqk_bounds; with the D of row t + 1 it does not."""
    prob = T.sense_problem(*T.MIX_WIDE_AUTOGRAD, sparse=True)
    assert T.full_senses(prob).all() and T.lse_error(prob) + float(T.row_p_error(prob).max()) < P.HALF_ULP[dtype]
    want, bq, bk = T.rebuild_dqk_bounds(prob, dtype)
    alpha = prob['p'].to(dtype).float()
    assert torch.equal(alpha.double(), prob['p'])
    dalpha = torch.einsum('btw,bslw->blts', prob['dout'].to(dtype).float(), prob['content'].to(dtype).float())
    assert torch.equal(dalpha.to(dtype).float(), dalpha)
    q, key = prob['qk'][:, :, 0].float(), prob['qk'][:, :, 1].float()
    scale = torch.tensor(prob['scale'], dtype=torch.float32)

    def model(shift=False):
        dd = (alpha * dalpha).sum(-1)
        if shift:
            dd = torch.cat([dd[..., 1:], dd[..., -1:]], dim=-1)
        ds = ((scale * alpha) * (dalpha - dd[..., None])).to(dtype).float()
        return torch.einsum('blts,bsld->btld', ds, key).to(dtype), torch.einsum('blts,btld->bsld', ds, q).to(dtype)
    dq, dk = model()
    bad = P.near_failures(dq, want[:, :, 0], bq, 'dq') + P.near_failures(dk, want[:, :, 1], bk, 'dk')
    assert not bad, bad
    dq, dk = model(shift=True)
    assert P.near_failures(dq, want[:, :, 0], bq, 'dq') and P.near_failures(dk, want[:, :, 1], bk, 'dk'), 'mutant passes'
