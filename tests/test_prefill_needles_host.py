"""CPU: the inputs of tests/test_gpu_prefill_needles.py (tests/prefill_needles.py) do what that file relies on, as
test_needle_construction_is_exact_in_fp32 (tests/test_kv_cache_host.py) shows for the decode needles: for every collected
case a plain fp32 reference gives exactly the expected bits, its fp64 autograd the expected gradients under the criteria
the GPU tests apply -- and three mutants of the reference (a dropped key, a key counted twice, row i + 1's D for row i)
FAIL those criteria, which is the proof that the GPU tests can fail.

The pair problems (two needles per row, second half) get the same proof for their non-zero gradients: P == 1/2 in fp32,
fp64 autograd == the closed forms, every expected tensor representable, the kernels' fp64 models inside the GPU criteria for
every row reference and P off by +-pair_p_error, nine mutants outside them, and the coverage conditions.  They keep all
columns (representability is a property of the whole row).

Subsampling of the single-needle part, to stay under half a minute: value / content / gradient COLUMNS are the first 32 (exactness rests on the
score gap and on integers, not on the column; sense_dqk, whose sparse dout spreads over all columns, keeps them all);
every ROW of every case is checked."""
import pytest
import torch

import prefill_needles as P

DTYPES = (torch.bfloat16, torch.float16)
INF = float('inf')


def _representable(want, dtype, tag):
    assert torch.equal(want.to(dtype).double(), want.double()), f'{tag}: expected result not representable in {dtype}'


# ---- references ----------------------------------------------------------------------------------------------------------

def _scores(prob, causal, dt, drop=None):
    s = prob['scale'] * torch.einsum('bthd,bshd->bhts', prob['q'].to(dt), prob['k'].to(dt))
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(s.shape[-2:], dtype=torch.bool), 1), -INF)
    if drop is not None:
        s = s.clone()
        s[..., drop] = -INF
    return s


def _attend(prob, causal, dt=torch.float32, drop=None, dup=None, v=None):
    """Plain softmax attention -> out (b, sq, h, w), lse (b, h, sq).  drop: key j is masked out; dup: key j counts twice."""
    s = _scores(prob, causal, dt, drop)
    v = prob['v'].to(dt) if v is None else v
    if dup is not None:
        s = torch.cat([s, s[..., dup:dup + 1]], dim=-1)
        v = torch.cat([v, v[:, dup:dup + 1]], dim=1)
    return torch.einsum('bhts,bshw->bthw', torch.softmax(s, dim=-1), v), torch.logsumexp(s.float(), dim=-1)


def _attend_bwd_model(prob, causal, drop=None, dup=None, shift_d=False):
    """fp64 backward as the kernels order it: P rebuilt from the saved LSE (the needle score), dS = P (dP - D).  The three
    mutants: key `drop` contributes nothing, key `dup` twice, row i takes D of row i + 1 (the last row its own)."""
    dt = torch.float64
    p = torch.exp(_scores(prob, causal, dt, drop) - prob['lse'])
    if dup is not None:
        p[..., dup] *= 2
    q, k, v, do = (prob[x].to(dt) for x in ('q', 'k', 'v', 'dout'))
    dsum = (do * prob['want'].to(dt)).sum(-1).permute(0, 2, 1)                         # (b, h, sq)
    if shift_d:
        dsum = torch.cat([dsum[..., 1:], dsum[..., -1:]], dim=-1)
    ds = p * (torch.einsum('bthw,bshw->bhts', do, v) - dsum[..., None])
    return (prob['scale'] * torch.einsum('bhts,bshd->bthd', ds, k), prob['scale'] * torch.einsum('bhts,bthd->bshd', ds, q),
            torch.einsum('bhts,bthw->bshw', p, do))


def _bwd_failures(grads, prob, dtype):
    dq, dk, dv = grads
    return (P.grad_failures(dv, prob['want_dv'], prob['fan'], dtype, 'dv') + P.dust_failures(dq, P.GRAD_DUST, 'dq')
            + P.dust_failures(dk, P.GRAD_DUST, 'dk'))


def _check_forward(prob, causal, tag, lse_tol=P.LSE_TOL, dtypes=DTYPES):
    out, lse = _attend(prob, causal)
    for dtype in dtypes:
        _representable(prob['want'], dtype, tag)
        assert not P.flash_failures(out, lse.permute(0, 2, 1), prob, dtype, lse_tol), (tag, dtype)


def _check_backward(prob, causal, tag):
    q, k, v = (prob[x].double().requires_grad_() for x in ('q', 'k', 'v'))
    out, _ = _attend(dict(prob, q=q, k=k), causal, torch.float64, v=v)
    grads = torch.autograd.grad(out, (q, k, v), prob['dout'].double())
    model = _attend_bwd_model(prob, causal)
    for dtype in DTYPES:
        _representable(prob['want_dv'], dtype, tag)
        assert not _bwd_failures(grads, prob, dtype), (tag, dtype, _bwd_failures(grads, prob, dtype))
        assert not _bwd_failures(model, prob, dtype), (tag, dtype, 'model')


def _fixed(maps, s, d, rot, bh=None, **kw):
    b, h = bh or P.bh_of(s)
    return P.attn_problem(P.slot_maps(maps, b * h, rot), b, h, s, s, d, cols=min(d, 32), **kw)


# ---- attention -----------------------------------------------------------------------------------------------------------

def test_flash_forward_needles_are_exact_in_fp32():
    """Every case of the forward test: out.to(dtype) == V[j*] and the fp32 LSE within the decode tolerance, all rows."""
    checked = 0
    for case in P.FLASH_FWD_CASES:
        for s in case['seqlens']:
            for rot in P.rotations(P.FWD_MAPS, 3):
                _check_forward(_fixed(P.FWD_MAPS, s, case['d'], rot), True, (case['d'], s, rot))
                checked += 3 * s
    c = P.FLASH_BH9
    _check_forward(_fixed(P.FWD_MAPS, c['s'], c['d'], 0, (c['b'], c['h'])), True, 'bh9')
    c = P.FLASH_CROSS
    for causal, maps in ((True, P.FWD_MAPS), (False, P.CROSS_MAPS + P.FWD_MAPS)):
        for rot in P.rotations(maps, 3):
            prob = P.attn_problem(P.slot_maps(maps, 3, rot), c['b'], c['h'], c['sq'], c['sk'], c['d'], cols=32)
            _check_forward(prob, causal, ('cross', causal, rot))
    c = P.FLASH_RAGGED
    for rot in P.rotations(P.FWD_MAPS, c['h']):
        for part in P.ragged_problem(c['lens'], c['h'], c['d'], P.FWD_MAPS, rot, cols=32)['parts']:
            _check_forward(part, True, ('ragged', rot))
    assert checked > 50000


def test_flash_stale_reference_case_is_exact_in_bf16():
    """FLASH_STALE at its full S = 641: with softmax_scale = 9 / reps the fp32 reference still rounds to V[j*] in bf16 (the
    other keys weigh < 641 e^-18 = 1e-5 of the needle, far under half a bf16 ulp), and the needle's p against the best key of
    the row's first tile lies between the fp16 and the bf16 limit of the steady-state body."""
    c = P.FLASH_STALE
    prob = P.attn_problem([P.STALE_MAP] * 3, c['b'], c['h'], c['s'], c['s'], c['d'], scale_num=c['scale_num'], cols=32)
    _check_forward(prob, True, 'stale', P.STALE_LSE_TOL, dtypes=(torch.bfloat16,))
    s = _scores(prob, True, torch.float64)[..., 128:, :]
    p = torch.exp(s.max(dim=-1).values - s[..., :64].max(dim=-1).values)
    assert 2.0 ** 14 < float(p.min()) and float(p.max()) < 2.0 ** 30
    assert torch.equal(s.argmax(dim=-1), prob['js'][..., 128:]) and int(prob['js'][..., 128:].min()) >= 64


def test_flash_backward_needles_are_exact():
    """Every case of the backward test: the fp64 autograd gradients and the LSE-rebuilding model of the kernels give
    dV == the fan-in sums (representable in both dtypes), |dV| <= 1e-12 without a fan-in, |dQ|, |dK| <= 1e-6."""
    for case in P.FLASH_BWD_CASES:
        for s in case['seqlens']:
            for rot in P.rotations(P.BWD_MAPS, 3):
                _check_backward(_fixed(P.BWD_MAPS, s, case['d'], rot), True, (case['d'], s, rot))
    c = P.FLASH_CROSS
    for rot in P.rotations(P.CROSS_MAPS + P.BWD_MAPS, 3):
        prob = P.attn_problem(P.slot_maps(P.CROSS_MAPS + P.BWD_MAPS, 3, rot), c['b'], c['h'], c['sq'], c['sk'], c['d'], cols=32)
        _check_backward(prob, False, ('cross', rot))
    c = P.FLASH_BWD_RAGGED
    for rot in P.rotations(P.BWD_MAPS, c['h']):
        for part in P.ragged_problem(c['lens'], c['h'], c['d'], P.BWD_MAPS, rot, cols=32)['parts']:
            _check_backward(part, True, ('ragged', rot))


@pytest.mark.parametrize('s,d', [(385, 64), (641, 80), (129, 16)])
def test_flash_mutants_fail_the_gpu_criteria(s, d):
    """Drop the needle of the last row / count it twice / give row i the D of row i + 1: the forward criterion (bits, LSE)
    and the backward criterion (dV bits, dust bounds) each notice."""
    prob = _fixed(P.BWD_MAPS, s, d, 0)
    j = int(prob['js'][0, 0, -1])
    for dtype in DTYPES:
        assert not P.flash_failures(*_lse_last(_attend(prob, True)), prob, dtype)
        drop = P.flash_failures(*_lse_last(_attend(prob, True, drop=j)), prob, dtype)
        assert any('differ' in x for x in drop), drop
        dup = P.flash_failures(*_lse_last(_attend(prob, True, dup=j)), prob, dtype)
        assert any('LSE' in x for x in dup), dup
        assert any(x.startswith('dv') for x in _bwd_failures(_attend_bwd_model(prob, True, drop=j), prob, dtype))
        assert any(x.startswith('dv') for x in _bwd_failures(_attend_bwd_model(prob, True, dup=j), prob, dtype))
        shifted = _bwd_failures(_attend_bwd_model(prob, True, shift_d=True), prob, dtype)
        assert any(x.startswith('dq') for x in shifted) and any(x.startswith('dk') for x in shifted), shifted


def _lse_last(out_lse):
    return out_lse[0], out_lse[1].permute(0, 2, 1)


def test_probability_criterion_on_the_reference():
    """softmax of the needle scores in fp32, rounded: 1.0 at the needles, 0 where masked, <= 2e-21 elsewhere; a needle moved
    by one key fails."""
    for sk in P.PROBS_SK:
        for causal, sq in ((True, sk), (False, sk), (False, P.PROBS_CROSS_SQ), (True, P.PROBS_CROSS_SQ)):
            maps = P.FWD_MAPS if causal else P.CROSS_MAPS + P.FWD_MAPS
            prob = P.attn_problem(P.slot_maps(maps, 3, sk), 1, 3, sq, sk, 64, cols=8)
            p = torch.softmax(_scores(prob, causal, torch.float32), dim=-1)
            for dtype in DTYPES:
                assert not P.probs_failures(p.to(dtype), prob['js'], causal, 'ref')
            if sq > 1:
                assert P.probs_failures(p.roll(1, dims=-1).to(torch.bfloat16), prob['js'], causal, 'ref')
    for width in (10, 16, 24, 40, 48, 64, 80, 128, 160, 640):
        # a kernel that rebuilds P from the saved LSE gets 1 - e in fp32: it must round to 1.0 in fp16 as well
        assert P.needle_p_error(width) < P.HALF_ULP[torch.float16]


# ---- sense mix -----------------------------------------------------------------------------------------------------------

def _mix_p(prob, dt, drop=None, dup=None, from_lse=False):
    """alpha (b, k, t, s) of a sense problem.  drop / dup: (sense, key)."""
    q, k = prob['qk'][:, :, 0].to(dt), prob['qk'][:, :, 1].to(dt)
    s = prob['scale'] * torch.einsum('btld,bsld->blts', q, k)
    s = s.masked_fill(torch.triu(torch.ones(s.shape[-2:], dtype=torch.bool), 1), -INF)
    if drop is not None:
        s[:, drop[0], :, drop[1]] = -INF
    p = torch.exp(s - prob['lse']) if from_lse else torch.softmax(s, dim=-1)
    if dup is not None:
        p = p.clone()
        p[:, dup[0], :, dup[1]] *= 2
    return p, torch.logsumexp(s.float(), dim=-1)


def _mix(prob, dt=torch.float32, content=None, **mut):
    p, lse = _mix_p(prob, dt, **mut)
    if prob['key_weight'] is not None:
        p = p * prob['key_weight'].to(dt)[:, :, None, :]
    return torch.einsum('blts,bslw->btw', p, prob['content'].to(dt) if content is None else content), lse


def _mix_failures(out, lse, prob, dtype):
    return P.flash_failures(out, lse, prob, dtype)


def _mix_cases():
    for shape in P.MIX_NARROW + [P.MIX_STAGED] + P.MIX_WIDE:
        yield shape, {}
    for shape in P.MIX_GATHER:
        yield shape, dict(form='gather')
    yield P.MIX_WEIGHTED, dict(weighted=True)


def test_sense_mix_needles_are_exact_in_fp32():
    """Every forward sense case: the fp32 mix gives sum_l C[j*_l(t), l, :] bit for bit, a sum representable in both dtypes,
    and the LSE of every (sense, row) is the needle score; a dropped needle changes bits, a doubled one the LSE-free sum."""
    for shape, kw in _mix_cases():
        prob = P.sense_problem(*shape, cols=32, **kw)
        out, lse = _mix(prob)
        for dtype in DTYPES:
            _representable(prob['want'], dtype, (shape, kw))
            assert not _mix_failures(out, lse, prob, dtype), (shape, kw, dtype)
        assert int(prob['want'].min()) >= 1 and float(prob['content'].max()) <= P.value_cap(shape[1])
    prob = P.sense_problem(*P.MIX_NARROW[1], cols=32)
    l, j = 3, int(prob['js'][0, 3, -1])
    for dtype in DTYPES:
        assert any('differ' in x for x in _mix_failures(*_mix(prob, drop=(l, j)), prob, dtype))
        assert any('differ' in x for x in _mix_failures(*_mix(prob, from_lse=True, dup=(l, j)), prob, dtype))


def test_sense_dc_needles_are_exact():
    """Every sense_mix_dc case: fp64 autograd and the LSE-rebuilding model give dC == the fan-in sums of dout (representable),
    <= 1e-12 without a fan-in; the drop and twice mutants fail."""
    for shape in P.MIX_DC:
        prob = P.sense_problem(*shape, maps=P.BWD_MAPS, cols=32, pad=True)
        c = prob['content'].double().requires_grad_()
        out, _ = _mix(prob, torch.float64, content=c)
        truth, = torch.autograd.grad(out, c, prob['dout'].double())
        model = torch.einsum('blts,btw->bslw', _mix_p(prob, torch.float64, from_lse=True)[0], prob['dout'].double())
        l, j = 1, int(prob['js'][0, 1, -1])
        mutants = [torch.einsum('blts,btw->bslw', _mix_p(prob, torch.float64, from_lse=True, **m)[0], prob['dout'].double())
                   for m in (dict(drop=(l, j)), dict(dup=(l, j)))]
        for dtype in DTYPES:
            _representable(prob['want_dc'], dtype, shape)
            for got in (truth, model):
                assert not P.grad_failures(got, prob['want_dc'], prob['fan'], dtype, 'dc'), (shape, dtype)
            for got in mutants:
                assert P.grad_failures(got, prob['want_dc'], prob['fan'], dtype, 'dc'), (shape, dtype)


def _dqk_model(prob, dtype, r_of, e, shift_d=False):
    """fp64 model of bp.sense_dqk's arithmetic on a needle problem (prefill_needles.dqk_bounds): only the needle of a row
    has weight; its probability is 1 - e, the row reference r = r_of(dP of the row's visible keys) rounded to 16 bit, and
    g_n is rounded to 16 bit before the product with k.  -> dq (b, t, k, dk), dk (b, s, k, dk)."""
    qk = prob['qk'].double()
    dp = torch.einsum('btw,bslw->blts', prob['dout'].double(), prob['content'].double())
    causal = torch.tril(torch.ones(dp.shape[-2:], dtype=torch.bool))
    dp_n = torch.gather(dp, 3, prob['js'][..., None])[..., 0]                               # (b, k, t)
    r = r_of(dp, causal).to(dtype).double()
    p_n = 1.0 - e
    g_n = p_n * (dp_n - r)
    d_row = g_n + r * p_n                                                                    # D as the kernel forms it
    d_used = torch.cat([d_row[..., 1:], d_row[..., -1:]], dim=-1) if shift_d else d_row
    k_n = torch.gather(qk[:, :, 1].permute(0, 2, 1, 3), 2, prob['js'][..., None].expand(*prob['js'].shape, qk.shape[-1]))  # (b, k, t, dk)
    dq = prob['scale'] * (g_n.to(dtype).double() - (d_used - r)) [..., None] * k_n          # A1 - (D - r) A2, A2 = k_n
    ds_n = (p_n * (dp_n - d_used)).to(dtype).double()                                        # the dk kernel's 16-bit dS
    dk, _ = P.fan_in(prob['js'], (ds_n[..., None] * qk[:, :, 0].permute(0, 2, 1, 3)).permute(0, 2, 1, 3), dp.shape[-1])
    return dq.permute(0, 2, 1, 3), prob['scale'] * dk


def test_sense_dqk_bounds_hold_for_the_model_and_fail_for_a_shifted_d():
    """bp.sense_dqk keeps |dqk| <= 1e-6 only where the needle's rebuilt probability is exactly 1 and dP_n - r is a 16-bit
    number; prefill_needles.dqk_bounds derives what its arithmetic can legitimately leave.  Here: the fp64 truth (autograd)
    is dust; the model stays inside the bounds for r = min, max and mean of the row's dP and e = +-needle_p_error; with row
    i + 1's D for row i it leaves them; dP is an integer <= 64, so the 16-bit slab is exact."""
    for shape in P.MIX_DQK:
        prob = P.sense_problem(*shape, maps=P.BWD_MAPS, sparse=True, pad=True)
        assert int((prob['dout'] != 0).sum(-1).max()) <= 4 and float(prob['dout'].max()) <= 2
        qk = prob['qk'].double().requires_grad_()
        out, _ = _mix(dict(prob, qk=qk), torch.float64)
        truth, = torch.autograd.grad(out, qk, prob['dout'].double())
        assert float(truth.abs().max()) <= 1e-12
        e = P.needle_p_error(prob['dk'], prob['scale'])
        inf = torch.tensor(INF, dtype=torch.float64)
        refs = (lambda dp, m: torch.where(m, dp, inf).min(-1).values, lambda dp, m: torch.where(m, dp, -inf).max(-1).values,
                lambda dp, m: (dp * m).sum(-1) / m.sum(-1))
        for dtype in DTYPES:
            bound_q, bound_k = P.dqk_bounds(prob, dtype)
            for r_of in refs:
                for err in (e, -e, 0.0):
                    dq, dk = _dqk_model(prob, dtype, r_of, err)
                    assert not P.dust_failures(dq, bound_q, 'dq') + P.dust_failures(dk, bound_k, 'dk'), (shape, dtype, err)
            dq, dk = _dqk_model(prob, dtype, refs[2], e, shift_d=True)
            assert P.dust_failures(dq, bound_q, 'dq') and P.dust_failures(dk, bound_k, 'dk'), (shape, dtype)


# ---- two needles per row: the non-zero arithmetic of dQ, dK, dqk ---------------------------------------------------------------

def _r16(x, dtype):
    return x.to(dtype).double()


def _pair_dense(prob, causal, dtype, e=0.0, route='flash', shift_d=False, half=0.5):
    """fp64 model of a backward that rebuilds P from the saved LSE, dense over (row, key), with the 16-bit roundings of
    route 'flash' (csrc/flash_bwd.hip: D = dO . O from the given O, P and dS = P (dP - D) rounded for the products) or
    'rebuild' (_sense_mix_backward_rebuild: sense_alpha to 16 bit, the 16-bit dP of the GEMM, softmax_bwd_causal_ with its fp32
    row sum and scale inside dS, 16-bit GEMM outputs).  Every probability is off by the factor 1 + e.  q, k (b, s, g, d), v,
    dout (b, s, g, w), lse (b, g, t) -> dict of p16, ds (b, g, t, s; scale NOT applied) and dq, dk, dv."""
    dt = torch.float64
    q, k, v, do = (prob[x].to(dt) for x in ('q', 'k', 'v', 'dout'))
    s = prob['scale'] * torch.einsum('btgd,bsgd->bgts', q, k)
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(s.shape[-2:], dtype=torch.bool), 1), -INF)
    p = torch.exp(s - prob['lse'][..., None]) * (1 + e)
    p16 = _r16(p, dtype)
    dp = torch.einsum('btgw,bsgw->bgts', do, v)
    if route == 'flash':
        dsum = (do * prob['want'].to(dt)).sum(-1).permute(0, 2, 1)
        src = p
    else:
        dp = _r16(dp, dtype)
        dsum = (p16 * dp).sum(-1)
        src = p16
    if shift_d:
        dsum = torch.cat([dsum[..., 1:], dsum[..., -1:]], dim=-1)
    ds = _r16(src * (dp - dsum[..., None]), dtype)
    return dict(p16=p16, ds=ds, dp=dp, dsum=dsum, q=q, k=k, do=do, scale=prob['scale'],
                dq=prob['scale'] * torch.einsum('bgts,bsgd->btgd', ds, k), dk=prob['scale'] * torch.einsum('bgts,btgd->bsgd', ds, q),
                dv=torch.einsum('bgts,btgw->bsgw', p16, do))


def _pair_dense_failures(m, prob, dtype):
    return (P.exact_failures(m['dq'], prob['want_dq'], dtype, 'dq', prob['zero_dq']) + P.exact_failures(m['dk'], prob['want_dk'], dtype, 'dk', prob['zero_dk'])
            + P.exact_failures(m['dv'], prob['want_dv'], dtype, 'dv', P.DUST))


def _victim(prob, tile):
    """(sample, slot, row, needle key, rows of the row's query tile / slab) of the mutants: the last row with n != 0."""
    n = prob['n']                                                    # (b, t, g)
    b, i, g = (n != 0).nonzero()[-1].tolist()
    return b, g, i, int(prob['js'][b, g, i]), slice(i - i % tile, min(i - i % tile + tile, n.shape[1]))


def _pair_dense_mutants(m, prob, dtype, tile=64):
    """The mutants of the dense model -> (name, model).  All but the last touch dK alone."""
    b, g, i, j, rows = _victim(prob, tile)
    sc = m['scale']
    one = sc * m['ds'][b, g, i, j] * m['q'][b, i, g]                                             # row i's term of dK[j]
    keys = slice(j - j % 64, j - j % 64 + 64)
    block = sc * torch.einsum('ts,td->sd', m['ds'][b, g, rows], m['q'][b, rows, g])              # the query tile's term of every dK
    jj = j - 1 if j >= 1 else j + 1

    def with_dk(delta_at, delta):
        dk = m['dk'].clone()
        for at, d in zip(delta_at, delta):
            dk[b, at, g] += d
        return dict(m, dk=dk)
    yield 'one contribution dropped', with_dk([j], [-one])
    yield 'one contribution twice', with_dk([j], [one])
    yield 'one contribution to the neighbouring key', with_dk([j, jj], [-one, one])
    yield 'a query tile dropped', with_dk([slice(None)], [-block])
    yield 'scale twice in one tile', with_dk([keys], [(sc - 1) * block[keys]])
    yield 'no scale in one tile', with_dk([keys], [(1 / sc - 1) * block[keys]])
    # P = 1 instead of 1/2 at (i, j): dS there doubles, dV[j] takes the whole dO row
    new = _r16(1.0 * (m['dp'][b, g, i, j] - m['dsum'][b, g, i]), dtype) - m['ds'][b, g, i, j]
    dq, dv = m['dq'].clone(), m['dv'].clone()
    dq[b, i, g] += sc * new * m['k'][b, j, g]
    dv[b, j, g] += (1.0 - m['p16'][b, g, i, j]) * m['do'][b, i, g]
    yield 'P = 1 at one needle', dict(with_dk([j], [sc * new * m['q'][b, i, g]]), dq=dq, dv=dv)


def _pair_forward_and_truth(prob, causal, dtypes, tag):
    """The fp32 softmax gives P == 1/2 at both needles and the forward rows bit for bit; fp64 autograd the closed forms;
    every expected tensor is representable."""
    s = prob['scale'] * torch.einsum('btgd,bsgd->bgts', prob['q'], prob['k'])
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(s.shape[-2:], dtype=torch.bool), 1), -INF)
    p = torch.softmax(s, dim=-1)
    paired = prob['js2'] != prob['js']
    at1, at2 = torch.gather(p, 3, prob['js'][..., None])[..., 0], torch.gather(p, 3, prob['js2'][..., None])[..., 0]
    assert torch.equal(at1, torch.where(paired, 0.5, 1.0).float()) and torch.equal(at2[paired], at1[paired]), tag
    rest = p.scatter(3, prob['js'][..., None], 0.0).scatter(3, prob['js2'][..., None], 0.0)
    assert float(rest.max()) < 1e-20, tag
    out = torch.einsum('bgts,bsgw->btgw', p, prob['v'])
    assert not P.exact_failures(out, prob['want'], torch.float32, 'out'), (tag, 'the fp32 forward is not the closed form bit for bit')
    assert not P.lse_failures(torch.logsumexp(s, dim=-1), prob['lse']), tag
    for dtype in dtypes:
        assert not P.exact_failures(out, prob['want'], dtype, 'out'), (tag, dtype)
    q, k, v = (prob[x].double().requires_grad_() for x in ('q', 'k', 'v'))
    s = prob['scale'] * torch.einsum('btgd,bsgd->bgts', q, k)
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(s.shape[-2:], dtype=torch.bool), 1), -INF)
    out = torch.einsum('bgts,bsgw->btgw', torch.softmax(s, dim=-1), v)
    grads = torch.autograd.grad(out, (q, k, v), prob['dout'].double())
    for got, name in zip(grads, ('want_dq', 'want_dk', 'want_dv')):
        assert float((got - prob[name]).abs().max()) <= 1e-12, (tag, name)
    for name in ('want', 'want_dq', 'want_dk', 'want_dv'):
        assert torch.equal(prob[name].float().double(), prob[name]), (tag, name)
        for dtype in dtypes:
            _representable(prob[name], dtype, (tag, name))


def _pair_coverage(js, js2, n, s, tag):
    """The coverage conditions of a case with S >= 129: all its (sample, slot) pairs, over every map rotation (row 256 of
    S = 257 reaches key 256 under diag and tile0 only).  js, js2 (b, g, t), n (b, t, g), or lists of them."""
    if isinstance(js, list):
        js, js2, n = (torch.cat([x.reshape(-1, s) for x in xs]) for xs in (js, js2, [x.permute(0, 2, 1) for x in n]))
    paired = js2 != js
    assert paired[..., 1:].all(), (tag, 'a row >= 1 without a partner')
    assert float((n != 0).double().mean()) >= 2 / 3, (tag, 'too few rows with n != 0')
    straddle = (js // 64 != js2 // 64)[paired]
    assert float(straddle.double().mean()) >= 1 / 8, (tag, 'too few pairs across a 64-key border', float(straddle.double().mean()))
    lo, hi = torch.minimum(js, js2), torch.maximum(js, js2)
    for border in (128, 256):
        if s > border + (border == 128) * 128:
            assert ((lo < border) & (hi >= border)).any(), (tag, f'no pair across key {border}')


def _as_attn(prob):
    """A pair sense problem in the layout of an attention problem (senses as heads, dout shared by them)."""
    b, s, _, k, _ = prob['qk'].shape
    return dict(prob, zero_dq=prob['zero_dqk'][:, :, 0], zero_dk=prob['zero_dqk'][:, :, 1], q=prob['qk'][:, :, 0], k=prob['qk'][:, :, 1], v=prob['content'], dout=prob['dout'][:, :, None, :].expand(b, s, k, -1),
                want=prob['v_want'], want_dq=prob['want_dqk'][:, :, 0], want_dk=prob['want_dqk'][:, :, 1], want_dv=prob['want_dc'])


def _check_pair_attn(tag, prob, causal, dtype):
    _pair_forward_and_truth(prob, causal, (dtype,), tag)
    e = P.pair_p_error(prob['width'], prob['scale'])
    assert e < P.HALF_ULP[torch.float16] / 2
    for err in (e, -e, 0.0):
        m = _pair_dense(prob, causal, dtype, err)
        assert not _pair_dense_failures(m, prob, dtype), (tag, dtype, err, _pair_dense_failures(m, prob, dtype))
    if not (prob['n'] != 0).any():
        return 0
    for name, mutant in _pair_dense_mutants(m, prob, dtype):
        bad = _pair_dense_failures(mutant, prob, dtype)
        assert any(x.startswith('dk') for x in bad), (tag, dtype, name)
    shifted = _pair_dense_failures(_pair_dense(prob, causal, dtype, e, shift_d=True), prob, dtype)
    assert any(x.startswith('dq') for x in shifted) and any(x.startswith('dk') for x in shifted), (tag, dtype, 'D of row i + 1')
    return 1


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_pair_flash_cases_are_exact_and_their_mutants_fail(dtype):
    """Every attention pair case (fixed length, cross, ragged) of `dtype`: P == 1/2 in fp32 and the forward rows bit for bit,
    fp64 autograd == the closed forms, all of them representable, the LSE-rebuilding model with P off by +-pair_p_error
    inside the GPU criteria, every mutant outside them, and the coverage conditions."""
    done, cases = 0, {}
    for tag, prob in P.pair_fixed_problems(dtype):
        done += _check_pair_attn(tag, prob, True, dtype)
        cases.setdefault((prob['width'], prob['q'].shape[1]), []).append(prob)
    for (d, s), probs in cases.items():
        if s >= 129:
            _pair_coverage(*([x[name] for x in probs] for name in ('js', 'js2', 'n')), s, (d, s, dtype))
    for tag, prob in P.pair_cross_problems(dtype):
        done += _check_pair_attn(tag, prob, False, dtype)
        assert (prob['js2'] != prob['js']).all() and (torch.maximum(prob['js'], prob['js2']) > torch.arange(prob['q'].shape[1])).any()
    for tag, prob in P.pair_ragged_problems(dtype):
        for n, part in enumerate(prob['parts']):
            done += _check_pair_attn((tag, n), part, True, dtype)
    assert done >= 40


def test_pair_bf16_exclusions_are_the_unrepresentable_ones():
    """PAIR_BF16_LEFT_OUT is exactly the set of (map, d, S) whose expected gradients, with the map in all three slots, bf16
    cannot hold; fp16 holds every one; tile0 or prevtile_last stays in bf16 at some d >= 48 for every length."""
    found = set()
    for case in P.PAIR_BWD_CASES:
        for s in case['seqlens']:
            for m in P.BWD_MAPS:
                for dtype in DTYPES:
                    prob = P.pair_attn_problem([m] * 3, *P.bh_of(s), s, s, case['d'], **P.PAIR_MAGS[dtype])
                    ok = all(torch.equal(prob[x].to(dtype).double(), prob[x]) for x in ('want', 'want_dq', 'want_dk', 'want_dv'))
                    assert ok or dtype == torch.bfloat16, (m, case['d'], s)
                    if not ok:
                        found.add((m, case['d'], s))
    assert found == set(P.PAIR_BF16_LEFT_OUT)
    for s in P.PAIR_SEQLENS:
        assert any(m in P.pair_maps(d, torch.bfloat16, s) for m in ('tile0', 'prevtile_last') for d in (64, 80, 128))
    for shape in P.PAIR_MIX_DQK + [P.PAIR_MIX_WIDE]:
        built = {}                                                  # both dtypes take the same sense problem today
        for dtype in DTYPES:
            mags = P.PAIR_SENSE_MAGS[dtype]
            for m in P.BWD_MAPS:
                key = (m,) + tuple(sorted(mags.items()))
                if key not in built:
                    prob = P.pair_sense_problem(*shape, maps=(m,), pad=True, **mags)
                    built[key] = (prob['want_dqk'], prob['want_dc'])
            bad = tuple(m for m in P.BWD_MAPS
                        if not all(torch.equal(x.to(dtype).double(), x) for x in built[(m,) + tuple(sorted(mags.items()))]))
            assert bad == (P.PAIR_SENSE_BF16_LEFT_OUT.get(shape, ()) if dtype == torch.bfloat16 else ()), (shape, dtype, bad)
    c = P.FLASH_BWD_RAGGED
    prob = P.pair_ragged_problem(c['lens'], c['h'], c['d'], P.BWD_MAPS, 4, **P.PAIR_MAGS[torch.bfloat16])
    assert not torch.equal(prob['want_dk'].bfloat16().double(), prob['want_dk'])         # why PAIR_RAGGED_BF16_LEFT_OUT exists


def test_pair_forward_cases_are_exact_in_fp32():
    """The forward-only pair cases (flash_fwd at d = 8, 36, 64, 128; the two sense_mix shapes): P == 1/2, rows bit for bit."""
    for dtype in DTYPES:
        for tag, prob in P.pair_fixed_problems(dtype, cases=P.PAIR_FWD_CASES, mags=P.PAIR_FWD_MAGS):
            _pair_forward_only(prob, dtype, tag)
    for shape in P.PAIR_MIX_FWD:
        prob = P.pair_sense_problem(*shape, maps=P.FWD_MAPS, **P.PAIR_FWD_MAGS)
        out, lse = _mix(prob)
        assert not P.exact_failures(out, prob['want'], torch.float32, 'out'), shape
        assert not P.lse_failures(lse, prob['lse']), shape
        for dtype in DTYPES:
            _representable(prob['want'], dtype, shape)
            assert not P.exact_failures(out, prob['want'], dtype, 'out'), (shape, dtype)
        other = out.clone()
        other[0, -1] = _mix(prob, drop=(1, int(prob['js2'][0, 1, -1])))[0][0, -1]
        assert P.exact_failures(other, prob['want'], torch.float16, 'out'), shape


def _pair_forward_only(prob, dtype, tag):
    s = prob['scale'] * torch.einsum('btgd,bsgd->bgts', prob['q'], prob['k'])
    s = s.masked_fill(torch.triu(torch.ones(s.shape[-2:], dtype=torch.bool), 1), -INF)
    out = torch.einsum('bgts,bsgw->btgw', torch.softmax(s, dim=-1), prob['v'])
    assert not P.exact_failures(out, prob['want'], torch.float32, 'out'), tag
    _representable(prob['want'], dtype, tag)
    assert not P.lse_failures(torch.logsumexp(s, dim=-1), prob['lse']), tag


# ---- ... the sense backward ------------------------------------------------------------------------------------------------------

def _pair_sense(shape, dtype):
    prob = P.pair_sense_problem(*shape, maps=P.pair_sense_maps(shape, dtype), pad=True, **P.PAIR_SENSE_MAGS[dtype])
    b, s, k, w = prob['content'].shape
    forms = P._pair_closed_forms(prob['qk'][:, :, 0], prob['qk'][:, :, 1], prob['content'], prob['dout'][:, :, None, :].expand(b, s, k, w),
                                 prob['js'], prob['js2'], prob['scale'], s)
    prob['v_want'] = forms['want']
    prob['width'] = prob['dk']
    return prob


R_OF = dict(
    min=lambda dp, seen, near: torch.where(seen, dp, torch.tensor(INF, dtype=dp.dtype)).min(-1).values,
    max=lambda dp, seen, near: torch.where(seen, dp, torch.tensor(-INF, dtype=dp.dtype)).max(-1).values,
    mean=lambda dp, seen, near: (dp * seen).sum(-1) / seen.sum(-1),
    zero=lambda dp, seen, near: torch.zeros(dp.shape[:-1], dtype=dp.dtype),      # every weight of the first 32 keys underflows
    kernel=lambda dp, seen, near: near)                                           # the P-weighted mean over the first 32 keys


def _pair_dqk_model(prob, dtype, r_name, e, mutant=None):
    """fp64 model of bp.sense_dqk / sense_mix_dc on a pair problem (prefill_needles.pair_dqk_bounds): only the two needles of
    a row have weight, P = (1 + e) / 2 each (1 + e for an unpaired row); r is the 16-bit row reference; g_j = P_j (dP_j - r) is
    rounded to 16 bit for A1, not inside D; the dk kernel rounds dS = P (dP - D) with that fp32 D.  -> dq (b, t, k, dk),
    dk (b, s, k, dk), dc (b, s, k, w).  mutant: one of the names below."""
    qk = prob['qk'].double()
    q, key = qk[:, :, 0], qk[:, :, 1]
    js, js2, sc = prob['js'], prob['js2'], prob['scale']
    s = js.shape[-1]
    dp = prob['dp']
    seen = torch.tril(torch.ones(s, s, dtype=torch.bool))
    paired = js2 != js
    dp1, dp2 = torch.gather(dp, 3, js[..., None])[..., 0], torch.gather(dp, 3, js2[..., None])[..., 0]          # (b, k, t)
    p1, p2 = torch.where(paired, 0.5, 1.0) * (1 + e), torch.where(paired, 0.5, 0.0) * (1 + e)
    vb, vl, vi, vj, slab = _victim(prob, 128)
    if mutant == 'P = 1 at one needle':
        p1[vb, vl, vi] = 1.0
    # the P-weighted mean of dP over the first 32 keys: weights relative to the row's LSE
    first = sc * torch.einsum('btld,bsld->blts', q, key[:, :32])
    first = first.masked_fill(~seen[:, :32], -INF) - prob['lse'][..., None]
    wgt = torch.exp(first) * (1 + e)
    if mutant == 'P = 1 at one needle' and vj < 32:
        wgt[vb, vl, vi, vj] = 1.0
    near = (wgt * dp[..., :32]).sum(-1) / wgt.sum(-1)
    r = _r16(R_OF[r_name](dp, seen, near), dtype)
    g1, g2 = p1 * (dp1 - r), p2 * (dp2 - r)
    dsum = g1 + g2 + r * (p1 + p2)                                                      # D as the dq kernel hands it over
    if mutant == 'D of row i + 1':
        dsum = torch.cat([dsum[..., 1:], dsum[..., -1:]], dim=-1)
    k1, k2 = (P._rows_of(key, x).permute(0, 2, 1, 3) for x in (js, js2))                # (b, k, t, dk)
    a1 = _r16(g1, dtype)[..., None] * k1 + _r16(g2, dtype)[..., None] * k2
    a2 = _r16(p1, dtype)[..., None] * k1 + _r16(p2, dtype)[..., None] * k2
    dq = sc * (a1 - (dsum - r)[..., None] * a2)
    ds1, ds2 = _r16(p1 * (dp1 - dsum), dtype), _r16(p2 * (dp2 - dsum), dtype)
    js_k = js
    if mutant == 'one contribution dropped':
        ds1[vb, vl, vi] = 0.0
    elif mutant == 'one contribution twice':
        ds1[vb, vl, vi] *= 2
    elif mutant == 'one contribution to the neighbouring key':
        js_k = js.clone()
        js_k[vb, vl, vi] = vj - 1 if vj >= 1 else vj + 1
    elif mutant == 'a slab dropped':
        ds1[vb, vl, slab], ds2[vb, vl, slab] = 0.0, 0.0
    elif mutant == 'scale twice in one slab':
        ds1[vb, vl, slab] *= sc
        ds2[vb, vl, slab] *= sc
    elif mutant == 'no scale in one slab':
        ds1[vb, vl, slab] /= sc
        ds2[vb, vl, slab] /= sc
    qt = q.permute(0, 2, 1, 3)                                                          # (b, k, t, dk)
    dk = sc * (P.fan_in(js_k, (ds1[..., None] * qt).permute(0, 2, 1, 3), s)[0] + P.fan_in(js2, (ds2[..., None] * qt).permute(0, 2, 1, 3), s)[0])
    do = prob['dout'].double()[:, None]                                                 # (b, 1, t, w)
    dc = (P.fan_in(js, (_r16(p1, dtype)[..., None] * do).permute(0, 2, 1, 3), s)[0]
          + P.fan_in(js2, (_r16(p2, dtype)[..., None] * do).permute(0, 2, 1, 3), s)[0])
    return dq.permute(0, 2, 1, 3), dk, dc, r


SENSE_MUTANTS = ('one contribution dropped', 'one contribution twice', 'one contribution to the neighbouring key', 'a slab dropped',
                 'scale twice in one slab', 'no scale in one slab')


def _pair_dqk_failures(dq, dk, dc, prob, dtype, bounds):
    return (P.near_failures(dq, prob['want_dqk'][:, :, 0], bounds[0], 'dq') + P.near_failures(dk, prob['want_dqk'][:, :, 1], bounds[1], 'dk')
            + P.exact_failures(dc, prob['want_dc'], dtype, 'dc'))


@pytest.mark.parametrize('shape', P.PAIR_MIX_DQK, ids=lambda s: 'x'.join(map(str, s)))
def test_pair_sense_backward_model_stays_inside_its_bounds_and_mutants_leave(shape):
    """Every sense_dqk / sense_mix_dc pair case, both dtypes: the fp32 mix has P == 1/2, fp64 autograd gives the closed forms
    (representable), pair_dqk_bounds stays under scale / 8, the model of csrc/sense_mix_bwd.hip stays inside the GPU criteria
    for every row reference (min, max, mean of the row's dP, 0, and the kernel's own P-weighted mean over the first 32 keys)
    and P off by +-pair_p_error, and every mutant leaves them.  With the kernel's reference, the rows whose two needles both
    lie in the first 32 keys have r = (dP_1 + dP_2) / 2 exactly, and their dq is exact where it is not 0."""
    for dtype in DTYPES:
        prob = _pair_sense(shape, dtype)
        attn = _as_attn(prob)
        _pair_forward_and_truth(attn, True, (dtype,), (shape, dtype))
        s, js, js2 = shape[0], prob['js'], prob['js2']
        if s >= 129:
            _pair_coverage(js, js2, prob['n'], s, (shape, dtype))
        paired = js2 != js
        both_low, both_high = paired & (js < 32) & (js2 < 32), paired & (js >= 32) & (js2 >= 32)
        assert both_low.any() and both_high.any() and (paired & ~both_low & ~both_high).any(), shape
        prob['dp'] = torch.einsum('btw,bslw->blts', prob['dout'].double(), prob['content'].double())
        assert torch.equal(prob['dp'].to(dtype).double(), prob['dp']) and float(prob['dp'].abs().max()) <= 8     # exact in the slab
        e = P.pair_p_error(prob['dk'], prob['scale'])
        bounds = P.pair_dqk_bounds(prob, dtype)
        assert float(bounds[0].max()) < prob['scale'] / 8 and float(bounds[1].max()) < prob['scale'] / 8, (shape, dtype)
        for r_name in R_OF:
            for err in (e, -e, 0.0):
                dq, dk, dc, r = _pair_dqk_model(prob, dtype, r_name, err)
                bad = _pair_dqk_failures(dq, dk, dc, prob, dtype, bounds)
                assert not bad, (shape, dtype, r_name, err, bad)
                if r_name == 'kernel':
                    low = both_low.permute(0, 2, 1)[..., None]                         # (b, t, k, 1)
                    mean = (torch.gather(prob['dp'], 3, js[..., None]) + torch.gather(prob['dp'], 3, js2[..., None]))[..., 0] / 2
                    assert float((r - mean)[both_low].abs().max()) <= P.DUST, (shape, dtype, 'r is not exact below key 32')     # 1e-21 where the mean is 0
                    want = prob['want_dqk'][:, :, 0]
                    assert not P.exact_failures(torch.where(low, dq, want), want, dtype, 'dq', bounds[0]), (shape, dtype)
        for name in SENSE_MUTANTS + ('D of row i + 1', 'P = 1 at one needle'):
            dq, dk, dc, _ = _pair_dqk_model(prob, dtype, 'kernel', e, mutant=name)
            bad = _pair_dqk_failures(dq, dk, dc, prob, dtype, bounds)
            assert any(x.startswith('dk') for x in bad), (shape, dtype, name, bad)
            if name in ('D of row i + 1', 'P = 1 at one needle'):
                assert any(x.startswith('dq') for x in bad), (shape, dtype, name, bad)
            if name == 'P = 1 at one needle':
                assert any(x.startswith('dc') for x in bad), (shape, dtype, name, bad)


def test_pair_wide_rebuild_route_is_predicted_bit_exact():
    """PAIR_MIX_WIDE through the model of _sense_mix_backward_rebuild (sense_alpha to 16 bit, the 16-bit GEMM outputs,
    softmax_bwd_causal_): dqk and dcontent meet the exact criterion with the dust bounds for P off by +-pair_p_error, so the GPU
    test asks for bit equality; the mutants fail it."""
    for dtype in DTYPES:
        prob = _as_attn(_pair_sense(P.PAIR_MIX_WIDE, dtype))
        assert prob['scale'] == 2.0
        _pair_forward_and_truth(prob, True, (dtype,), ('wide', dtype))
        _pair_coverage(prob['js'], prob['js2'], prob['n'], P.PAIR_MIX_WIDE[0], ('wide', dtype))
        e = P.pair_p_error(prob['dk'], prob['scale'])
        for err in (e, -e, 0.0):
            m = _pair_dense(prob, True, dtype, err, route='rebuild')
            m = dict(m, dq=_r16(m['dq'], dtype), dk=_r16(m['dk'], dtype), dv=_r16(m['dv'], dtype))
            assert not _pair_dense_failures(m, prob, dtype), (dtype, err, _pair_dense_failures(m, prob, dtype))
        for name, mutant in _pair_dense_mutants(m, prob, dtype, tile=128):
            assert any(x.startswith('dk') for x in _pair_dense_failures(mutant, prob, dtype)), (dtype, name)
        shifted = _pair_dense_failures(_pair_dense(prob, True, dtype, e, route='rebuild', shift_d=True), prob, dtype)
        assert any(x.startswith('dq') for x in shifted) and any(x.startswith('dk') for x in shifted), dtype
