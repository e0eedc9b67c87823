"""CPU: the inputs of tests/test_gpu_prefill_needles.py (tests/prefill_needles.py) do what that file relies on, as
test_needle_construction_is_exact_in_fp32 (tests/test_kv_cache_host.py) shows for the decode needles: for every collected
case a plain fp32 reference gives exactly the expected bits, its fp64 autograd the expected gradients under the criteria
the GPU tests apply -- and three mutants of the reference (a dropped key, a key counted twice, row i + 1's D for row i)
FAIL those criteria, which is the proof that the GPU tests can fail.

Subsampling, to stay under half a minute: value / content / gradient COLUMNS are the first 32 (exactness rests on the
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
