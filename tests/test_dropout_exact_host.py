"""CPU: the inputs of tests/test_gpu_dropout_exact.py (tests/dropout_exact.py) do what that file relies on -- a plain fp32 /
fp64 reference of every problem meets every criterion the GPU tests apply, and eight mutants of the reference do NOT, which is
the proof that the GPU tests can fail:

  the mask        shifted by one key | shifted by one run of 4 columns | rows and columns swapped | the stream of the
                  neighbouring head | offset >> 32 ignored                    (against the read-outs and the LayerNorm mask)
  the arithmetic  Z applied to D as well, dS = P Z (dP - D) | Z missing from dV | the row sum taken after the mask
                                                                                      (against the pair problems)

It also holds what the problems promise: every visible P of a read-out is far above the dtype's smallest normal number, the
two-rounding fp32 model of every read-out stays within 2 u, the p = 1e-6 cases drop something, every closed form of a pair
problem is representable in its dtype (dropout_exact.PAIR_BF16_LEFT_OUT is exactly what is not), and every keep pattern (both
needles, one, none) occurs on at least 10 % of the paired rows of every pair problem."""
import pytest
import torch

import dropout_exact as X
import prefill_needles as P

DTYPES = (torch.bfloat16, torch.float16)
DTYPE_IDS = ('bf16', 'fp16')
CASE_IDS = [X.case_id(c) for c in X.READ_CASES]


def _r16(x, dtype):
    return x.float().to(dtype).float()


# ---- A. read-outs -------------------------------------------------------------------------------------------------------------

def _readout_model(prob, keeps, p, dtype):
    """An fp32 evaluation with exactly the two 16-bit roundings of the kernels' path: the forward rounds the unnormalised
    exp(s - max) for the matrix unit and the product with Z / l at the store; the backward rounds P Z (dV) or dS = P Z dP (dQ,
    dK) for the matrix unit and the result at the store."""
    zf = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))
    per_seq = []
    for s, keep in zip(prob['seqs'], keeps):
        if s is None:
            per_seq.append(None)
            continue
        sc = s['s'].float()
        z = keep.float() * zf
        if prob['kind'] == 'fwd':
            pun = torch.exp(sc - sc.max(-1, keepdim=True).values)
            per_seq.append(_r16(_r16(pun, dtype) * (z / pun.sum(-1, keepdim=True)), dtype).double())
        else:
            pr = torch.exp(sc - s['lse'].float()[..., None])
            per_seq.append(_r16(pr * z * (1.0 if prob['kind'] == 'dv' else float(prob['d'])), dtype).double())
    got = X.readout_gather(prob, per_seq, factor=False)
    if prob['kind'] in ('dq', 'dk'):
        got = _r16(got.float() * prob['scale'], dtype).double()
    return got


@pytest.mark.parametrize('case', X.READ_CASES, ids=CASE_IDS)
def test_readout_models_meet_the_criteria_and_wrong_masks_do_not(case):
    """Per case and read-out: the margins, the two-rounding model within MODEL_TOL roundings under every p and both states,
    and the five wrong masks outside the criterion at p = 0.17, 0.5 and 0.9."""
    for kind in X.KINDS:
        prob = X.readout_problem(case, kind)
        for s in prob['seqs']:
            if s is not None:
                visible = s['p'][s['p'] > 0]
                for dtype in DTYPES:             # the forward rounds exp(s - max) >= P, the backward P Z >= P
                    assert float(visible.min()) >= 2 * X.SMALLEST_NORMAL[dtype], (kind, float(visible.min()))
        for n, p in enumerate(X.P_VALUES):
            for state in X.STATES:
                want = X.readout_want(prob, state, p)
                keeps = X.readout_keep(prob, state, p)
                for dtype in DTYPES:
                    got = _readout_model(prob, keeps, p, dtype)
                    assert not X.readout_failures(got, want, dtype, kind), (kind, p, dtype)
                    rel = ((got - want).abs() / want.abs().clamp(min=1e-300))[want != 0].max().item()
                    assert rel <= X.MODEL_TOL * X.ROUNDING[dtype], (kind, p, dtype, rel)
                if p == X.P_VALUES[-1]:
                    continue
                for mutant in X.MASK_MUTANTS:
                    if mutant == 'offset >> 32 ignored' and state[1] >> 32 == 0:
                        continue                 # the first state has no high word to ignore
                    wrong = X.readout_want(prob, state, p, mutant)
                    assert X.readout_failures(wrong, want, DTYPES[n % 2], kind), (kind, p, state, mutant)


def test_the_smallest_p_drops_something():
    """p = 1e-6: the threshold clamps to 65535 and a pair drops with probability 2^-16.  Under the two states together every
    case drops at least one visible pair (1 to 15 of them), so the case is not vacuous: the probability dump of the GPU file
    sees every one of them.  The windows of the read-outs cover d / S of the pairs; the dropped pairs they see (printed: none
    at d = 80 and at sq != sk, up to two elsewhere) come on top, and everywhere else they demand a non-zero entry."""
    p = X.P_VALUES[-1]
    assert X.R.threshold(p) == 65535
    for case in X.READ_CASES:
        hidden, seen = 0, []
        for state in X.STATES:
            prob = X.readout_problem(case, 'fwd')
            keeps = X.readout_keep(prob, state, p)
            hidden += sum(int(((s['p'] > 0) & ~k).sum()) for s, k in zip(prob['seqs'], keeps) if s is not None)
            for kind in X.KINDS:
                prob = X.readout_problem(case, kind)
                full = X.readout_gather(prob, [None if s is None else s['p'] for s in prob['seqs']])
                seen.append(int(((full != 0) & (X.readout_want(prob, state, p) == 0)).sum()))
        print(f'{X.case_id(case)}: {hidden} visible pairs dropped, seen by the read-outs (state x kind): {seen}')
        assert hidden >= 1, X.case_id(case)


# ---- B. pair problems -----------------------------------------------------------------------------------------------------------

def _dense(prob, keep, causal, mutant=None):
    """fp64 attention with dropout at p = 1/2, forward and backward, from the operands alone.  keep (b, h, sq, sk)."""
    q, k, v, dout = (prob[x].double() for x in ('q', 'k', 'v', 'dout'))
    sq, sk = q.shape[1], k.shape[1]
    s = prob['scale'] * torch.einsum('bthd,bshd->bhts', q, k)
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(sq, sk, dtype=torch.bool), 1), float('-inf'))
    z = 2.0 * keep.double()
    lse = torch.logsumexp(s, -1)
    pr = torch.exp(s - lse[..., None])
    zp = z * pr
    if mutant == 'the row sum after the mask':
        e = keep * torch.exp(s - s.max(-1, keepdim=True).values)
        total = e.sum(-1, keepdim=True)
        zp = torch.where(total > 0, 2.0 * e / total.clamp(min=1e-300), 0.0)
        lse = torch.log(total[..., 0]) + s.max(-1).values
    out = torch.einsum('bhts,bshd->bthd', zp, v)
    dd = (dout * out).sum(-1).permute(0, 2, 1)[..., None]                   # (b, h, t, 1)
    dp = torch.einsum('bthd,bshd->bhts', dout, v)
    ds = pr * z * (dp - dd) if mutant == 'Z applied to D as well' else pr * (z * dp - dd)
    dv = torch.einsum('bhts,bthd->bshd', pr if mutant == 'Z missing from dV' else zp, dout)
    return dict(out=out, lse=lse, dq=prob['scale'] * torch.einsum('bhts,bshd->bthd', ds, k),
                dk=prob['scale'] * torch.einsum('bhts,bthd->bshd', ds, q), dv=dv)


ARITHMETIC_MUTANTS = ('Z applied to D as well', 'Z missing from dV', 'the row sum after the mask')


def _pair_failures(m, prob, dtype):
    return (P.exact_failures(m['out'], prob['want'], dtype, 'out', prob['zero_out']) + P.lse_failures(m['lse'], prob['lse'])
            + P.exact_failures(m['dq'], prob['want_dq'], dtype, 'dq', prob['zero_dq'])
            + P.exact_failures(m['dk'], prob['want_dk'], dtype, 'dk', prob['zero_dk'])
            + P.exact_failures(m['dv'], prob['want_dv'], dtype, 'dv'))


def _representable(prob, dtype, tag):
    for x in ('want', 'want_dq', 'want_dk', 'want_dv'):
        assert torch.equal(prob[x].to(dtype).double(), prob[x]), f'{tag}: {x} not representable in {dtype}'


def _shares(prob, tag):
    """both / one / none of a paired row's two needles kept: expected 25, 50, 25 %."""
    parts = prob.get('parts', [prob])
    paired = torch.cat([(p['js2'] != p['js']).flatten() for p in parts])
    kept = torch.cat([(p['k1'].long() + p['k2'].long()).flatten() for p in parts])[paired]
    for count in (0, 1, 2):
        share = (kept == count).float().mean().item()
        assert share >= 0.10, (tag, count, share)


def _keep_of(prob, state, sq, sk, slot0=0, streams=None):
    b, h = prob['js'].shape[:2]
    return X.keep_mask(state, streams or slot0 + b * h, sq, sk, X.PAIR_P)[slot0:slot0 + b * h].view(b, h, sq, sk)


def _check_pair(tag, prob, causal, dtype, state, slot0=0, streams=None):
    _representable(prob, dtype, tag)
    sq, sk = prob['q'].shape[1], prob['k'].shape[1]
    keep = _keep_of(prob, state, sq, sk, slot0, streams)
    assert not _pair_failures(_dense(prob, keep, causal), prob, dtype), tag
    for mutant in ARITHMETIC_MUTANTS:
        assert _pair_failures(_dense(prob, keep, causal, mutant), prob, dtype), (tag, mutant)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_pair_cases_are_their_closed_forms_and_mutants_are_not(dtype):
    """Every pair problem the GPU file runs: representable, the fp64 reference == the closed forms under the GPU criteria,
    the three arithmetic mutants outside them, the keep patterns' shares."""
    done = 0
    for tag, prob in X.pair_fixed_problems(dtype):
        _check_pair(tag, prob, True, dtype, X.PAIR_STATE['fixed'])
        _shares(prob, tag)
        done += 1
    for tag, prob in X.pair_cross_problems(dtype):
        _check_pair(tag, prob, False, dtype, X.PAIR_STATE['cross'])
        _shares(prob, tag)
        done += 1
    c = P.FLASH_BWD_RAGGED
    for tag, prob in X.pair_ragged_problems(dtype):
        _representable(prob, dtype, tag)
        _shares(prob, tag)
        for n, part in enumerate(prob['parts']):
            seq = [i for i, length in enumerate(c['lens']) if length > 0][n]
            _representable(part, dtype, tag)
            length = part['q'].shape[1]
            keep = _keep_of(part, X.PAIR_STATE['ragged'], length, length, seq * c['h'], len(c['lens']) * c['h'])
            assert not _pair_failures(_dense(part, keep, True), part, dtype), (tag, seq)
            if length >= 70:                                                  # enough rows for every mutant to bite
                for mutant in ARITHMETIC_MUTANTS:
                    assert _pair_failures(_dense(part, keep, True, mutant), part, dtype), (tag, seq, mutant)
        done += 1
    assert done >= 50


def test_pair_wrong_masks_fail_the_pair_criteria():
    """The closed forms built from a wrong mask are not the closed forms: the pair problems see the mask as well."""
    for dtype in DTYPES:
        case = [dict(d=P.PAIR_CHAIN['d'], seqlens=[P.PAIR_CHAIN['s']])]
        for mutant in X.MASK_MUTANTS:
            right = list(X.pair_cross_problems(dtype)) + list(X.pair_ragged_problems(dtype))        # the second state
            wrong = list(X.pair_cross_problems(dtype, mutant=mutant)) + list(X.pair_ragged_problems(dtype, mutant=mutant))
            if mutant != 'offset >> 32 ignored':                                                     # the first state
                right += list(X.pair_fixed_problems(dtype, cases=case))
                wrong += list(X.pair_fixed_problems(dtype, cases=case, mutant=mutant))
            for (tag, prob), (_, bad) in zip(right, wrong):
                got = dict(out=bad['want'], lse=None, dq=bad['want_dq'], dk=bad['want_dk'], dv=bad['want_dv'])
                fails = (P.exact_failures(got['out'], prob['want'], dtype, 'out', prob['zero_out'])
                         + P.exact_failures(got['dq'], prob['want_dq'], dtype, 'dq', prob['zero_dq'])
                         + P.exact_failures(got['dk'], prob['want_dk'], dtype, 'dk', prob['zero_dk'])
                         + P.exact_failures(got['dv'], prob['want_dv'], dtype, 'dv'))
                assert fails, (tag, mutant)


def test_pair_bf16_exclusions_are_the_unrepresentable_ones():
    """dropout_exact.PAIR_BF16_LEFT_OUT is exactly the set of (map, d, S) whose closed forms, with the map in its slot of the
    rotation (the mask is a function of the slot), bf16 cannot hold; fp16 holds every one.  At most 8 of the 162 triples are
    left out and every map survives at every d."""
    triples = 0
    for dtype in DTYPES:
        found = set()
        for case in P.PAIR_BWD_CASES:
            for s in case['seqlens']:
                b, h = P.bh_of(s)
                for rot in P.rotations(P.BWD_MAPS, 3):
                    maps = P.slot_maps(P.BWD_MAPS, 3, rot)
                    prob = X.pair_problem(maps, b, h, s, s, case['d'], X.PAIR_STATE['fixed'], **X.PAIR_MAGS[dtype])
                    for slot, m in enumerate(maps):
                        triples += 1
                        sl = [prob[x][slot] if b == 3 else prob[x][0, :, slot] for x in ('want', 'want_dq', 'want_dk', 'want_dv')]
                        if not all(torch.equal(x.to(dtype).double(), x) for x in sl):
                            found.add((m, case['d'], s))
        assert found == (set(X.PAIR_BF16_LEFT_OUT) if dtype == torch.bfloat16 else set()), (dtype, found)
    assert triples == 2 * 162 and len(X.PAIR_BF16_LEFT_OUT) <= 8
    for case in P.PAIR_BWD_CASES:
        for m in P.BWD_MAPS:
            assert any((m, case['d'], s) not in X.PAIR_BF16_LEFT_OUT for s in case['seqlens']), (m, case['d'])


def test_pair_closed_forms_without_dropout_are_unchanged():
    """prefill_needles._pair_closed_forms with keep = None: the forms of tests/test_gpu_prefill_needles.py, n / 4 and all."""
    prob = P.pair_attn_problem(P.slot_maps(P.BWD_MAPS, 3, 0), 1, 3, 385, 385, 64, **P.PAIR_MAGS[torch.float16])
    paired = (prob['js2'] != prob['js']).permute(0, 2, 1)[..., None]
    k1, k2 = P._rows_of(prob['k'].double(), prob['js']), P._rows_of(prob['k'].double(), prob['js2'])
    v1, v2 = P._rows_of(prob['v'].double(), prob['js']), P._rows_of(prob['v'].double(), prob['js2'])
    n = prob['n'][..., None]
    assert torch.equal(prob['want_dq'], prob['scale'] * n / 4 * (k1 - k2))
    assert torch.equal(prob['want'], torch.where(paired, (v1 + v2) / 2, v1))
    assert torch.equal(prob['zero_dq'], P.GRAD_DUST + prob['scale'] * P.FP32_SUM * n.abs() / 4 * (k1.abs() + k2.abs()))
    dk = P.fan_in(prob['js'], n / 4 * prob['q'].double(), 385)[0] - P.fan_in(prob['js2'], n / 4 * prob['q'].double() * paired, 385)[0]
    assert torch.equal(prob['want_dk'], prob['scale'] * dk)
    ones = (torch.ones_like(prob['js'], dtype=torch.bool),) * 2
    same = P._pair_closed_forms(prob['q'], prob['k'], prob['v'], prob['dout'], prob['js'], prob['js2'], prob['scale'], 385, keep=ones)
    assert torch.equal(same['want'], 2 * prob['want']) and torch.equal(same['want_dv'], 2 * prob['want_dv'])


# ---- C. LayerNorm -----------------------------------------------------------------------------------------------------------------

def test_layer_norm_problems_and_wrong_masks():
    """The plain evaluation of dropout(x0 rowscale) / (1 - p) colscale at p = 1/2 is exactly 2 x0 (times the power-of-two
    scales) where kept, representable in both dtypes; the wrong masks that can differ with one stream differ on every width, a
    run of 4 on in the last 256-column chunk too."""
    for cols in X.LN_FWD_COLS:
        rows = X.LN_ROWS[-1]
        x0 = X.ln_x0(rows, cols)
        rs, cs = X.ln_scales(rows, cols)
        for dtype in DTYPES:
            assert torch.equal(x0.to(dtype).float(), x0) and int(x0.abs().min()) >= 1
            assert torch.equal(rs.to(dtype).float(), rs) and torch.equal(cs.to(dtype).float(), cs)
        for state in X.STATES:
            keep = X.ln_keep(state, rows, cols, 0.5)
            plain = torch.where(keep, x0 * rs[:, None] / (1 - 0.5), torch.zeros(())) * cs
            assert torch.equal(plain, 2 * x0 * rs[:, None] * cs * keep)
            for p in X.LN_P:
                keep = X.ln_keep(state, rows, cols, p)
                assert abs(1 - keep.float().mean().item() - p) < 0.01
                for mutant in ('one key on', 'one run of 4 on', 'rows and columns swapped') + (('offset >> 32 ignored',) if state[1] >> 32 else ()):
                    if mutant == 'rows and columns swapped' and cols > 2048:
                        continue
                    wrong = X.ln_keep(state, rows, cols, p, mutant)
                    assert not torch.equal(wrong, keep), (cols, mutant)
                    last = (cols - 1) // 256 * 256
                    assert not torch.equal(wrong[:, last:], keep[:, last:]), (cols, mutant)
