"""GPU: the backward of the sense mix on packed batches (bp_sense_mix_dc_varlen, bp_sense_dp_slab_varlen,
bp_sense_dq_dk_varlen through bp_hip.sense_mix_varlen_autograd) against fp32 autograd of the dense causal expression, per
sample, with the eager 16-bit autograd as yardstick (the rule of test_gpu_backward.py::test_sense_mix_backward).  One lengths
vector: a single token, a zero-length sample in the middle, the 64-query tile, the 128-query slab, the 256-key tile met and crossed."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
LENGTHS = (1, 129, 0, 300, 64, 257)
CU = [0, 1, 130, 130, 430, 494, 751]
MAX_S = 300
# (k, d_k, d_out): a full column chunk; padded K fragments and a partial chunk; the widest narrow sense, chunk + remainder
SHAPES = [(2, 64, 256), (2, 8, 40), (1, 128, 264)]
CASES = [(dt, shape) for dt in (torch.float16, torch.bfloat16) for shape in SHAPES]
IDS = ['%s-k%d-dk%d-d%d' % ((str(dt)[6:],) + shape) for dt, shape in CASES]


def _dense_grads(qk, c, dout):
    """dqk, dcontent of out[t] = sum_l sum_{s<=t} softmax_s(q_l[t].k_l[s] / sqrt(d_k)) c[s, l] for ONE sample, in qk's dtype."""
    qk, c = qk.clone().requires_grad_(), c.clone().requires_grad_()
    q, k = qk[:, 0].transpose(0, 1), qk[:, 1].transpose(0, 1)                      # (k, S, d_k)
    scores = (q @ k.transpose(1, 2)) * qk.shape[-1] ** -0.5
    hidden = torch.ones(scores.shape[-2:], dtype=torch.bool).triu(1)
    alpha = torch.softmax(scores.masked_fill(hidden, float('-inf')), dim=-1)
    return torch.autograd.grad(torch.einsum('lts,sld->td', alpha, c), (qk, c), dout)


def _packed_grads(qk, c, dout):
    import bp_hip
    qk, c = qk.to(DEV).requires_grad_(), c.to(DEV).requires_grad_()
    cu = torch.tensor(CU, dtype=torch.int32, device=DEV)
    out = bp_hip.sense_mix_varlen_autograd(qk, c, cu, MAX_S)
    return [g.cpu() for g in torch.autograd.grad(out, (qk, c), dout.to(DEV))]


@functools.lru_cache(maxsize=None)
def _case(dtype, shape):
    """inputs, the packed gradients of two runs, and per sample the fp32 / eager 16-bit dense gradients: computed once"""
    k, dk, d = shape
    g = torch.Generator().manual_seed(7 + dk)
    qk = (torch.randn(CU[-1], 2, k, dk, generator=g) * 1.2).to(dtype)
    c = torch.randn(CU[-1], k, d, generator=g).to(dtype)
    dout = torch.randn(CU[-1], d, generator=g).to(dtype)
    rows = [slice(CU[b], CU[b + 1]) for b in range(len(LENGTHS))]
    ref = [_dense_grads(qk[r].float(), c[r].float(), dout[r].float()) if n else None for r, n in zip(rows, LENGTHS)]
    eager = [_dense_grads(qk[r], c[r], dout[r]) if n else None for r, n in zip(rows, LENGTHS)]
    return qk, c, dout, rows, _packed_grads(qk, c, dout), _packed_grads(qk, c, dout), ref, eager


@pytest.mark.parametrize('dtype,shape', CASES, ids=IDS)
def test_packed_gradients_against_the_dense_expression(dtype, shape):
    qk, c, dout, rows, got, again, ref, eager = _case(dtype, shape)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])          # two runs, identical bits
    for b, r in enumerate(rows):
        if not LENGTHS[b]:
            continue
        for g, want, base, name in zip(got, ref[b], eager[b], ('dqk', 'dcontent')):
            err = (g[r].float() - want).abs().max().item()
            yard = (base.float() - want).abs().max().item()
            print(f'varlen bwd {shape} {dtype} sample {b} (len {LENGTHS[b]}) {name}: hip {err:.3e} eager {yard:.3e}')
            assert torch.isfinite(g[r].float()).all()
            assert err <= 2 * yard + 1e-3 * max(1.0, want.abs().max().item()), (b, name, err, yard)


@pytest.mark.parametrize('dtype,shape', CASES, ids=IDS)
def test_dcontent_carries_the_bits_of_the_fixed_length_kernel(dtype, shape):
    """same schedule, same order of sums: every sample's dC equals bp_sense_mix_dc on that sample alone, bit for bit"""
    import bp_hip
    qk, c, dout, rows, got = _case(dtype, shape)[:5]
    scale = shape[1] ** -0.5
    for b, r in enumerate(rows):
        if not LENGTHS[b]:
            continue
        qk_b, dout_b = qk[r].to(DEV)[None].contiguous(), dout[r].to(DEV)[None].contiguous()
        alone = bp_hip.sense_mix_dc(qk_b, dout_b, bp_hip.sense_lse(qk_b, scale), scale, qk_b.new_empty(0, shape[2]))
        assert torch.equal(alone[0].cpu(), got[1][r]), b


@pytest.mark.parametrize('dtype,shape', CASES, ids=IDS)
def test_a_nan_sample_stays_in_its_rows(dtype, shape):
    qk, c, dout, rows, got = _case(dtype, shape)[:5]
    bad = rows[3]                                                                  # the longest sample, in the middle
    qk, c, dout = qk.clone(), c.clone(), dout.clone()
    qk[bad], c[bad], dout[bad] = float('nan'), float('nan'), float('nan')
    poisoned = _packed_grads(qk, c, dout)
    for b, r in enumerate(rows):
        if b != 3:
            assert torch.equal(poisoned[0][r], got[0][r]) and torch.equal(poisoned[1][r], got[1][r]), b
    assert torch.isfinite(poisoned[0][:bad.start].float()).all() and torch.isfinite(poisoned[1][bad.stop:].float()).all()


@pytest.mark.parametrize('dtype,shape', CASES, ids=IDS)
def test_a_needle_in_dout_stays_in_its_sample_and_behind_its_row(dtype, shape):
    """dout is non-zero in ONE row (sample 3, in-sample query 200), the content one-hot: no gradient leaves the sample, and inside
    it dcontent is non-zero only at keys at or before the needle (and is non-zero there: the column the needle names)"""
    k, dk, d = shape
    qk = _case(dtype, shape)[0]
    c = torch.zeros(CU[-1], k, d, dtype=dtype)
    c[:, :, 3] = 1
    dout = torch.zeros(CU[-1], d, dtype=dtype)
    needle = CU[3] + 200
    dout[needle, 5] = 1
    dqk, dc = _packed_grads(qk, c, dout)
    inside = torch.zeros(CU[-1], dtype=torch.bool)
    inside[CU[3]:needle + 1] = True
    assert not dc[~inside].any() and dc[inside][:, :, 5].float().abs().sum() > 0
    assert not dc[inside][:, :, :5].any() and not dc[inside][:, :, 6:].any()
    assert not dqk[:CU[3]].any() and not dqk[CU[4]:].any()
    assert not dqk[needle + 1:CU[4], 1].any()                                      # dk of keys behind the needle
    assert torch.isfinite(dqk.float()).all()
