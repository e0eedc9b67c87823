"""CPU: bp_sense_mix_gather_mx8 refuses what it does not take before any launch, bp_hip.sense_mix_gather_mx8_limits names the
limit, and the torch twin is sense_mix's arithmetic on the dequantised rows."""
import ctypes

import pytest
import torch

import __graft_entry__  # noqa: F401  (puts the package on sys.path)
import bp_hip

# what follows (qk, q8, scale8, row_index, out, lse_ws, lse_ready, batch, seqlen, nsenses): d_k, d_out, rows, the strides of
# qk (4), q8 (2), scale8 (2), the index and out (2), the scale and the dtype
GOOD = dict(d_k=48, d_out=768, dtype=1, q8=0x1000)
REFUSALS = [(dict(d_out=776), -6, 'd_out % 32'), (dict(d_out=16), -6, 'd_out % 32'), (dict(d_k=136), -2, '> 128'),
            (dict(d_k=12), -2, None), (dict(q8=0x1008), -3, '16-byte aligned'), (dict(dtype=2), -1, 'dtype')]


@pytest.mark.parametrize('change, code, reason', REFUSALS, ids=[str(r[0]) for r in REFUSALS])
def test_refusals_have_their_codes_and_the_limits_name_them(change, code, reason):
    a = dict(GOOD, **change)
    p = ctypes.c_void_p(0x1000)
    k, dk, dout = 16, a['d_k'], a['d_out']
    rc = bp_hip.lib().bp_sense_mix_gather_mx8(p, ctypes.c_void_p(a['q8']), p, p, p, p, 1, 2, 64, k, dk, dout, 100,
                                              64 * 2 * k * dk, 2 * k * dk, k * dk, dk, k * 768, 768, k * 24, 24, 64,
                                              64 * 768, 768, 0.125, a['dtype'], None)
    assert rc == code
    if reason is None:          # the binding pads such a d_k to a multiple of 8 itself
        return
    qk = torch.zeros(2, 64, 2, k, dk, dtype=torch.float32 if a['dtype'] == 2 else torch.bfloat16)
    off = a['q8'] - 0x1000          # torch's allocations are 64-byte aligned
    q8 = torch.zeros(100 * k * dout + 16, dtype=torch.uint8)[off:off + 100 * k * dout].view(100, k, dout)
    s8 = torch.zeros(100, k, dout // 32, dtype=torch.uint8)
    # CPU tensors: 'not on the GPU' is always among the limits, so only what is named ON TOP of it tells
    named = bp_hip.sense_mix_gather_mx8_limits(qk, q8, s8, 64).split('; ')
    assert any(reason in n for n in named) and any('not on the GPU' in n for n in named)


def test_limits_name_nothing_else_for_a_call_the_kernel_takes():
    qk = torch.zeros(2, 64, 2, 16, 48, dtype=torch.bfloat16)
    q8, s8 = torch.zeros(100, 16, 768, dtype=torch.uint8), torch.zeros(100, 16, 24, dtype=torch.uint8)
    assert bp_hip.sense_mix_gather_mx8_limits(qk, q8, s8, 64) == 'qk, q8 or scale8 not on the GPU'
    assert 'workgroups' in bp_hip.sense_mix_gather_mx8_limits(qk, q8, s8, 2 ** 37)


def test_torch_twin_is_sense_mix_on_the_dequantised_rows():
    g = torch.Generator().manual_seed(0)
    qk = torch.randn(2, 9, 2, 3, 8, generator=g)
    q8, s8 = bp_hip._eager_sense_table_quantize(torch.randn(11, 3, 64, generator=g))
    index = torch.randint(0, 11, (2, 9), generator=g, dtype=torch.int32)
    index[1, 2], index[0, 3] = 4000, -1                 # both read the last row, as the kernel's unsigned clamp does
    rows = index.long().clamp(max=10)
    rows[0, 3] = 10
    content = bp_hip._eager_sense_table_dequantize(q8, s8, torch.float32)[rows]
    scores = torch.einsum('btld,bsld->blts', qk[:, :, 0], qk[:, :, 1]) * 8 ** -0.5
    alpha = torch.softmax(scores.masked_fill(~torch.ones(9, 9, dtype=torch.bool).tril(), float('-inf')), dim=-1)
    want = torch.einsum('blts,bsld->btd', alpha, content)
    got = bp_hip._eager_sense_mix_gather_mx8(qk, q8, s8, index)
    assert (got - want).abs().max() <= 1e-5 * want.abs().max()
