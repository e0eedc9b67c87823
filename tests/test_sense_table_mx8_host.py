"""CPU: the torch twins of the MXFP8 sense table (bp_hip._eager_sense_table_quantize / _dequantize) against a float64
restatement of the format of include/bp_hip.h, the config switch on a nano model, and the argument checks of the C ABI."""
import ctypes

import pytest
import torch

from decode_support import PROMPT, STEPS, _nano_backpack

import bp_hip
from src.models.backpack import BackpackConfig, BackpackLMHeadModel


def _value64(q8, scale8):
    """e4m3(q8) * 2^(scale8 - 127) per element, in float64."""
    return q8.view(torch.float8_e4m3fn).double() * (2.0 ** (scale8.double() - 127)).repeat_interleave(32, dim=-1)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('scale', [2.0 ** -6, 1.0, 2.0 ** 5])
def test_round_trip_is_within_half_an_ulp_and_idempotent(scale, dtype):
    """Every element comes back within half an E4M3 ulp of its own binade, times its block's scale (ulp = 2^(e - 3) for a
    scaled magnitude in [2^e, 2^(e+1)), 2^-9 below the smallest normal 2^-6): round to nearest.  The format clamps scaled
    magnitudes to 448 before rounding, so an element above 448 scales (the block maximum normalises to [256, 512)) comes back
    as exactly +-448 scales instead.  A second quantisation of the dequantised table returns the same bytes."""
    table = (torch.randn(5, 3, 96, generator=torch.Generator().manual_seed(3)) * scale).to(dtype)
    q8, scale8 = bp_hip._eager_sense_table_quantize(table)
    back = bp_hip._eager_sense_table_dequantize(q8, scale8, dtype)
    assert torch.equal(back.double(), _value64(q8, scale8)), 'the dequantised value is exact in the 16-bit type'
    unit = (2.0 ** (scale8.double() - 127)).repeat_interleave(32, dim=-1)
    x = table.double() / unit
    half_ulp = 0.5 * torch.maximum(2.0 ** (torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -6))) - 3), torch.tensor(2.0 ** -9))
    clamped = x.abs() > 448
    err = (back.double() / unit - x).abs()
    print(f'scale {scale} {dtype}: worst error {(err / half_ulp)[~clamped].max().item():.3f} half ulps, {int(clamped.sum())} clamped')
    assert (err <= half_ulp)[~clamped].all()
    assert torch.equal((back.double() / unit)[clamped], 448.0 * torch.sign(x[clamped]))
    assert x.abs().amax() < 512 and (x.abs().reshape(5, 3, 3, 32).amax(-1) >= 256).all()
    again = bp_hip._eager_sense_table_quantize(back)
    assert torch.equal(again[0], q8) and torch.equal(again[1], scale8)


def test_special_blocks_round_trip_exactly():
    table = torch.zeros(1, 1, 96, dtype=torch.bfloat16)
    table[0, 0, 32 + 5], table[0, 0, 64 + 31] = 2.0 ** -9, -(2.0 ** 6)     # one element of +-amax, a power of two, 31 zeros
    q8, scale8 = bp_hip._eager_sense_table_quantize(table)
    assert scale8.flatten().tolist() == [127, 127 - 9 - 8, 127 + 6 - 8]
    assert not q8[0, 0, :32].any() and int(q8.count_nonzero()) == 2
    assert torch.equal(bp_hip._eager_sense_table_dequantize(q8, scale8, torch.bfloat16), table)


def test_config_switch_on_a_nano_model():
    """'mxfp8': the table's 16-bit rows are exactly the values of its 8-bit twin, and the cached loop generates the tokens of
    the full-forward loop; the default config's table carries no twin; a width that is no multiple of 32 is refused."""
    model = _nano_backpack(seed=3, sense_table_dtype='mxfp8')
    ids = torch.randint(0, 200, (2, PROMPT), generator=torch.Generator().manual_seed(4))
    assert torch.equal(model.generate(ids, PROMPT + STEPS, kv_cache=True), model.generate(ids, PROMPT + STEPS))
    owner = model.transformer._sense_table
    rows = model.transformer.sense_table()
    assert owner.q8.shape == rows.shape and torch.equal(rows.double(), _value64(owner.q8, owner.scale8))
    plain = _nano_backpack(seed=3)
    assert plain.transformer.sense_table() is not None and plain.transformer._sense_table.q8 is None
    assert not torch.equal(plain.transformer.sense_table(), rows)
    with pytest.raises(ValueError, match='mxfp8'):
        BackpackLMHeadModel(BackpackConfig(n_embd=48, n_head=2, n_layer=1, num_content_vectors=2, vocab_size=50,
                                           n_positions=16, sense_table_dtype='mxfp8'))


def test_entry_points_reject_bad_arguments_before_any_launch():
    h = bp_hip.lib()
    p, null = ctypes.c_void_p(0x1000), None
    st = (768, 768, 768, 768, 24, 24)
    assert h.bp_sense_table_quantize(p, p, p, 5, 1, 48, *st, 1, null) == -3           # d_out % 32
    assert h.bp_sense_table_quantize(p, p, p, 5, 1, 768, *st, 7, null) == -1
    assert h.bp_sense_table_dequantize(p, null, p, 5, 1, 768, *st, 1, null) == -3
    assert h.bp_sense_table_dequantize(p, p, p, 5, 1, 768, 768, 768, 776, 768, 24, 24, 1, null) == -3   # q8 rows not 16-byte
    tail = (64, 64, 64, 64, 64, 64, 64, 768, 768, 24, 24, 256, 768, 0, 0, 0.125, 1, null)
    args = (p, p, p, p, p, p, p, p, null, p, p, 1 << 30, 1, 1, 64)
    assert h.bp_sense_decode_mx8(*args, 776, 256, 100, *tail) == -3                   # d_out % 32
    assert h.bp_sense_decode_mx8(*args[:14], 12, 768, 256, 100, *tail) == -2
    assert h.bp_sense_decode_mx8(*args[:11], 8, 1, 1, 64, 768, 256, 100, *tail) == -9   # workspace too small
