"""GPU: the MXFP8 sense table -- bp_sense_table_quantize / _dequantize bit for bit against their torch twins,
bp_sense_decode_mx8 against fp32 on the dequantised table (the rule of decode_support), exact needles, side effects, and
BackpackConfig(sense_table_dtype='mxfp8') decoding through it."""
import copy
from unittest import mock

import pytest
import torch

from decode_support import DEV, VOCAB, _bp, _model, _same_bits, _within_2x

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('d_out', [32, 96, 768])
def test_quantize_and_dequantize_match_the_torch_twins(d_out, k, dtype):
    """A strided table (a slice of a wider one) of magnitudes 2^-3 .. 2^3 with an all-zero block and two blocks of one
    +-power of two among zeros: both kernels give the bytes of the twins run on the CPU; every dequantised value is a
    multiple of 2^-24 (checked), so the fp16 table holds it exactly."""
    bp = _bp()
    g = torch.Generator().manual_seed(d_out + k)
    sign = torch.randint(0, 2, (5, k, d_out + 32), generator=g) * 2 - 1
    wide = (torch.exp2(torch.rand(5, k, d_out + 32, generator=g) * 6 - 3) * sign).to(dtype)
    table = wide[:, :, 16:16 + d_out]
    table[0, 0, :32] = 0
    table[1, 0, -32:], table[2, 0, :32] = 0, 0
    table[1, 0, -7], table[2, 0, 0] = 4.0, -0.25
    want_q8, want_s8 = bp._eager_sense_table_quantize(table)
    want = bp._eager_sense_table_dequantize(want_q8, want_s8, dtype)
    assert ((want.double() * 2.0 ** 24) % 1 == 0).all() and want.abs().max() < 65504
    assert want_s8[0, 0, 0] == 127 and not want[0, 0, :32].any()
    assert torch.equal(want[1, 0, -32:], table[1, 0, -32:]) and torch.equal(want[2, 0, :32], table[2, 0, :32])
    q8, s8 = bp.sense_table_quantize(table.to(DEV))
    assert torch.equal(q8.cpu(), want_q8) and torch.equal(s8.cpu(), want_s8)
    out = torch.zeros_like(wide, device=DEV)
    got = bp.sense_table_dequantize(q8, s8, dtype, out=out[:, :, 16:16 + d_out])
    assert _same_bits(got.cpu(), want) and not out[:, :, :16].any() and not out[:, :, 16 + d_out:].any()
    again = bp.sense_table_quantize(got)
    assert torch.equal(again[0], q8) and torch.equal(again[1], s8)


def _twin(q, k_new, keys, q8, s8, rows, new_row, lengths, scale, kw, dtype):
    """src.models.backpack._eager_sense_decode_mx8 in `dtype` on copies of the caches, the row index clamped as the kernel's."""
    from src.models.backpack import _eager_sense_decode_mx8
    rows = rows.clone().clamp_(0, q8.shape[0] - 1)
    return _eager_sense_decode_mx8(q.to(dtype), k_new.to(dtype), keys.clone().to(dtype), q8, s8, rows, new_row, 0, lengths, scale,
                                   key_weight=kw)


LENGTHS = [0, 63, 64, 200]      # the empty cache, both sides of a tile edge, several splits


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('shape', [(64, 16, 768), (160, 4, 640), (640, 1, 640), (8, 3, 32), (48, 2, 96)], ids=str)
def test_sense_decode_mx8_matches_fp32_and_appends_like_sense_decode(shape, dtype, weighted):
    """max|kernel - fp32 twin| <= 2 max|same-dtype twin - fp32 twin| + 1e-5 per sample, on the dequantised table; one cached
    row index lies outside the table (clamped to its last row).  The key cache and the row index end as bp_sense_decode on
    the 16-bit table leaves clones of them; a second call gives the same bits."""
    bp = _bp()
    dk, k, dout = shape
    g = torch.Generator(device=DEV).manual_seed(dk + k)
    b, max_s, vocab = len(LENGTHS), 256, 97
    q, k_new = (torch.randn(b, k, dk, device=DEV, generator=g).to(dtype) * s for s in (2.0, 1.0))
    keys = torch.randn(b, max_s, k, dk, device=DEV, generator=g).to(dtype)
    q8, s8 = bp.sense_table_quantize(torch.randn(vocab, k, dout, device=DEV, generator=g).to(dtype))
    rows = torch.randint(0, vocab, (b, max_s), device=DEV, generator=g, dtype=torch.int32)
    rows[3, 5] = vocab + 1000
    new_row = torch.randint(0, vocab, (b,), device=DEV, generator=g, dtype=torch.int32)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    kw = torch.rand(b, k, max_s, device=DEV, generator=g) * 3 if weighted else None
    scale = dk ** -0.5
    ref, eager = (_twin(q, k_new, keys, q8, s8, rows, new_row, lengths, scale, kw, dt) for dt in (torch.float32, dtype))
    keys16, rows16 = keys.clone(), rows.clone()
    bp.sense_decode(q, k_new, keys16, bp.sense_table_dequantize(q8, s8, dtype), rows16, new_row, lengths, scale, key_weight=kw)
    out = bp.sense_decode_mx8(q, k_new, keys, q8, s8, rows, new_row, lengths, scale, key_weight=kw)
    assert _same_bits(keys, keys16) and torch.equal(rows, rows16)
    for i, L in enumerate(LENGTHS):
        _within_2x(out[i], ref[i], eager[i], f'sense_decode_mx8 {shape} {dtype} weighted={weighted} L={L}')
    assert _same_bits(bp.sense_decode_mx8(q, k_new, keys, q8, s8, rows, new_row, lengths, scale, key_weight=kw), out)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('d_out', [96, 768])
def test_needle_returns_the_dequantised_row_bit_for_bit(d_out, dtype):
    """k = 1, every key zero but one whose score is 32 * 16 / sqrt(8) * log2(e) = 261 in the exp2 domain: its probability
    is exactly 1, the others' exactly 0 (2^-261 underflows), so out[b] is the needle's dequantised table row.  Three samples
    of L = 200 (3 rows of 1 sense at 256 cached positions: 4 splits of 51 keys): the needle at 0, at the last key of the
    second split, and at L (the new key)."""
    bp = _bp()
    g = torch.Generator(device=DEV).manual_seed(d_out)
    L, at, vocab = 200, [0, 101, 200], 61
    q, k_new = torch.zeros(3, 1, 8, device=DEV, dtype=dtype), torch.zeros(3, 1, 8, device=DEV, dtype=dtype)
    keys = torch.zeros(3, 256, 1, 8, device=DEV, dtype=dtype)
    q[:, 0, 0], keys[0, 0, 0, 0], keys[1, 101, 0, 0], k_new[2, 0, 0] = 32.0, 16.0, 16.0, 16.0
    q8, s8 = bp.sense_table_quantize(torch.randn(vocab, 1, d_out, device=DEV, generator=g).to(dtype))
    rows = torch.randint(0, vocab, (3, 256), device=DEV, generator=g, dtype=torch.int32)
    new_row = torch.randint(0, vocab, (3,), device=DEV, generator=g, dtype=torch.int32)
    out = bp.sense_decode_mx8(q, k_new, keys, q8, s8, rows, new_row, torch.full((3,), L, dtype=torch.int32, device=DEV))
    table = bp.sense_table_dequantize(q8, s8, dtype)
    for i, j in enumerate(at):     # rows[i, L] holds new_row[i] after the call
        assert _same_bits(out[i], table[rows[i, j].long(), 0]), (i, j)


# ---- model level -------------------------------------------------------------------------------------------------------

def _mx8_model(name, seed=0):
    from src.models.backpack import BackpackLMHeadModel
    base = _model(name, seed)
    cfg = copy.deepcopy(base.config)
    cfg.sense_table_dtype = 'mxfp8'
    model = BackpackLMHeadModel(cfg, device=DEV, dtype=torch.bfloat16).eval()
    model.load_state_dict(base.state_dict())
    return model


def _steps(model, bp, steps, spy_on='sense_decode_mx8', never='sense_decode'):
    """Prefill 16, then `steps` cached steps with every call of bp.<spy_on> checked against its eager twin by the 2 x rule;
    bp.<never> must not be reached.  Returns the key_weight of every call."""
    from src.utils.generation import InferenceParams
    seen, real = [], getattr(bp, spy_on)

    def checked(q, k_new, keys, q8, s8, rows, new_row, lengths, scale=None, out=None, key_weight=None):
        ref, eager = (_twin(q, k_new, keys, q8, s8, rows, new_row, lengths, scale, key_weight, dt) for dt in (torch.float32, q.dtype))
        got = real(q, k_new, keys, q8, s8, rows, new_row, lengths, scale, out, key_weight)
        _within_2x(got, ref, eager, f'model step {len(seen)}')
        seen.append(key_weight)
        return got
    ids = torch.randint(0, VOCAB, (2, 16 + steps), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    ip = InferenceParams(max_sequence_len=16 + steps, max_batch_size=2)
    boom = mock.Mock(side_effect=AssertionError(f'bp_hip.{never} reached'))
    with torch.inference_mode(), mock.patch.object(bp, never, boom), \
            mock.patch.object(bp, spy_on, checked if spy_on == 'sense_decode_mx8' else real):
        model(ids[:, :16], inference_params=ip)
        for t in range(16, 16 + steps):
            ip.sequence_len_offset = t
            model(ids[:, t:t + 1], inference_params=ip)
    return seen


@pytest.mark.parametrize('name', ['small', 'mini_k4'])
def test_mxfp8_model_decodes_through_the_8_bit_kernel(name):
    """Every one of 32 cached steps calls bp_hip.sense_decode_mx8 (never sense_decode), each within the 2 x rule of its
    eager twin; generate(cg=True) returns generate(cg=False)'s tokens.  The new kernel deals keys to threads in another
    order than bp_sense_decode (R = 256 / (d / 16) residues, not 256 / (d / 8)), so the issue's "bit-identical to the 16-bit
    kernel" variant of this test does not apply and is left out."""
    bp, model = _bp(), _mx8_model(name)
    assert _steps(model, bp, 32) == [None] * 32
    ids = torch.randint(0, VOCAB, (3, 16), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    assert torch.equal(model.generate(ids, 48, kv_cache=True, cg=True), model.generate(ids, 48, kv_cache=True, cg=False))


def test_weighted_wrapper_without_annealing_decodes_through_the_8_bit_kernel():
    from src.models.intervened_models import WeightedBackpackLMHeadModel
    bp, model = _bp(), _mx8_model('small')
    cw = (torch.rand(model.lm_head.weight.shape[0], 16, generator=torch.Generator().manual_seed(11)) * 3).to(DEV)
    seen = _steps(WeightedBackpackLMHeadModel(model, cw, None, 0.1, anneal=False).eval(), bp, 8)
    assert len(seen) == 8 and all(w is not None for w in seen)


def test_default_config_never_reaches_the_8_bit_kernel():
    bp, model = _bp(), _model('small')
    _steps(model, bp, 2, spy_on='sense_decode', never='sense_decode_mx8')
    assert model.transformer._sense_table.rows is not None and model.transformer._sense_table.q8 is None
