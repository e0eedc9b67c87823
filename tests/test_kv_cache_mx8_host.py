"""CPU: the MXFP8 KV cache of the trunk -- the row size, the torch twins (bp_hip._eager_kv_cache_quantize / _dequantize), the
argument checks of bp_flash_decode_mx8 / bp_kv_cache_quantize, and kv_cache_dtype='mxfp8' on a nano eager model."""
import ctypes
from unittest import mock

import pytest
import torch

from decode_support import PROMPT, STEPS, _close_fp32, _nano_backpack

import bp_hip
from flash_attn.modules.mha import MHA, _eager_decode_mx8
from src.utils.generation import InferenceParams


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('h,d', [(1, 32), (3, 64), (2, 96)])
def test_twins_round_trip(h, d, dtype):
    """quantise -> dequantise -> quantise gives the same bytes; the row is K, V elements then K, V scales, pad bytes zero."""
    kv = (torch.randn(2, 5, 2, h, d, generator=torch.Generator().manual_seed(h + d)) * 3).to(dtype)
    rows = bp_hip._eager_kv_cache_quantize(kv)
    assert rows.shape == (2, 5, bp_hip.kv_cache_mx8_row_bytes(h, d)) and rows.dtype == torch.uint8
    q8, s8 = bp_hip._eager_sense_table_quantize(kv[1, 3])          # (2, h, d): K heads then V heads
    used = 2 * h * d + 2 * h * d // 32
    assert torch.equal(rows[1, 3, :2 * h * d], q8.flatten()) and torch.equal(rows[1, 3, 2 * h * d:used], s8.flatten())
    assert not rows[..., used:].any()
    back = bp_hip._eager_kv_cache_dequantize(rows, h, d, dtype)
    assert back.shape == kv.shape and torch.equal(bp_hip._eager_kv_cache_quantize(back), rows)


def test_row_bytes_and_the_entry_points_argument_checks():
    assert bp_hip.kv_cache_mx8_row_bytes(12, 64) == 1584          # 1536 + 48
    assert bp_hip.kv_cache_mx8_row_bytes(1, 32) == 80             # 64 + 2, padded to a multiple of 16
    lib = bp_hip.lib()
    p, null = ctypes.c_void_p(0x1000), None

    def decode(d=64, row=1584, ws=1 << 30, dtype=1):
        return lib.bp_flash_decode_mx8(p, p, p, p, p, p, null, p, ws, 2, 12, d, 256, 768, 64, 768, 64, 768, 64, 256 * 1584, row,
                                       768, 64, 12, 0.125, dtype, null)

    def fill(d=64, row=1584, dtype=1):
        return lib.bp_kv_cache_quantize(p, p, null, 2, 40, 0, 12, d, 256, 40 * 2304, 2304, 768, 64, 256 * 1584, row, dtype, null)
    for call in (decode, fill):
        assert call(dtype=7) == -1                                # BP_ERR_DTYPE
        assert call(d=40) == -2                                   # BP_ERR_HEAD_DIM: head_dim % 32
        assert call(row=24) == -3                                 # BP_ERR_SHAPE: a row stride off its multiple of 16
        assert call(row=1536) == -3                               # ... and one that does not hold the scales
    assert decode(ws=8) == -9                                     # BP_ERR_WORKSPACE


def _recomputing_forward(real):
    """A cached step recomputes the K/V of ALL positions from every input the layer has seen and builds the cache anew."""
    history = {}

    def forward(self, x, inference_params=None, **kw):
        if inference_params.sequence_len_offset == 0:
            history[self.layer_idx] = [x]
            return real(self, x, **kw)                            # the prompt's own attention runs on the unquantised K/V
        history[self.layer_idx].append(x)
        xs = torch.cat(history[self.layer_idx], dim=1)
        qkv = self.Wqkv(xs).unflatten(-1, (3, self.num_heads, self.head_dim))
        cache = bp_hip._eager_kv_cache_quantize(qkv[:, :, 1:])
        lengths = torch.full((x.shape[0],), xs.shape[1] - 1, dtype=torch.int32)
        context = _eager_decode_mx8(qkv[:, -1, 0], qkv[:, -1, 1:], cache, 0, lengths, self.inner_attn.softmax_scale)
        return self.out_proj(context.unsqueeze(1).flatten(-2))
    return forward


def _cached_run(model, ids):
    ip = InferenceParams(max_sequence_len=ids.shape[1], max_batch_size=ids.shape[0])
    logits = []
    with torch.no_grad():
        model(ids[:, :PROMPT], inference_params=ip)
        for t in range(PROMPT, ids.shape[1]):
            ip.sequence_len_offset = t
            logits.append(model(ids[:, t:t + 1], inference_params=ip).logits[:, -1])
    return logits, ip


def test_nano_eager_model_decodes_on_the_byte_cache():
    """CPU, fp32, use_flash_attn=False: each of 20 cached steps gives the logits of the from-scratch recomputation (the fp32
    tolerance of the other CPU decode tests); a layer cache is the byte tensor; the 16-bit-cache model gives other logits; a
    bad kv_cache_dtype or head_dim raises at construction."""
    model = _nano_backpack(seed=5, kv_cache_dtype='mxfp8')
    ids = torch.randint(0, 200, (2, PROMPT + STEPS), generator=torch.Generator().manual_seed(6))
    got, ip = _cached_run(model, ids)
    with mock.patch.object(MHA, 'forward', _recomputing_forward(MHA.forward)):
        want, _ = _cached_run(model, ids)
    for t, (g, w) in enumerate(zip(got, want)):
        _close_fp32(g, w, f'step {PROMPT + t}')
    cache = ip.key_value_memory_dict[1]
    assert cache.dtype == torch.uint8 and cache.shape == (2, PROMPT + STEPS, bp_hip.kv_cache_mx8_row_bytes(6, 64))
    assert cache.any(dim=-1).all()                                # 1584 bytes, no pad
    plain, _ = _cached_run(_nano_backpack(seed=5), ids)
    assert not torch.allclose(got[-1], plain[-1], rtol=0, atol=1e-6), 'the 8-bit cache must be what the model reads'
    with pytest.raises(ValueError, match='kv_cache_dtype'):
        _nano_backpack(kv_cache_dtype='fp8')
    with pytest.raises(ValueError, match='head_dim'):
        MHA(96, 2, kv_cache_dtype='mxfp8', layer_idx=0)           # head_dim 48
