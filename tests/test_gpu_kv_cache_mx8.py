"""GPU: the trunk's MXFP8 KV cache -- bp_kv_cache_quantize bit for bit against its torch twin, bp_flash_decode_mx8 against fp32
on the dequantised cache, exact needles, side effects, and kv_cache_dtype='mxfp8' through generate / sample / beam_search."""
import copy
from unittest import mock

import pytest
import torch

from decode_support import DEV, VOCAB, _bp, _model, _same_bits, _within_2x

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(1, 32), (3, 64), (2, 96), (2, 128)]
TILE = 128                      # flash_decode_mx8.hip, KV8_TILE


@pytest.mark.parametrize('form', ['padded', 'packed'])
@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('h,d', SHAPES)
def test_fill_matches_the_torch_twin_and_writes_nothing_else(h, d, dtype, form):
    """A batch_size_offset slice of a cache pre-filled with 0xA5; the source is the strided K/V part of a qkv tensor with an
    all-zero block and a block of one power of two among zeros.  Written bytes = the CPU twin's, every other byte still 0xA5."""
    bp = _bp()
    b, max_s, off, lengths = 3, 80, 2, [40, 40, 40] if form == 'padded' else [1, 33, 64]
    rows = b * 40 if form == 'padded' else sum(lengths)
    g = torch.Generator().manual_seed(h * d)
    sign = torch.randint(0, 2, (rows, 3, h, d), generator=g) * 2 - 1
    qkv = (torch.exp2(torch.rand(rows, 3, h, d, generator=g) * 6 - 3) * sign).to(dtype)    # magnitudes 2^-3 .. 2^3
    qkv[0, 1, 0, :32] = 0
    qkv[rows - 1, 2, h - 1, -32:], qkv[rows - 1, 2, h - 1, -7] = 0, 4.0
    want_rows, used = bp._eager_kv_cache_quantize(qkv[:, 1:]), bp._kv_mx8_used_bytes(h, d)
    full = torch.full((b + 3, max_s, bp.kv_cache_mx8_row_bytes(h, d)), 0xA5, dtype=torch.uint8, device=DEV)
    want = full.cpu()
    start = 0
    for i, n in enumerate(lengths):
        want[off + i, :n, :used] = want_rows[start:start + n, :used]
        start += n
    if form == 'padded':
        bp.kv_cache_quantize(qkv.to(DEV).view(b, 40, 3, h, d)[:, :, 1:], full[off:off + b])
    else:
        cu = torch.tensor([0, 1, 34, 98], dtype=torch.int32, device=DEV)
        bp.kv_cache_quantize(qkv.to(DEV)[:, 1:], full[off:off + b], cu, max(lengths))
    assert torch.equal(full.cpu(), want)


def _filled_cache(bp, rows, max_s, h, d, dtype, seed):                # quantised random K/V, every pad byte 0xA5
    g = torch.Generator(device=DEV).manual_seed(seed)
    cache = bp._eager_kv_cache_quantize(torch.randn(rows, max_s, 2, h, d, device=DEV, generator=g).to(dtype))
    cache[:, :, bp._kv_mx8_used_bytes(h, d):] = 0xA5
    return cache


def _twin(q, k_new, v_new, cache, lengths, scale, dtype):
    from flash_attn.modules.mha import _eager_decode_mx8
    return _eager_decode_mx8(q.to(dtype), torch.stack([k_new, v_new], dim=1).to(dtype), cache, 0, lengths, scale)


# one sample per length: empty cache, both sides of the tile edge, full cache, several splits; the last case: 132 (sample,
# head) rows give 4 splits of up to 256 keys, so a workgroup walks one tile, one tile + 1 key, two tiles
CASES = [(h, d, [0, TILE - 1, TILE, 2 * TILE - 1, 200], 256) for h, d in SHAPES + [(12, 64)]]
CASES.append((12, 64, [0, 4 * TILE - 1, 4 * TILE, 4 * TILE + 1, 600, 1023, 767, 5, 300, 511, 1000], 1024))


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('h,d,lengths,max_s', CASES, ids=lambda v: str(v) if not isinstance(v, list) else f'b{len(v)}')
def test_decode_matches_fp32_and_appends_the_quantised_token(h, d, lengths, max_s, dtype):
    """The 2 x rule against the fp32 twin per sample; the whole cache (a slice of a larger one) then equals the twin's byte
    for byte (row L holds the quantised new K/V and scales, nothing else moved); a second call gives the same bits."""
    bp, b, off = _bp(), len(lengths), 1
    g = torch.Generator(device=DEV).manual_seed(h + d)
    full = _filled_cache(bp, b + 2, max_s, h, d, dtype, d)
    q, k_new, v_new = (torch.randn(b, h, d, device=DEV, generator=g).to(dtype) * s for s in (2.0, 1.0, 1.0))
    seqlens, scale = torch.tensor(lengths, dtype=torch.int32, device=DEV), d ** -0.5
    want_full = full.clone()
    ref = _twin(q, k_new, v_new, want_full[off:off + b], seqlens, scale, torch.float32)
    eager = _twin(q, k_new, v_new, full.clone()[off:off + b], seqlens, scale, dtype)
    out, lse = bp.flash_decode_mx8(q, k_new, v_new, full[off:off + b], seqlens, scale, return_lse=True)
    assert torch.equal(full, want_full)
    for i, L in enumerate(lengths):
        _within_2x(out[i], ref[i], eager[i], f'flash_decode_mx8 {(h, d)} {dtype} L={L}')
    k = bp._eager_kv_cache_dequantize(want_full[off:off + b], h, d, torch.float32)[:, :, 0]
    scores = torch.einsum('bhd,bshd->bhs', q.float(), k) * scale
    scores.masked_fill_((torch.arange(max_s, device=DEV)[None, :] > seqlens[:, None])[:, None, :], float('-inf'))
    torch.testing.assert_close(lse, torch.logsumexp(scores, dim=-1), rtol=1e-5, atol=1e-4)
    assert _same_bits(bp.flash_decode_mx8(q, k_new, v_new, full[off:off + b], seqlens, scale), out)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('d', [32, 128])
def test_needle_returns_the_dequantised_value_row_bit_for_bit(d, dtype):
    """One head, every key zero but one: q . k = 256 * 16, at least 4096 / sqrt(128) * log2(e) = 522 in the exp2 domain against
    0, so the probabilities are exactly 1 and 0 and out[b] is the needle's dequantised V row.  L = 200 (4 splits of 51 keys):
    the needle at key 0, at the last key of the second split, and at L (the new token: the ROUNDED v_new)."""
    bp = _bp()
    at, cache = [0, 101, 200], _filled_cache(bp, 3, 256, 1, d, dtype, d)
    cache[:, :, :d] = 0                                            # K elements: every cached key is zero
    q, k_new = torch.zeros(3, 1, d, device=DEV, dtype=dtype), torch.zeros(3, 1, d, device=DEV, dtype=dtype)
    v_new = torch.randn(3, 1, d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d)).to(dtype)
    q[:, 0, 0], k_new[2, 0, 0] = 256.0, 16.0
    key = torch.zeros(1, 2, 1, d, dtype=dtype, device=DEV)
    key[0, 0, 0, 0] = 16.0
    key_row = bp._eager_kv_cache_quantize(key)[0]
    for i in (0, 1):
        cache[i, at[i], :d], cache[i, at[i], 2 * d:2 * d + d // 32] = key_row[:d], key_row[2 * d:2 * d + d // 32]
    seqlens, want_cache = torch.full((3,), 200, dtype=torch.int32, device=DEV), cache.clone()
    _twin(q, k_new, v_new, want_cache, seqlens, d ** -0.5, torch.float32)                   # appends row L
    values = bp._eager_kv_cache_dequantize(want_cache, 1, d, dtype)[:, :, 1, 0]             # (3, 256, d)
    if dtype == torch.float16:
        assert ((values.double() * 2.0 ** 24) % 1 == 0).all() and values.abs().max() < 65504
    out = bp.flash_decode_mx8(q, k_new, v_new, cache, seqlens)
    assert torch.equal(cache, want_cache)
    for i, j in enumerate(at):
        assert _same_bits(out[i, 0], values[i, j]), (i, j)


def _steps(model, ids, patches):
    """Prefill 16 tokens, then one cached step per further column of `ids`, under the given patches of bp_hip."""
    from src.utils.generation import InferenceParams
    ip = InferenceParams(max_sequence_len=ids.shape[1], max_batch_size=ids.shape[0])
    with torch.inference_mode(), mock.patch.multiple(_bp(), **patches):
        model(ids[:, :16], inference_params=ip)
        for t in range(16, ids.shape[1]):
            ip.sequence_len_offset = t
            model(ids[:, t:t + 1], inference_params=ip)
    return ip.key_value_memory_dict[0]


def test_mxfp8_model_decodes_through_the_8_bit_kernels():
    """32 cached steps call bp_hip.flash_decode_mx8 (never flash_decode), each within the 2 x rule of its twin; generate,
    sample on a packed prefill and beam_search return with cg=True what they return with cg=False.  The default config
    reaches neither new call and keeps the 5-D 16-bit cache."""
    from src.models.backpack import BackpackLMHeadModel
    bp, base = _bp(), _model('small')
    cfg = copy.deepcopy(base.config)
    cfg.kv_cache_dtype = 'mxfp8'
    model = BackpackLMHeadModel(cfg, device=DEV, dtype=torch.bfloat16).eval()
    model.load_state_dict(base.state_dict())
    calls, real = [], bp.flash_decode_mx8

    def checked(q, k_new, v_new, cache, lengths, scale=None, out=None, return_lse=False):
        ref, eager = (_twin(q, k_new, v_new, cache.clone(), lengths, scale, dt) for dt in (torch.float32, q.dtype))
        got = real(q, k_new, v_new, cache, lengths, scale, out, return_lse)
        _within_2x(got, ref, eager, f'model call {len(calls)}')
        calls.append(cache.shape)
        return got
    boom = mock.Mock(side_effect=AssertionError('the other cache format\'s call reached'))
    ids = torch.randint(0, VOCAB, (2, 48), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    cache = _steps(model, ids, dict(flash_decode=boom, flash_decode_mx8=checked))
    assert calls == [(2, 48, 1584)] * 64                           # 2 layers x 32 steps
    assert cache.dtype == torch.uint8 and cache.any(dim=-1).all()
    cache = _steps(base, ids[:, :18], dict(flash_decode_mx8=boom, kv_cache_quantize=boom))
    assert cache.shape == (2, 18, 2, 12, 64) and cache.dtype == torch.bfloat16
    ids = ids[:, :16]
    with mock.patch.object(bp, 'flash_decode', boom):
        assert torch.equal(model.generate(ids, 48, kv_cache=True, cg=True), model.generate(ids, 48, kv_cache=True, cg=False))
        drawn = [model.sample(ids, 40, kv_cache=True, cg=cg, prompt_lengths=[16, 9], packed_prefill=True, top_k=20,
                              rng_state=torch.tensor([1234, 77], dtype=torch.int64, device=DEV)) for cg in (True, False)]
        assert torch.equal(drawn[0], drawn[1])
        beams = [model.beam_search(ids, 32, 3, return_dict_in_generate=True, cg=cg) for cg in (True, False)]
        assert torch.equal(beams[0].beam_sequences, beams[1].beam_sequences)
        assert _same_bits(beams[0].beam_scores, beams[1].beam_scores)
