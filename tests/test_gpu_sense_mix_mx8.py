"""GPU: bp_sense_mix_gather_mx8 -- the gathering sense mix on the MXFP8 sense table -- against fp32 on the dequantised rows
(the 2 x rule of decode_support) and against exact needles that pin the conversion, the scale bytes and the LDS image."""
import pytest
import torch

from decode_support import DEV, _bp, _same_bits, _within_2x

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]

# (B, S, k, d_k, d_out, rows)
SHAPES = [(2, 77, 4, 16, 512, 7),           # partial key step, few rows
          (3, 300, 4, 24, 96, 97),          # second query tile, d_k padded to 32, a chunk narrower than 256 columns
          (1, 288, 2, 48, 288, 300),        # one full plus one partial chunk, a 32-column tail
          (2, 1024, 16, 48, 768, 5000),     # the Small shape
          (1, 320, 64, 16, 640, 65536)]     # 64 senses, byte offsets of q8 beyond 2 GiB


def _pair(rows, k, d_out, g, lowest=118):
    """Every E4M3 code but the two NaNs and -0 (a sum that starts at +0 cannot return -0, so a needle could not be compared
    bit for bit) under scales 2^-9 .. 2^-1: the sum over 64 senses stays inside fp16.  `lowest`: the smallest scale byte."""
    q8 = torch.randint(0, 256, (rows, k, d_out), device=DEV, generator=g, dtype=torch.uint8)
    q8[((q8 & 0x7f) == 0x7f) | (q8 == 0x80)] = 0
    return q8, torch.randint(lowest, 127, (rows, k, d_out // 32), device=DEV, generator=g, dtype=torch.uint8)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_matches_fp32_on_the_dequantised_rows(shape, dtype):
    """max|kernel - fp32 twin| <= 2 max|same-dtype twin - fp32 twin| + 1e-5 per sample; the index holds 0, rows - 1 and one
    value outside the table (it reads the last row).  A second call gives the same bits, the out= / lse= form those of the
    plain one, and bp.sense_mix on the gathered dequantised rows agrees bit for bit."""
    bp = _bp()
    b, s, k, dk, dout, rows = shape
    g = torch.Generator(device=DEV).manual_seed(s + k)
    qk = torch.randn(b, s, 2, k, dk, device=DEV, generator=g).to(dtype)
    q8, s8 = _pair(rows, k, dout, g)
    index = torch.randint(0, rows, (b, s), device=DEV, generator=g, dtype=torch.int32)
    index[0, 0], index[0, 1], index[-1, 5] = 0, rows - 1, rows + 1000
    ref, eager = (bp._eager_sense_mix_gather_mx8(qk.to(dt), q8, s8, index) for dt in (torch.float32, dtype))
    out = bp.sense_mix_gather_mx8(qk, q8, s8, index)
    for i in range(b):
        _within_2x(out[i], ref[i], eager[i], f'sense_mix_gather_mx8 {shape} {dtype} sample {i}')
    assert _same_bits(bp.sense_mix_gather_mx8(qk, q8, s8, index), out)
    into = torch.full_like(out, float('nan'))
    assert bp.sense_mix_gather_mx8(qk, q8, s8, index, out=into, lse=bp.sense_lse(qk)) is into and _same_bits(into, out)
    flat = index.long().clamp(max=rows - 1).reshape(-1)
    content = bp.sense_table_dequantize(q8[flat], s8[flat], dtype).view(b, s, k, dout)
    assert _same_bits(bp.sense_mix(qk, content), out)


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('d_out', [96, 768])
def test_needle_returns_the_dequantised_row_bit_for_bit(d_out, dtype):
    """k = 1, every key zero but one per sample whose score against the probed query is 32 * 16 / sqrt(8) * log2(e) = 261 in
    the exp2 domain: its probability is exactly 1, the others' exactly 0, so out[b, query] is the needle's dequantised row.
    Needles (key, query): key 0 seen from the second 256-query tile, the last key of a 32-key step on its diagonal, the
    first key of the next step, and the diagonal of a query in the second tile.  Scales down to 2^-15: every value is a
    multiple of 2^-24, so the fp16 table holds it exactly (the contract of bp_sense_table_dequantize), subnormals included."""
    bp = _bp()
    g = torch.Generator(device=DEV).manual_seed(d_out)
    needles, s, rows = [(0, 299), (31, 31), (32, 33), (300, 300)], 320, 61
    qk = torch.zeros(len(needles), s, 2, 1, 8, device=DEV, dtype=dtype)
    for i, (key, query) in enumerate(needles):
        qk[i, query, 0, 0, 0], qk[i, key, 1, 0, 0] = 32.0, 16.0
    q8, s8 = _pair(rows, 1, d_out, g, lowest=112)
    index = torch.randint(0, rows, (len(needles), s), device=DEV, generator=g, dtype=torch.int32)
    out = bp.sense_mix_gather_mx8(qk, q8, s8, index)
    table = bp.sense_table_dequantize(q8, s8, dtype)
    for i, (key, query) in enumerate(needles):
        assert _same_bits(out[i, query], table[index[i, key].long(), 0]), (key, query)


# ---- model level: BackpackConfig(sense_table_dtype='mxfp8_only') ------------------------------------------------------------

BUILD_ROWS = 1024      # four build chunks over the 4096-row vocabulary of decode_support's models


def _with_table(name, dtype):
    import copy
    from decode_support import _model
    from src.models.backpack import BackpackLMHeadModel
    base = _model(name)
    cfg = copy.deepcopy(base.config)
    cfg.sense_table_dtype, cfg.sense_table_build_rows = dtype, BUILD_ROWS
    model = BackpackLMHeadModel(cfg, device=DEV, dtype=torch.bfloat16).eval()
    model.load_state_dict(base.state_dict())
    return model


@pytest.mark.parametrize('name', ['small', 'mini_k64'])
def test_mxfp8_only_model_serves_the_pair_alone(name):
    """'mxfp8_only' against 'mxfp8' on the same weights: eval logits within the 2 x rule of the fp32 eager model (the 'mxfp8'
    model in the place of the same-dtype leg: both encode one table), equal greedy tokens from generate(kv_cache=True, cg=True)
    (the kernel-level comparison gave equal bits); the 16-bit gather and the dequantiser are never reached; after the table
    build the model holds less memory by at least the 16-bit table minus one build chunk; the default and 'mxfp8' models
    never reach the new kernel."""
    from unittest import mock
    from decode_support import _fp32_twin
    bp = _bp()
    ids = torch.randint(0, 4096, (2, 48), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    refuse = AssertionError('not in this mode')
    out, held = {}, {}
    for mode in (None, 'mxfp8', 'mxfp8_only'):
        model = _with_table(name, mode)
        never = ['sense_mix_gather', 'sense_table_dequantize'] if mode == 'mxfp8_only' else ['sense_mix_gather_mx8']
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        with mock.patch.multiple(bp, **{n: mock.DEFAULT for n in never}) as spies, torch.no_grad():
            for spy in spies.values():
                spy.side_effect = refuse
            model.transformer.refresh_inference_caches()
            torch.cuda.synchronize()
            held[mode] = torch.cuda.memory_allocated() - before
            out[mode] = (model(ids).logits.float(), model.generate(ids, 64, kv_cache=True, cg=True))
        table = model.transformer._sense_table
        assert (table.rows is None) == (mode == 'mxfp8_only') and (table.q8 is None) == (mode is None)
        if mode is None:
            ref = _fp32_twin(model)(ids).logits
    k, d = model.config.num_content_vectors, model.config.n_embd
    print(f'{name}: table memory default {held[None]} mxfp8 {held["mxfp8"]} mxfp8_only {held["mxfp8_only"]} bytes')
    assert held['mxfp8'] - held['mxfp8_only'] >= 4096 * k * d * 2 - BUILD_ROWS * k * d * 2
    _within_2x(out['mxfp8_only'][0], ref, out['mxfp8'][0], f'{name} mxfp8_only logits')
    assert torch.equal(out['mxfp8_only'][1], out['mxfp8'][1])
