"""GPU: bp_sense_anneal_step against the formulas of include/bp_hip.h in float64, exactly on integers, and in the wrapper."""
from unittest import mock

import pytest
import torch

from decode_support import (SENSE_SHAPES, VOCAB, _anneal_scale, _ar, _assert_scores_in_band, _bp, _fp32_twin, _model,
                            _within_2x)

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
P, MAX_S, SCALE, SENTINEL = 16, 203, 0.1, -12345.0         # P: positions per workgroup (AS_POS of csrc/bp_kernels.h)
LENGTHS = [0, 1, P - 1, P, P + 1, 63, 64, 65, MAX_S - 1]
SHAPES = dict(argvalues=SENSE_SHAPES, ids=[f'k{s[2]}_d{s[3]}' for s in SENSE_SHAPES])
DTYPES = dict(argvalues=[torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])


def _inputs(shape, dtype, integers):
    _, _, k, dout = shape
    g = torch.Generator(device=DEV).manual_seed(dout + k + integers)
    b, vocab = len(LENGTHS), 61                            # few tokens: ids repeat

    def draw(*size):
        if integers:
            return torch.randint(-1, 2, size, device=DEV, generator=g).to(dtype)
        return (torch.randn(*size, device=DEV, generator=g) * dout ** -0.5).to(dtype)
    table, emb = draw(vocab, k, dout), draw(vocab, dout)
    ids = torch.randint(0, vocab, (b, MAX_S), device=DEV, generator=g)
    rows = torch.randint(0, vocab, (b, MAX_S), device=DEV, generator=g, dtype=torch.int32)
    new_row = torch.randint(0, vocab, (b,), device=DEV, generator=g, dtype=torch.int32)
    new_ids = torch.randint(0, vocab, (b,), device=DEV, generator=g)
    rows[5, 3], rows[6, 40], rows[7, 64], ids[8, 100] = -1, vocab, 2 ** 31 - 1, vocab + 5    # clamped to the last row
    if integers:
        sims = torch.randint(0, 8, (b, k, MAX_S), device=DEV, generator=g).float()
    else:
        sims = (torch.rand(b, k, MAX_S, device=DEV, generator=g) + 0.5) * 6 / SCALE
    weight = torch.full((b, k, MAX_S), SENTINEL, device=DEV)
    for i, L in enumerate(LENGTHS):
        ids[i, L:] = -7
        sims[i, :, L:] = SENTINEL
    cw = torch.rand(vocab, k, device=DEV, generator=g) * 3
    lens = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    return table, rows, new_row, lens, emb, ids, new_ids, cw, sims, weight


def _reference(table, rows, new_row, emb, ids, new_ids, cw, sims, upweight, ft):
    """sims, scores before the nearby factor and weights at positions 0 .. L of every sample, computed in `ft`."""
    last = table.shape[0] - 1
    out = []
    for i, L in enumerate(LENGTHS):
        r = torch.cat([rows[i, :L], new_row[i:i + 1]]).long()
        r = torch.where((r < 0) | (r > last), last, r)
        x = torch.cat([ids[i, :L], new_ids[i:i + 1]])
        x = torch.where((x < 0) | (x > last), last, x)
        hit = torch.relu(table[r].to(ft) @ emb[x[L]].to(ft))                          # (L + 1, k)
        own = torch.relu(table[r[L]].to(ft) @ emb[x].to(ft).T).sum(dim=1)             # (k,): the pair (L, L) included
        s = torch.cat([sims[i, :, :L].to(ft) + hit[:L].T, own[:, None]], dim=1)      # (k, L + 1)
        score = torch.sigmoid(6 - SCALE * s)
        near = score * (1 + _ar(L + 1).to(torch.float32) / 100).to(ft) if upweight else score
        out.append((s, score, cw[x].to(ft).T * near + (1 - near)))
    return out


def _run(inputs, upweight):
    table, rows, new_row, lens, emb, ids, new_ids, cw, sims, weight = inputs
    state = ids.clone(), sims.clone(), weight.clone()
    _bp().sense_anneal_step(table, rows, new_row, lens, emb, state[0], new_ids, cw, state[1], state[2], SCALE, upweight)
    torch.cuda.synchronize()
    return state


@pytest.mark.parametrize('upweight', [True, False], ids=['nearby', 'flat'])
@pytest.mark.parametrize('dtype', **DTYPES)
@pytest.mark.parametrize('shape', **SHAPES)
def test_anneal_step_matches_fp64(shape, dtype, upweight):
    """err <= 2 err(fp32 torch restatement) + 1e-5 max|ref| on sims and on weight at [0, L]; ids[b, L] = the new id; nothing
    past L and no read-only operand changes; a second call from the same state is bit-identical."""
    inputs = _inputs(shape, dtype, integers=False)
    assert _bp().sense_anneal_step_supported(inputs[0], inputs[4])
    before = [t.clone() for t in inputs]
    got_ids, got_sims, got_weight = _run(inputs, upweight)
    assert all(torch.equal(a, b) for a, b in zip(inputs, before)), 'only the state tensors are written'
    ref64 = _reference(*inputs[:3], *inputs[4:9], upweight, torch.float64)
    ref32 = _reference(*inputs[:3], *inputs[4:9], upweight, torch.float32)
    scores = torch.cat([r[1].flatten() for r in ref64])
    assert ((scores >= 0.05) & (scores <= 0.95)).double().mean().item() >= 0.5
    for i, L in enumerate(LENGTHS):
        for what, got, n in (('sims', got_sims, 0), ('weight', got_weight, 2)):
            ref = ref64[i][n]
            err = (got[i, :, :L + 1].double() - ref).abs().max().item()
            base = (ref32[i][n].double() - ref).abs().max().item()
            assert err <= 2 * base + 1e-5 * ref.abs().max().item(), (what, L, err, base)
            assert (got[i, :, L + 1:] == SENTINEL).all(), f'{what} past L is left untouched'
        assert got_ids[i, L] == inputs[6][i] and torch.equal(got_ids[i, :L], inputs[5][i, :L])
        assert (got_ids[i, L + 1:] == -7).all(), 'ids past L are left untouched'
    again = _run(inputs, upweight)
    assert all(torch.equal(a, b) for a, b in zip(again, (got_ids, got_sims, got_weight))), 'bit-identical across calls'


@pytest.mark.parametrize('dtype', **DTYPES)
@pytest.mark.parametrize('shape', **SHAPES)
def test_anneal_step_counts_every_pair_exactly_once(shape, dtype):
    """Entries of {-1, 0, 1} and small integer sums: every product and sum is an integer, exact in fp32 in any order."""
    inputs = _inputs(shape, dtype, integers=True)
    _, got_sims, _ = _run(inputs, True)
    ref64 = _reference(*inputs[:3], *inputs[4:9], True, torch.float64)
    for i, L in enumerate(LENGTHS):
        assert torch.equal(got_sims[i, :, :L + 1].double(), ref64[i][0]), f'{shape} {dtype} L={L}'


@pytest.mark.parametrize('name', ['micro', 'mini_k64'])
def test_fused_anneal_step_in_the_wrapper(name):
    """Prefill 16 + 10 cached steps: logits within 2 x the unfused wrapper's error against the fp32 twin, a replayed captured
    step = the eager fused steps bit for bit, and no step reaches bp_sense_rows_dot or the torch update."""
    import src.models.intervened_models as IM
    from src.utils.generation import InferenceParams
    bp = _bp()
    model = _model(name, seed=3)
    twin = _fp32_twin(model)
    prompt, steps, b = 16, 10, 3
    ids = torch.randint(0, VOCAB, (b, prompt + steps), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    lengths = range(prompt + 1, prompt + steps + 1)
    cw = (torch.rand(model.lm_head.weight.shape[0], model.config.num_content_vectors,
                     generator=torch.Generator().manual_seed(11)) * 3).to(DEV)
    scale = _anneal_scale(twin, ids, lengths)
    _assert_scores_in_band(twin, ids, scale, lengths)
    fused, plain, ref = (IM.WeightedBackpackLMHeadModel(m, cw, None, scale, anneal=True, upweight_nearby=True).eval()
                         for m in (model, model, twin))
    fused.fused_anneal_step = True

    def fresh(wrapper):
        ip = InferenceParams(max_sequence_len=prompt + steps, max_batch_size=b)
        ip.lengths_per_sample = torch.zeros(b, dtype=torch.int32, device=DEV)
        wrapper(ids[:, :prompt], inference_params=ip)
        ip.sequence_len_offset = prompt
        ip.lengths_per_sample.fill_(prompt)
        return ip

    def step(wrapper, ip, tokens):
        logits = wrapper(tokens, inference_params=ip).logits[:, -1]
        ip.lengths_per_sample += 1
        return logits

    boom = mock.Mock(side_effect=AssertionError('the unfused update was reached'))
    with torch.inference_mode():
        ip = fresh(fused)
        assert 'intervened_dots' not in ip.key_value_memory_dict
        with mock.patch.object(bp, 'sense_rows_dot', boom), mock.patch.object(IM, '_anneal_weights', boom), \
                mock.patch.object(IM, '_eager_rows_dot', boom):
            eager = [step(fused, ip, ids[:, t:t + 1]).clone() for t in range(prompt, prompt + steps)]
        ip = fresh(plain)
        unfused = [step(plain, ip, ids[:, t:t + 1]).clone() for t in range(prompt, prompt + steps)]
        for i, t in enumerate(range(prompt, prompt + steps)):
            _within_2x(eager[i], ref(ids[:, :t + 1]).logits[:, -1], unfused[i], f'{name} step {t}')
        ip = fresh(fused)
        replayed = [step(fused, ip, ids[:, prompt:prompt + 1]).clone()]
        static_ids = ids[:, prompt + 1:prompt + 2].clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_logits = step(fused, ip, static_ids)
        for t in range(prompt + 1, prompt + steps):
            static_ids.copy_(ids[:, t:t + 1])
            graph.replay()
            replayed.append(static_logits.clone())
    for i, (a, r) in enumerate(zip(eager, replayed)):
        assert torch.equal(a, r), f'step {i}'
