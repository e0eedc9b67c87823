"""GPU: KV-cached decoding -- bp_flash_decode and bp_sense_decode against fp32 eager references (the project's 2x rule),
the cache appends, repeatability, and the cached Backpack decode loop (eager and graph-replayed) against the full
forward."""
import pytest
import torch

from decode_support import (DEV, FLASH_LENGTHS, MODELS, SENSE_SHAPES, VOCAB, _cached_logits, _flash_decode_matches_fp32, _fp32_twin,
                            _model, _sense_decode_matches_fp32)

pytestmark = pytest.mark.gpu


# ---- bp_flash_decode --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('d', [64, 80, 128])
@pytest.mark.parametrize('lengths', FLASH_LENGTHS, ids=['mixed8', 'two', 'one'])
def test_flash_decode_matches_fp32(d, dtype, lengths):
    _flash_decode_matches_fp32(d, dtype, lengths)


# ---- bp_sense_decode --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('form', ['table', 'cache'])
@pytest.mark.parametrize('shape', SENSE_SHAPES, ids=[f'dk{s[1]}_k{s[2]}' for s in SENSE_SHAPES])
def test_sense_decode_matches_fp32(shape, form):
    _sense_decode_matches_fp32(shape, form, torch.bfloat16)


@pytest.mark.parametrize('form', ['table', 'cache'])
@pytest.mark.parametrize('shape', SENSE_SHAPES, ids=[f'dk{s[1]}_k{s[2]}' for s in SENSE_SHAPES])
def test_sense_decode_matches_fp32_in_fp16(shape, form):
    _sense_decode_matches_fp32(shape, form, torch.float16)


# ---- model level ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', ['cached', 'off'])
@pytest.mark.parametrize('name', list(MODELS))
def test_cached_decode_matches_the_full_forward(name, mode):
    """Prefill, then 64 cached steps ('cached': table form, 'off': cache form).  Against the fp32 eager twin on the full
    prefix, every step's logits are within 2^-7 of the max logit (the table-vs-per-position tolerance of
    tests/test_gpu_configs.py), or within the 3 x rule of the model-level oracle checks (tests/test_gpu_configs.py, smoke())
    relative to the full HIP forward of the same prefix.  (The two HIP
    paths differ by rounding: the flash forward rounds P to 16 bit for its PV product, the decode kernel keeps it in fp32;
    LayerNorm amplifies those ulps.)"""
    from src.utils.generation import InferenceParams
    model = _model(name)
    model.transformer.sense_table_mode = mode
    twin = _fp32_twin(model)
    prompt, steps, b = 16, 64, 2
    ids = torch.randint(0, VOCAB, (b, prompt + steps), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    ip = InferenceParams(max_sequence_len=prompt + steps, max_batch_size=b)
    ip.lengths_per_sample = torch.zeros(b, dtype=torch.int32, device=DEV)
    with torch.inference_mode():
        model(ids[:, :prompt], inference_params=ip)
        assert ('backpack_content' in ip.key_value_memory_dict) == (mode == 'off')
        ip.sequence_len_offset = prompt
        ip.lengths_per_sample.fill_(prompt)
        worst = 0.0
        for t in range(prompt, prompt + steps):
            got = model(ids[:, t:t + 1], inference_params=ip).logits[:, -1].float()
            ip.lengths_per_sample += 1
            ip.sequence_len_offset += 1
            full = model(ids[:, :t + 1]).logits[:, -1].float()
            ref = twin(ids[:, :t + 1]).logits[:, -1]
            err, base = (got - ref).abs().max().item(), (full - ref).abs().max().item()
            bound = max(2 ** -7 * ref.abs().max().item(), 3 * base)     # the 3 x rule of the model-level oracle checks
            worst = max(worst, err / bound)
            assert err <= bound, (name, mode, t, err, base, ref.abs().max().item())
    print(f'{name} [{mode}]: worst step error {worst:.2f} of the bound')


def test_graph_replay_is_bit_identical_to_eager_steps():
    """One captured decode step replayed N times gives the eager cached steps' logits bit for bit; generate(kv_cache=True,
    cg=True) equals generate(kv_cache=True)."""
    from src.utils.generation import InferenceParams
    model = _model('small', seed=2)
    prompt, steps, b = 16, 24, 3
    ids = torch.randint(0, VOCAB, (b, prompt + steps), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))

    def fresh():
        ip = InferenceParams(max_sequence_len=prompt + steps, max_batch_size=b)
        ip.lengths_per_sample = torch.zeros(b, dtype=torch.int32, device=DEV)
        model(ids[:, :prompt], inference_params=ip)
        ip.sequence_len_offset = prompt
        ip.lengths_per_sample.fill_(prompt)
        return ip

    with torch.inference_mode():
        ip = fresh()
        eager = []
        for t in range(prompt, prompt + steps):
            eager.append(model(ids[:, t:t + 1], inference_params=ip).logits[:, -1].clone())
            ip.lengths_per_sample += 1
        ip = fresh()
        first = model(ids[:, prompt:prompt + 1], inference_params=ip).logits[:, -1].clone()
        ip.lengths_per_sample += 1
        static_ids = ids[:, prompt + 1:prompt + 2].clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_logits = model(static_ids, inference_params=ip).logits[:, -1]
            ip.lengths_per_sample += 1
        replayed = [first]
        for t in range(prompt + 1, prompt + steps):
            static_ids.copy_(ids[:, t:t + 1])
            graph.replay()
            replayed.append(static_logits.clone())
    for i, (a, r) in enumerate(zip(eager, replayed)):
        assert torch.equal(a, r), f'step {i}'
    seq = model.generate(ids[:, :prompt], prompt + steps, kv_cache=True)
    seq_cg = model.generate(ids[:, :prompt], prompt + steps, kv_cache=True, cg=True)
    assert seq.shape == (b, prompt + steps - 1) and torch.equal(seq, seq_cg)


def test_generate_with_kv_cache_follows_generate():
    """Greedy tokens of generate(kv_cache=True) equal generate()'s up to the first step whose top-2 logit margin (on the
    full forward) is within the difference between the cached and the full-forward logits there."""
    model = _model('small', seed=4)
    with torch.no_grad():
        model.lm_head.weight.mul_(4.0)           # (tied) wider logit spread: fewer near-ties with random weights
    prompt, max_length = 16, 96
    ids = torch.randint(0, VOCAB, (4, prompt), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    full = model.generate(ids, max_length)
    cached = model.generate(ids, max_length, kv_cache=True)
    assert full.shape == cached.shape == (4, max_length - 1)
    assert torch.equal(cached[:, :prompt], ids)
    for b in range(4):
        diff = (full[b] != cached[b]).nonzero()
        if diff.numel() == 0:
            continue
        col = diff[0].item()
        with torch.inference_mode():
            logits = model(full[b:b + 1, :col]).logits[0, -1].float()
        top2 = logits.topk(2).values
        margin = (top2[0] - top2[1]).item()
        # a flip is only allowed where the two paths' logits differ by at least half the top-2 margin
        gap = (_cached_logits(model, full[b:b + 1, :col], prompt) - logits).abs().max().item()
        assert margin <= 2 * gap, (b, col, margin, gap)
