"""GPU: KV-cached decoding -- bp_flash_decode and bp_sense_decode against fp32 eager references (the project's 2x rule),
the cache appends, repeatability, and the cached Backpack decode loop (eager and graph-replayed) against the full
forward."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def _bp():
    import bp_hip
    bp_hip.lib()
    return bp_hip


def _within_2x(got, ref, eager, what):
    """max|kernel - fp32 oracle| <= 2 max|same-dtype eager - fp32 oracle| + 1e-5 (tests/test_gpu_kernels.py)."""
    ref = ref.float().cpu()
    err = (got.float().cpu() - ref).abs().max().item()
    base = (eager.float().cpu() - ref).abs().max().item()
    print(f'{what}: kernel {err:.3e} eager-same-dtype {base:.3e}')
    assert err <= 2 * base + 1e-5, (what, err, base)


def _attend(q, keys, values, scale, dtype):
    """softmax(scale q . k_j) v summed over j, in `dtype` (the eager twin's op order: scale K, softmax in v's dtype)."""
    q, keys, values = q.to(dtype), keys.to(dtype), values.to(dtype)
    scores = torch.einsum('hd,shd->hs', q, keys * scale)
    p = torch.softmax(scores, dim=-1, dtype=dtype)
    return torch.einsum('hs,shd->hd', p, values)


# ---- bp_flash_decode --------------------------------------------------------------------------------------------------

FLASH_LENGTHS = [[0, 1, 2, 63, 64, 65, 1000, 4096], [1024, 5], [1]]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('d', [64, 80, 128])
@pytest.mark.parametrize('lengths', FLASH_LENGTHS, ids=['mixed8', 'two', 'one'])
def test_flash_decode_matches_fp32(d, dtype, lengths):
    bp = _bp()
    g = torch.Generator(device=DEV).manual_seed(d + len(lengths))
    b, h, max_s, off = len(lengths), 4, 4104, 2
    full = torch.randn(b + off + 1, max_s, 2, h, d, device=DEV, generator=g).to(dtype)
    cache = full[off:off + b]                    # a cache at a non-zero batch_size_offset
    q, k_new, v_new = (torch.randn(b, h, d, device=DEV, generator=g).to(dtype) * s for s in (2.0, 1.0, 1.0))
    seqlens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    before = full.clone()
    scale = d ** -0.5
    out, lse = bp.flash_decode(q, k_new, v_new, cache, seqlens, scale, return_lse=True)
    torch.cuda.synchronize()
    want_cache = before.clone()
    for i, L in enumerate(lengths):
        want_cache[off + i, L, 0] = k_new[i]
        want_cache[off + i, L, 1] = v_new[i]
    assert torch.equal(full, want_cache), 'only row L of each sample may change, and it must hold k_new / v_new'
    for i, L in enumerate(lengths):
        keys = torch.cat([before[off + i, :L, 0], k_new[i:i + 1]])
        values = torch.cat([before[off + i, :L, 1], v_new[i:i + 1]])
        ref = _attend(q[i], keys, values, scale, torch.float32)
        eager = _attend(q[i], keys, values, scale, dtype)
        _within_2x(out[i], ref, eager, f'flash_decode d={d} {dtype} L={L}')
        ref_lse = torch.logsumexp(torch.einsum('hd,shd->hs', q[i].float(), keys.float()) * scale, dim=-1)
        torch.testing.assert_close(lse[i], ref_lse, rtol=1e-5, atol=1e-4)
    again = bp.flash_decode(q, k_new, v_new, cache, seqlens, scale)
    assert torch.equal(again, out), 'repeated calls must be bit-identical'


# ---- bp_sense_decode --------------------------------------------------------------------------------------------------

# (d_k as project() returns it, true d_k, senses, d_out): Micro, Small, Mini k = 64 (10 padded to 16), k = 4, k = 1
SENSE_SHAPES = [(24, 24, 16, 384), (48, 48, 16, 768), (16, 10, 64, 640), (160, 160, 4, 640), (640, 640, 1, 640)]
SENSE_LENGTHS = [0, 1, 63, 64, 65, 1000, 4096, 7]


def _sense_ref(q, keys, content, scale, dtype):
    """o = sum_l sum_j softmax_j(scale q_l . k_l(j)) content[j, l] (ContextSelfAttn + _combine_senses on the last row)."""
    q, keys, content = q.to(dtype), keys.to(dtype), content.to(dtype)
    scores = torch.einsum('ld,sld->ls', q, keys * scale)
    p = torch.softmax(scores, dim=-1, dtype=dtype)
    return torch.einsum('ls,sld->d', p, content)


@pytest.mark.parametrize('form', ['table', 'cache'])
@pytest.mark.parametrize('shape', SENSE_SHAPES, ids=[f'dk{s[1]}_k{s[2]}' for s in SENSE_SHAPES])
def test_sense_decode_matches_fp32(shape, form):
    _sense_decode_matches_fp32(shape, form, torch.bfloat16)


@pytest.mark.parametrize('form', ['table', 'cache'])
@pytest.mark.parametrize('shape', SENSE_SHAPES, ids=[f'dk{s[1]}_k{s[2]}' for s in SENSE_SHAPES])
def test_sense_decode_matches_fp32_in_fp16(shape, form):
    _sense_decode_matches_fp32(shape, form, torch.float16)


def _sense_decode_matches_fp32(shape, form, dtype):
    bp = _bp()
    dkp, dk, k, dout = shape
    g = torch.Generator(device=DEV).manual_seed(dkp * 7 + k)
    lengths = SENSE_LENGTHS if dkp <= 48 else SENSE_LENGTHS[:4] + [4096]
    b, max_s, vocab = len(lengths), 4100, 997
    pad = torch.zeros(dkp, device=DEV)
    pad[:dk] = 1.0                                # the padded columns of project() are exactly zero

    def senses(*lead):
        return (torch.randn(*lead, k, dkp, device=DEV, generator=g) * pad).to(dtype)
    q, k_new = senses(b) * 2, senses(b)
    k_cache = senses(b, max_s)
    if form == 'table':
        table = torch.randn(vocab, k, dout, device=DEV, generator=g).to(dtype)
        rows = torch.randint(0, vocab, (b, max_s), device=DEV, generator=g, dtype=torch.int32)
        new_row = torch.randint(0, vocab, (b,), device=DEV, generator=g, dtype=torch.int32)
    else:
        table = torch.randn(b * max_s, k, dout, device=DEV, generator=g).to(dtype)
        rows = (torch.arange(b, device=DEV)[:, None] * max_s + torch.arange(max_s, device=DEV)).int()
        new_row = (torch.arange(b, device=DEV) * max_s + torch.tensor(lengths, device=DEV)).int()
    seqlens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    kc_before, rows_before = k_cache.clone(), rows.clone()
    scale = dk ** -0.5
    out = bp.sense_decode(q, k_new, k_cache, table, rows, new_row, seqlens, scale)
    torch.cuda.synchronize()
    want_kc, want_rows = kc_before.clone(), rows_before.clone()
    for i, L in enumerate(lengths):
        want_kc[i, L] = k_new[i]
        want_rows[i, L] = new_row[i]
    assert torch.equal(k_cache, want_kc) and torch.equal(rows, want_rows)
    for i, L in enumerate(lengths):
        keys = torch.cat([kc_before[i, :L], k_new[i:i + 1]])
        idx = torch.cat([rows_before[i, :L], new_row[i:i + 1]]).long()
        content = table[idx]
        ref = _sense_ref(q[i], keys, content, scale, torch.float32)
        eager = _sense_ref(q[i], keys, content, scale, dtype)
        _within_2x(out[i], ref, eager, f'sense_decode {shape} {form} {dtype} L={L}')
    again = bp.sense_decode(q, k_new, k_cache, table, rows, new_row, seqlens, scale)
    assert torch.equal(again, out), 'repeated calls must be bit-identical'


# ---- model level ------------------------------------------------------------------------------------------------------

MODELS = {   # two layers of each trunk, the sense shapes of the named configurations
    'micro': dict(n_embd=384, n_head=6, num_content_vectors=16),
    'small': dict(n_embd=768, n_head=12, num_content_vectors=16),
    'mini_k64': dict(n_embd=640, n_head=8, num_content_vectors=64),
    'mini_k4': dict(n_embd=640, n_head=8, num_content_vectors=4),
    'mini_k1': dict(n_embd=640, n_head=8, num_content_vectors=1),
}
VOCAB = 4096


def _model(name, seed=0):
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    import warnings
    torch.manual_seed(seed)
    cfg = BackpackConfig(n_layer=2, vocab_size=VOCAB, n_positions=256, scale_attn_by_inverse_layer_idx=True,
                         use_flash_attn=True, fused_bias_fc=True, fused_dense_gelu_dense=True, fused_dropout_add_ln=True,
                         pad_vocab_size_multiple=8, **MODELS[name])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = BackpackLMHeadModel(cfg, device=DEV, dtype=torch.bfloat16).eval()
    # sharpen the sense softmax as Small's x 8 does at d_k = 48 (score spread ~ mult^2 sqrt(d_k)): a fixed x 8 would make the
    # one-sense d_k = 640 model 3.6 x sharper, where near-ties turn one-ulp trunk differences into large weight swings
    dk = cfg.n_embd // cfg.num_content_vectors
    with torch.no_grad():
        model.transformer.contextualization_attn.Wqkv.weight.mul_(8.0 * (48 / dk) ** 0.25)
    assert model.transformer.fused_senses
    return model


def _fp32_twin(model):
    """The eager op sequence (use_flash_attn=False) in fp32 with the same weights: the oracle of the model-level checks."""
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    kw = {k: v for k, v in model.config.to_dict().items() if k in ('n_embd', 'n_head', 'n_layer', 'num_content_vectors',
                                                                   'vocab_size', 'n_positions')}
    twin = BackpackLMHeadModel(BackpackConfig(scale_attn_by_inverse_layer_idx=True, use_flash_attn=False, **kw))
    twin.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    return twin.to(DEV).eval()


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


def _cached_logits(model, seq, prompt):
    """Logits of the last position of `seq` (1, S) by prefill on `prompt` tokens + cached steps."""
    from src.utils.generation import InferenceParams
    ip = InferenceParams(max_sequence_len=seq.shape[1], max_batch_size=1)
    with torch.inference_mode():
        logits = model(seq[:, :prompt], inference_params=ip).logits[:, -1]
        for t in range(prompt, seq.shape[1]):
            ip.sequence_len_offset = t
            logits = model(seq[:, t:t + 1], inference_params=ip).logits[:, -1]
    return logits[0].float()


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
