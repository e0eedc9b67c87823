"""What the decode tests share: the reference restatements, operand builders, models and closeness rules of
test_gpu_decode*.py, test_gpu_intervened_decode.py, test_gpu_fuzz.py and the two CPU modules test_kv_cache_host.py /
test_intervened_kv_cache_host.py.  Importing it touches no GPU.  (The exact-answer inputs live in decode_needles.py.)"""
import torch

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


FLASH_LENGTHS = [[0, 1, 2, 63, 64, 65, 1000, 4096], [1024, 5], [1]]


def _flash_decode_matches_fp32(d, dtype, lengths):
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


# (d_k as project() returns it, true d_k, senses, d_out): Micro, Small, Mini k = 64 (10 padded to 16), k = 4, k = 1
SENSE_SHAPES = [(24, 24, 16, 384), (48, 48, 16, 768), (16, 10, 64, 640), (160, 160, 4, 640), (640, 640, 1, 640)]
SENSE_LENGTHS = [0, 1, 63, 64, 65, 1000, 4096, 7]


def _sense_ref(q, keys, content, scale, dtype):
    """o = sum_l sum_j softmax_j(scale q_l . k_l(j)) content[j, l] (ContextSelfAttn + _combine_senses on the last row)."""
    q, keys, content = q.to(dtype), keys.to(dtype), content.to(dtype)
    scores = torch.einsum('ld,sld->ls', q, keys * scale)
    p = torch.softmax(scores, dim=-1, dtype=dtype)
    return torch.einsum('ls,sld->d', p, content)


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


def _close_drawn(got, ref32, eager, name, factor=2.0, floor=2.0, floor_range=0.0):
    dtype = got.dtype
    got, ref32, eager = got.float().cpu(), ref32.float().cpu(), eager.float().cpu()
    assert torch.isfinite(got).all(), name
    err = (got - ref32).abs().max().item() if got.numel() else 0.0
    base = (eager - ref32).abs().max().item() if got.numel() else 0.0
    # floor: two units of 16-bit rounding at the result's range (tiny drawn cases -- two keys, one head -- leave the eager
    # yardstick at zero or one ulp, where "twice the eager error" says nothing)
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    ulp = floor * eps * max(ref32.abs().max().item() if got.numel() else 0.0, floor_range)
    assert err <= factor * base + ulp + 1e-5, f'{name}: {err:.3e} > {factor} x {base:.3e} + {ulp:.1e}'


def _bits(t):
    """A 16-bit or int32 tensor as integers: torch.equal on these compares NaN payloads too."""
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _ar(n):
    return torch.arange(n, device=DEV)


# ---- the CPU (fp32, eager path) decode tests ------------------------------------------------------------------------------

PROMPT, STEPS = 7, 20



def _nano_backpack(seed=0, **kw):
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    torch.manual_seed(seed)
    cfg = BackpackConfig(n_embd=384, n_head=6, n_layer=2, num_content_vectors=16, vocab_size=200, n_positions=64,
                         resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, scale_attn_by_inverse_layer_idx=True,
                         use_flash_attn=False, **kw)
    model = BackpackLMHeadModel(cfg).eval()
    with torch.no_grad():
        model.transformer.contextualization_attn.Wqkv.weight.mul_(8.0)
        for layer in model.transformer.gpt2_model.layers:
            layer.mixer.Wqkv.weight.mul_(6.0)
    return model


def _close_fp32(got, want, what):
    err = (got - want).abs().max().item()
    assert err <= 1e-4 * want.abs().max().item(), (what, err, want.abs().max().item())


# ---- annealed wrappers: a scale that leaves the scores unsaturated ---------------------------------------------------------

def _sims(model, ids):
    """fp32 oracle of the similarity sums: (B,k,S) sum_j relu(C_l(x_i) . E[x_j]) over the whole of `ids`."""
    with torch.no_grad():
        content = model.transformer.content_model(ids)
        emb = model.lm_head.weight[ids]
        return torch.relu(content @ emb.transpose(1, 2).unsqueeze(1)).sum(dim=3)


def _in_band(scale, sims):
    scores = torch.sigmoid(-scale * sims + 6)
    return ((scores >= 0.1) & (scores <= 0.9)).float().mean().item()


def _anneal_scale(model, ids, lengths):
    """6 / q-quantile of the similarity sums pooled over the prefixes of the given lengths (score 1/2 at that quantile);
    of q = 0.3 .. 0.7 the one that leaves most scores unsaturated."""
    sims = torch.cat([_sims(model, ids[:, :n]).flatten() for n in lengths])
    return max((6.0 / sims.quantile(q).item() for q in (0.3, 0.4, 0.5, 0.6, 0.7)), key=lambda sc: _in_band(sc, sims))


def _assert_scores_in_band(model, ids, scale, lengths):
    sims = torch.cat([_sims(model, ids[:, :n]).flatten() for n in lengths])
    inside = _in_band(scale, sims)
    print(f'annealing scale {scale:.2f}: {100 * inside:.0f} % of {sims.numel()} scores in [0.1, 0.9]')
    assert inside >= 0.5, inside
