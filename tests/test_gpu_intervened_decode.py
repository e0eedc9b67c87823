"""GPU: KV-cached decoding of the intervened Backpacks -- bp_sense_decode_weighted and bp_sense_rows_dot against fp32 /
fp64 references (the project's 2x rule), exact visibility of keys AND weights on needle inputs (tests/decode_needles.py),
the wrappers' cached decode loop (eager and graph-replayed) against their fp32 twins, generate / sample.

Annealed cases: the scale is 6 / (a middle quantile of the fp32 twin's similarity sums over the compared prefixes), and
each annealed test asserts on the fp32 twin that at least half of the scores it compares (before `upweight_nearby`) lie
in [0.1, 0.9]: with the default scale every score of a fresh model is sigmoid(6) and a wrong running sum would not show.
content_weights are drawn from [0, 3) so that a dropped weight moves the logits."""
import inspect
from unittest import mock

import pytest
import torch

import decode_needles as N
from decode_support import (SENSE_LENGTHS, SENSE_SHAPES, VOCAB, _anneal_scale, _ar, _assert_scores_in_band, _bp,
                            _cached_logits, _fp32_twin, _model, _same_bits, _within_2x)

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ['bf16', 'fp16']
NAN = float('nan')
SHAPE_IDS = [f'dk{s[1]}_k{s[2]}' for s in SENSE_SHAPES]


def _operands(shape, form, dtype, g):
    """The operands of tests/test_gpu_decode.py::_sense_decode_matches_fp32, key-cache rows >= L poisoned."""
    dkp, dk, k, dout = shape
    lengths = SENSE_LENGTHS if dkp <= 48 else SENSE_LENGTHS[:4] + [4096]
    b, max_s, vocab = len(lengths), 4100, 997
    pad = torch.zeros(dkp, device=DEV)
    pad[:dk] = 1.0

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
        rows = (_ar(b)[:, None] * max_s + _ar(max_s)).int()
        new_row = (_ar(b) * max_s + torch.tensor(lengths, device=DEV)).int()
    for i, L in enumerate(lengths):
        k_cache[i, L:] = NAN
    seqlens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    return lengths, q, k_new, k_cache, table, rows, new_row, seqlens


# ---- bp_sense_decode_weighted -----------------------------------------------------------------------------------------

def _weighted_ref(q, keys, content, weight, scale, dtype):
    """_sense_ref with the probabilities times the weights (the eager twin multiplies in the tensors' dtype)."""
    q, keys, content = q.to(dtype), keys.to(dtype), content.to(dtype)
    scores = torch.einsum('ld,sld->ls', q, keys * scale)
    p = torch.softmax(scores, dim=-1, dtype=dtype) * weight.to(dtype)
    return torch.einsum('ls,sld->d', p, content)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('form', ['table', 'cache'])
@pytest.mark.parametrize('shape', SENSE_SHAPES, ids=SHAPE_IDS)
def test_sense_decode_weighted_matches_fp32(shape, form, dtype):
    bp = _bp()
    dkp, dk, k, dout = shape
    g = torch.Generator(device=DEV).manual_seed(dkp * 7 + k + 1)
    lengths, q, k_new, k_cache, table, rows, new_row, seqlens = _operands(shape, form, dtype, g)
    b, max_s = len(lengths), k_cache.shape[1]
    weight = torch.rand(b, k, max_s, device=DEV, generator=g) * 3
    for i, L in enumerate(lengths):
        weight[i, :, L + 1:] = NAN                       # entries [0, L] are read, L included
    assert bp.sense_decode_weighted_supported(q, k_cache, table, weight)
    kc_before, rows_before, weight_before = k_cache.clone(), rows.clone(), weight.clone()
    scale = dk ** -0.5
    out = bp.sense_decode(q, k_new, k_cache, table, rows, new_row, seqlens, scale, key_weight=weight)
    torch.cuda.synchronize()
    want_kc, want_rows = kc_before.clone(), rows_before.clone()
    for i, L in enumerate(lengths):
        want_kc[i, L] = k_new[i]
        want_rows[i, L] = new_row[i]
    assert _same_bits(k_cache, want_kc) and torch.equal(rows, want_rows), 'appends as bp_sense_decode'
    assert _same_bits(weight, weight_before), 'key_weight is never written'
    for i, L in enumerate(lengths):
        keys = torch.cat([kc_before[i, :L], k_new[i:i + 1]])
        content = table[torch.cat([rows_before[i, :L], new_row[i:i + 1]]).long()]
        w = weight[i, :, :L + 1]
        ref = _weighted_ref(q[i], keys, content, w, scale, torch.float32)
        eager = _weighted_ref(q[i], keys, content, w, scale, dtype)
        _within_2x(out[i], ref, eager, f'sense_decode_weighted {shape} {form} {dtype} L={L}')
    again = bp.sense_decode(q, k_new, k_cache, table, rows, new_row, seqlens, scale, key_weight=weight)
    assert torch.equal(again, out), 'repeated calls must be bit-identical'
    ones = torch.ones_like(weight)
    for i, L in enumerate(lengths):
        ones[i, :, L + 1:] = NAN
    plain = bp.sense_decode(q, k_new, k_cache, table, rows, new_row, seqlens, scale)
    unit = bp.sense_decode(q, k_new, k_cache, table, rows, new_row, seqlens, scale, key_weight=ones)
    assert torch.equal(unit, plain), 'key_weight = 1 is bp_sense_decode bit for bit'


NEEDLE_CASES = [c for c in N.SENSE_CASES if (c['dkp'], c['k'], c['dout']) in
                {(16, 20, 16), (24, 16, 104), (24, 16, 384), (48, 16, 768), (160, 4, 640), (640, 1, 640)}]
NEEDLE_LENGTHS = (63, 64, 65, 1000, 4096)


def _needle_weight(b, k, max_s):
    """2^e, e in -2 .. 2 a fixed function of (sample, sense, position) that moves with every step along the senses (by 2
    mod 5) and along the positions (by 3 mod 5): a weight taken from a neighbour changes the exact answer."""
    e = (_ar(b)[:, None, None] * 7 + _ar(k)[None, :, None] * 2 + _ar(max_s)[None, None, :] * 3) % 5 - 2
    return torch.exp2(e.float())


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('form', ['table', 'cache'])
@pytest.mark.parametrize('case', NEEDLE_CASES, ids=[f"dk{c['dk']}of{c['dkp']}_k{c['k']}_dout{c['dout']}" for c in NEEDLE_CASES])
def test_sense_decode_weighted_sees_exactly_keys_and_weights_0_to_L(case, form, dtype):
    """out[b] == sum_l w[b, l, j*] table[row(b, j*_{b,l}), l] bit for bit (exact in fp32, rounded once), a different needle
    per (sample, sense), at the tile and split borders.  Key-cache rows >= L and weights > L hold NaN, the table rows no
    visible index names hold NaN."""
    bp = _bp()
    dkp, dk, k, dout, b, max_s = (case[x] for x in ('dkp', 'dk', 'k', 'dout', 'batch', 'max_seqlen'))
    nsplit = bp.lib().bp_sense_decode_ws_floats(b, k, dout, max_s) // (b * k * (dout + 2))
    pos, bi, li = _ar(max_s), _ar(b)[:, None], _ar(k)[None, :]
    keys = N.code(pos, dk, dkp).to(dtype)
    table_rows = N.VOCAB if form == 'table' else b * max_s
    table_clean = N.sense_value(_ar(table_rows)[:, None], li, dout).to(dtype)
    rows_clean = N.sense_row(case, form, bi, pos[None, :])
    weight_clean = _needle_weight(b, k, max_s)
    k_cache = torch.empty(b, max_s, k, dkp, device=DEV, dtype=dtype)
    scale = N.scale(dk)
    top = min(N.max_length(dk), max_s - 8)
    for L in [L for L in NEEDLE_LENGTHS if L <= top]:
        k_cache.copy_(keys[None, :, None, :].expand_as(k_cache))
        k_cache[:, L:] = NAN
        k_new = keys[L].expand(b, k, dkp).contiguous()
        new_row = rows_clean[:, L].contiguous()
        rows = rows_clean.clone()
        rows[:, L:] = -1
        named = torch.zeros(table_rows, dtype=torch.bool, device=DEV)
        named[rows_clean[:, :L + 1].long().flatten()] = True
        table = table_clean.clone()
        table[~named] = NAN
        weight = weight_clean.clone()
        weight[:, :, L + 1:] = NAN
        weight_before = weight.clone()
        seqlens = torch.full((b,), L, dtype=torch.int32, device=DEV)
        for call in N.assign(N.needle_positions(L, nsplit), b * k):
            jstar = torch.tensor(call, device=DEV).view(b, k)
            q = N.code(jstar, dk, dkp).to(dtype)
            k_cache[:, L] = NAN
            rows[:, L] = -1
            out = bp.sense_decode(q, k_new, k_cache, table, rows, new_row, seqlens, scale, key_weight=weight)
            r = N.sense_row(case, form, bi, jstar).long()
            w = weight_clean[bi, li, jstar]                                          # (b, k)
            want = (table_clean[r, li].float() * w[:, :, None]).sum(dim=1).to(dtype)
            bad = (out != want).any(dim=-1)
            assert not bad.any(), (f'{case} {form} {dtype} nsplit={nsplit} L={L}: wrong samples '
                                   f'{bad.nonzero().flatten().tolist()} of needles {jstar[bad].tolist()}')
            assert torch.equal(rows[:, L], new_row) and _same_bits(k_cache[:, L], k_new), f'{case} L={L}: appends'
        assert _same_bits(weight, weight_before)


# ---- bp_sense_rows_dot -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('form', ['table', 'cache'])
@pytest.mark.parametrize('shape', SENSE_SHAPES, ids=SHAPE_IDS)
def test_sense_rows_dot_matches_fp64(shape, form, dtype):
    """out[b, l, j] = table[row(b, j), l] . vec[b] for j <= L_b: within 2 x the error of the fp32 product of the same 16-bit
    inputs (+ 1e-5 of the largest result); position L_b takes new_row (row_index[b, >= L_b] names rows outside the table,
    which would clamp to the last row); cached rows outside the table clamp to the last row; nothing else is written."""
    bp = _bp()
    dkp, dk, k, dout = shape
    g = torch.Generator(device=DEV).manual_seed(dkp * 11 + k)
    lengths, _, _, _, table, rows, new_row, seqlens = _operands(shape, form, dtype, g)
    b, max_s = rows.shape
    vec = torch.randn(b, dout, device=DEV, generator=g).to(dtype)
    assert bp.sense_rows_dot_supported(table, vec)
    bad = torch.tensor([-1, table.shape[0], 2 ** 31 - 1, -(2 ** 31)], dtype=torch.int32, device=DEV)
    for i, L in enumerate(lengths):
        rows[i, L:] = bad[(_ar(max_s - L) + i) % 4]
        if L >= 8:
            rows[i, 3], rows[i, L - 1] = bad[i % 4], bad[(i + 1) % 4]        # cached rows outside the table: the last row
    rows_before = rows.clone()
    sentinel = -12345.0
    out = torch.full((b, k, max_s), sentinel, device=DEV)
    bp.sense_rows_dot(table, rows, new_row, seqlens, vec, out)
    torch.cuda.synchronize()
    assert torch.equal(rows, rows_before), 'row_index is only read'
    for i, L in enumerate(lengths):
        idx = torch.cat([rows_before[i, :L], new_row[i:i + 1]]).long()
        idx = torch.where((idx < 0) | (idx >= table.shape[0]), table.shape[0] - 1, idx)
        content = table[idx]                                                   # (L + 1, k, dout)
        ref = torch.einsum('jld,d->lj', content.double(), vec[i].double())
        base = (torch.einsum('jld,d->lj', content.float(), vec[i].float()).double() - ref).abs().max().item()
        err = (out[i, :, :L + 1].double() - ref).abs().max().item()
        print(f'rows_dot {shape} {form} {dtype} L={L}: kernel {err:.3e} fp32 torch {base:.3e} max|ref| {ref.abs().max().item():.3e}')
        assert err <= 2 * base + 1e-5 * ref.abs().max().item(), (shape, form, dtype, L, err, base)
        assert (out[i, :, L + 1:] == sentinel).all(), 'entries past L are left untouched'
    again = torch.full_like(out, sentinel)
    bp.sense_rows_dot(table, rows, new_row, seqlens, vec, again)
    assert torch.equal(again, out), 'repeated calls must be bit-identical'


# ---- model level -------------------------------------------------------------------------------------------------------

WRAPPERS = ['weighted', 'weighted-anneal', 'replaced']


def _wrappers(kind, model, twin, ids, lengths, words=()):
    """The HIP wrapper and its fp32 twin, same intervention."""
    from src.models.intervened_models import ReplacedWordLMHeadModel, WeightedBackpackLMHeadModel
    cfg = model.config
    g = torch.Generator().manual_seed(11)
    if kind == 'replaced':
        senses = {int(w): torch.randn(cfg.num_content_vectors, cfg.n_embd, generator=g).bfloat16().float() * 0.25
                  for w in words}
        return (ReplacedWordLMHeadModel(model, {w: s.to(DEV, torch.bfloat16) for w, s in senses.items()}).eval(),
                ReplacedWordLMHeadModel(twin, {w: s.to(DEV) for w, s in senses.items()}).eval())
    cw = (torch.rand(model.lm_head.weight.shape[0], cfg.num_content_vectors, generator=g) * 3).to(DEV)
    anneal = kind == 'weighted-anneal'
    scale = _anneal_scale(twin, ids, lengths) if anneal else 0.1
    return tuple(WeightedBackpackLMHeadModel(m, cw, None, scale, anneal=anneal, upweight_nearby=True).eval()
                 for m in (model, twin))


@pytest.mark.parametrize('kind', WRAPPERS)
@pytest.mark.parametrize('mode', ['cached', 'off'])
@pytest.mark.parametrize('name', ['small', 'mini_k4'])
def test_cached_intervened_decode_matches_the_fp32_twin(name, mode, kind):
    """Prefill 16 + 64 cached steps of each wrapper ('cached': table form where the wrapper allows it, 'off': cache form).
    Every step's logits against the fp32 twin wrapper on the full prefix: within max(2^-7 max|ref|, 3 x base), base = the
    error of the uncached HIP forward of the same wrapper (tests/test_gpu_decode.py::test_cached_decode_matches_the_full_forward)."""
    from src.utils.generation import InferenceParams
    model = _model(name)
    model.transformer.sense_table_mode = mode
    twin = _fp32_twin(model)
    prompt, steps, b = 16, 64, 2
    ids = torch.randint(0, VOCAB, (b, prompt + steps), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    lengths = range(prompt + 1, prompt + steps + 1)
    wrapper, ref_wrapper = _wrappers(kind, model, twin, ids, lengths, words=(ids[0, 3], ids[1, prompt + 9]))
    if kind == 'weighted-anneal':
        _assert_scores_in_band(twin, ids, wrapper.annealing_scale, lengths)
    ip = InferenceParams(max_sequence_len=prompt + steps, max_batch_size=b)
    ip.lengths_per_sample = torch.zeros(b, dtype=torch.int32, device=DEV)
    with torch.inference_mode():
        wrapper(ids[:, :prompt], inference_params=ip)
        table_form = 'backpack_content' not in ip.key_value_memory_dict
        assert table_form == (mode == 'cached' and kind != 'replaced')
        ip.sequence_len_offset = prompt
        ip.lengths_per_sample.fill_(prompt)
        worst = 0.0
        for t in range(prompt, prompt + steps):
            got = wrapper(ids[:, t:t + 1], inference_params=ip).logits[:, -1].float()
            ip.lengths_per_sample += 1
            ip.sequence_len_offset += 1
            full = wrapper(ids[:, :t + 1]).logits[:, -1].float()
            ref = ref_wrapper(ids[:, :t + 1]).logits[:, -1]
            err, base = (got - ref).abs().max().item(), (full - ref).abs().max().item()
            bound = max(2 ** -7 * ref.abs().max().item(), 3 * base)
            worst = max(worst, err / bound)
            assert err <= bound, (name, mode, kind, t, err, base, ref.abs().max().item())
    print(f'{name} [{mode}] {kind}: worst step error {worst:.2f} of the bound')


def test_plain_model_step_launches_what_it_launched():
    """No hook: the plain model's cached step calls bp_hip.sense_decode once without key weights and never
    bp_hip.sense_rows_dot."""
    from src.utils.generation import InferenceParams
    bp = _bp()
    model = _model('small')
    ids = torch.randint(0, VOCAB, (2, 17), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    ip = InferenceParams(max_sequence_len=17, max_batch_size=2)
    boom = mock.Mock(side_effect=AssertionError('bp_sense_rows_dot reached from the plain model'))
    with torch.inference_mode(), mock.patch.object(bp, 'sense_rows_dot', boom), \
            mock.patch.object(bp, 'sense_decode', side_effect=bp.sense_decode) as spy:
        model(ids[:, :16], inference_params=ip)
        ip.sequence_len_offset = 16
        model(ids[:, 16:], inference_params=ip)
    assert spy.call_count == 1 and not boom.called
    args, kwargs = spy.call_args
    assert inspect.signature(bp.sense_decode).bind(*args, **kwargs).arguments.get('key_weight') is None


def test_annealed_graph_replay_is_bit_identical_to_eager_steps():
    """One captured step of the annealed Weighted wrapper replayed N times gives the eager cached steps' logits bit for bit
    (the running sums, the weights and the length all advance inside the graph)."""
    from src.utils.generation import InferenceParams
    model = _model('small', seed=2)
    twin = _fp32_twin(model)
    prompt, steps, b = 16, 24, 3
    ids = torch.randint(0, VOCAB, (b, prompt + steps), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    lengths = range(prompt + 1, prompt + steps + 1)
    wrapper, _ = _wrappers('weighted-anneal', model, twin, ids, lengths)
    _assert_scores_in_band(twin, ids, wrapper.annealing_scale, lengths)

    def fresh():
        ip = InferenceParams(max_sequence_len=prompt + steps, max_batch_size=b)
        ip.lengths_per_sample = torch.zeros(b, dtype=torch.int32, device=DEV)
        wrapper(ids[:, :prompt], inference_params=ip)
        ip.sequence_len_offset = prompt
        ip.lengths_per_sample.fill_(prompt)
        return ip

    with torch.inference_mode():
        ip = fresh()
        eager = []
        for t in range(prompt, prompt + steps):
            eager.append(wrapper(ids[:, t:t + 1], inference_params=ip).logits[:, -1].clone())
            ip.lengths_per_sample += 1
        ip = fresh()
        first = wrapper(ids[:, prompt:prompt + 1], inference_params=ip).logits[:, -1].clone()
        ip.lengths_per_sample += 1
        static_ids = ids[:, prompt + 1:prompt + 2].clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_logits = wrapper(static_ids, inference_params=ip).logits[:, -1]
            ip.lengths_per_sample += 1
        replayed = [first]
        for t in range(prompt + 1, prompt + steps):
            static_ids.copy_(ids[:, t:t + 1])
            graph.replay()
            replayed.append(static_logits.clone())
    for i, (a, r) in enumerate(zip(eager, replayed)):
        assert torch.equal(a, r), f'step {i}'


@pytest.mark.parametrize('kind', WRAPPERS)
def test_wrapper_generate_and_sample_with_kv_cache(kind):
    """sample / generate(kv_cache=True, cg=True) on a wrapper return (batch, max_length - 1) with the prompt intact; the
    greedy tokens equal the uncached generate()'s up to the first step whose top-2 margin is within the difference
    between the cached and the full-forward logits there (tests/test_gpu_decode.py::test_generate_with_kv_cache_follows_generate)."""
    model = _model('small', seed=4)
    with torch.no_grad():
        model.lm_head.weight.mul_(4.0)
    twin = _fp32_twin(model)
    prompt, max_length = 16, 96
    ids = torch.randint(0, VOCAB, (4, prompt), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    plain = model.generate(ids, max_length)
    lengths = range(prompt, max_length, 8)
    wrapper, _ = _wrappers(kind, model, twin, plain, lengths, words=(ids[0, 3], plain[1, prompt + 9]))
    full = wrapper.generate(ids, max_length)
    if kind == 'weighted-anneal':
        _assert_scores_in_band(twin, full, wrapper.annealing_scale, lengths)
    cached = wrapper.generate(ids, max_length, kv_cache=True, cg=True)
    assert full.shape == cached.shape == (4, max_length - 1)
    assert torch.equal(cached[:, :prompt], ids)
    drawn = wrapper.sample(ids, max_length, kv_cache=True, cg=True)
    assert drawn.shape == (4, max_length - 1) and torch.equal(drawn[:, :prompt], ids)
    assert int(drawn.min()) >= 0 and int(drawn.max()) < model.lm_head.weight.shape[0]
    for b in range(4):
        diff = (full[b] != cached[b]).nonzero()
        if diff.numel() == 0:
            continue
        col = diff[0].item()
        with torch.inference_mode():
            logits = wrapper(full[b:b + 1, :col]).logits[0, -1].float()
        top2 = logits.topk(2).values
        margin = (top2[0] - top2[1]).item()
        gap = (_cached_logits(wrapper, full[b:b + 1, :col], prompt) - logits).abs().max().item()
        assert margin <= 2 * gap, (kind, b, col, margin, gap)
