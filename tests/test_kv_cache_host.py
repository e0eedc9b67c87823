"""CPU: KV-cached decoding (InferenceParams) on the eager twins of the GPT trunk and the Backpack, the C ABI of the two
decode kernels (argument checks before any device work), and the register account of their code objects."""
import ctypes
import os
import sys

import pytest
import torch

from conftest import ROOT

import bp_hip
import decode_needles as N
from decode_support import PROMPT, STEPS
from decode_support import _close_fp32 as _close
from decode_support import _nano_backpack as _backpack
from flash_attn.models.gpt import GPTLMHeadModel
from src.utils.generation import InferenceParams
from transformers import GPT2Config

def _gpt(seed=0):
    torch.manual_seed(seed)
    cfg = GPT2Config(n_embd=128, n_head=4, n_layer=2, vocab_size=200, n_positions=64, resid_pdrop=0.0, embd_pdrop=0.0,
                     attn_pdrop=0.0, scale_attn_by_inverse_layer_idx=True, use_flash_attn=False)
    model = GPTLMHeadModel(cfg).eval()
    with torch.no_grad():
        for layer in model.transformer.layers:
            layer.mixer.Wqkv.weight.mul_(6.0)      # sharp attention: the cache has to be right, not just near uniform
    return model


def _model(kind):
    return _gpt() if kind == 'gpt' else _backpack()


@pytest.mark.parametrize('kind', ['gpt', 'backpack'])
def test_cached_steps_match_the_full_forward(kind):
    """Prompt 7, then 20 cached steps: the prefill's rows and every step's logits equal the full forward's last row."""
    model = _model(kind)
    ids = torch.randint(0, 200, (2, PROMPT + STEPS), generator=torch.Generator().manual_seed(1))
    ip = InferenceParams(max_sequence_len=PROMPT + STEPS, max_batch_size=2)
    with torch.inference_mode():
        _close(model(ids[:, :PROMPT], inference_params=ip).logits, model(ids[:, :PROMPT]).logits, 'prefill')
        ip.sequence_len_offset = PROMPT
        for t in range(PROMPT, PROMPT + STEPS):
            got = model(ids[:, t:t + 1], inference_params=ip).logits
            assert got.shape == (2, 1, model.lm_head.weight.shape[0])
            _close(got[:, -1], model(ids[:, :t + 1]).logits[:, -1], f'step {t}')
            ip.sequence_len_offset += 1


@pytest.mark.parametrize('kind', ['gpt', 'backpack'])
def test_per_sample_lengths_on_the_device(kind):
    """Two prompts of different lengths prefilled at their own batch_size_offset, then decoded together: the lengths come
    from `lengths_per_sample` (device int32) and are advanced by the caller."""
    model = _model(kind)
    g = torch.Generator().manual_seed(2)
    seqs = [torch.randint(0, 200, (1, 5 + 6), generator=g), torch.randint(0, 200, (1, 9 + 6), generator=g)]
    prompts = [5, 9]
    ip = InferenceParams(max_sequence_len=16, max_batch_size=2)
    ip.lengths_per_sample = torch.zeros(2, dtype=torch.int32)
    with torch.inference_mode():
        for b, (seq, p) in enumerate(zip(seqs, prompts)):
            ip.batch_size_offset, ip.sequence_len_offset = b, 0
            model(seq[:, :p], inference_params=ip)
        ip.batch_size_offset, ip.sequence_len_offset = 0, 1
        ip.lengths_per_sample.copy_(torch.tensor(prompts, dtype=torch.int32))
        for step in range(6):
            tok = torch.cat([seq[:, p + step:p + step + 1] for seq, p in zip(seqs, prompts)])
            got = model(tok, inference_params=ip).logits[:, -1]
            ip.lengths_per_sample += 1
            for b, (seq, p) in enumerate(zip(seqs, prompts)):
                _close(got[b], model(seq[:, :p + step + 1]).logits[0, -1], f'sample {b} step {step}')


def test_reference_greedy_decode_loop_on_gpt():
    """The reference's greedy_decode (flash_attn/utils/generation.py:23-55), restated: prefill, then one token per call
    with explicit position_ids; its tokens equal argmax decoding on the full forward."""
    model = _gpt(seed=4)
    input_ids = torch.randint(0, 200, (3, PROMPT), generator=torch.Generator().manual_seed(5))
    max_length = PROMPT + STEPS
    batch_size, seqlen_og = input_ids.shape
    inference_params = InferenceParams(max_sequence_len=max_length, max_batch_size=batch_size)
    with torch.inference_mode():
        logits = model(input_ids, inference_params=inference_params).logits[:, -1]
        next_token = logits.argmax(dim=-1)
        sequences = [next_token]
        inference_params.sequence_len_offset = seqlen_og
        while True:
            position_ids = torch.full((batch_size, 1), inference_params.sequence_len_offset, dtype=torch.long)
            logits = model(next_token.unsqueeze(1), position_ids=position_ids,
                           inference_params=inference_params).logits[:, -1]
            next_token = logits.argmax(dim=-1)
            sequences.append(next_token)
            inference_params.sequence_len_offset += 1
            if inference_params.sequence_len_offset >= max_length - 1:
                break
        cached = torch.cat([input_ids, torch.stack(sequences, dim=1)], dim=1)
        full = input_ids
        while full.shape[1] < cached.shape[1]:
            full = torch.cat([full, model(full).logits[:, -1].argmax(dim=-1, keepdim=True)], dim=1)
    assert torch.equal(cached, full)


def test_cache_tensors_have_the_reference_layout():
    """key_value_memory_dict[layer_idx]: (max_batch, max_seqlen, 2, nheads, head_dim), K then V of the prompt at rows
    [0, S) (mha.py _update_kv_cache); the Backpack's sense keys and row index under keys of their own."""
    model = _backpack()
    ids = torch.randint(0, 200, (2, PROMPT), generator=torch.Generator().manual_seed(6))
    ip = InferenceParams(max_sequence_len=30, max_batch_size=3)
    with torch.inference_mode():
        model(ids, inference_params=ip)
        trunk = model.transformer.gpt2_model
        x = trunk.ln_0(trunk.embeddings(ids))
        qkv = trunk.layers[0].mixer.Wqkv(x).unflatten(-1, (3, 6, 64))
        qk = model.transformer.contextualization_attn.project(trunk(ids))
    caches = ip.key_value_memory_dict
    for i in range(2):
        assert caches[i].shape == (3, 30, 2, 6, 64) and caches[i].dtype == torch.float32
    torch.testing.assert_close(caches[0][:2, :PROMPT], qkv[:, :, 1:], rtol=0, atol=1e-6)
    assert caches['backpack_sense_k'].shape == (3, 30, 16, 24)
    torch.testing.assert_close(caches['backpack_sense_k'][:2, :PROMPT], qk[:, :, 1], rtol=0, atol=1e-5)
    rows = caches['backpack_rows']
    assert rows.shape == (3, 30) and rows.dtype == torch.int32
    # off the HIP path there is no sense table: cache form, row = b * max_seqlen + j into the per-position content cache
    assert torch.equal(rows[:2, :PROMPT], (torch.arange(2)[:, None] * 30 + torch.arange(PROMPT)).int())
    assert caches['backpack_content'].shape == (3 * 30, 16, 384)


@pytest.mark.parametrize('kind', ['gpt', 'backpack'])
def test_multi_token_continuation_and_autograd_raise(kind):
    model = _model(kind)
    ids = torch.randint(0, 200, (1, PROMPT))
    ip = InferenceParams(max_sequence_len=20, max_batch_size=1)
    with torch.inference_mode():
        model(ids, inference_params=ip)
        ip.sequence_len_offset = PROMPT
        with pytest.raises(NotImplementedError, match='one new token'):
            model(ids[:, :2], inference_params=ip)
    with pytest.raises(RuntimeError, match='inference-only'):
        model(ids[:, :1], inference_params=ip)


def test_generate_with_kv_cache_equals_generate():
    model = _backpack(seed=7)
    ids = torch.randint(0, 200, (2, PROMPT), generator=torch.Generator().manual_seed(8))
    want = model.generate(ids, PROMPT + STEPS, return_dict_in_generate=True, output_scores=True)
    got = model.generate(ids, PROMPT + STEPS, return_dict_in_generate=True, output_scores=True, kv_cache=True)
    assert got.sequences.shape == (2, PROMPT + STEPS - 1)
    assert torch.equal(got.sequences, want.sequences)
    assert len(got.scores) == 1
    _close(got.scores[0], want.scores[0], 'first scores')
    # prompt longer than max_length: nothing is decoded beyond the first pick, as upstream
    assert torch.equal(model.generate(ids, 3, kv_cache=True), model.generate(ids, 3))


def test_decode_entry_points_reject_bad_arguments_before_any_launch():
    h = bp_hip.lib()
    p = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first
    odd = ctypes.c_void_p(0x1008)
    null = None
    assert h.bp_flash_decode_ws_floats(1, 12, 64, 1024) > 0
    assert h.bp_flash_decode_ws_floats(0, 12, 64, 1024) == 0
    ws = h.bp_flash_decode_ws_floats(1, 12, 64, 1024)

    def flash(q=p, kv=p, lse=null, wsp=p, ws_floats=ws, b=1, hd=64, scale=0.125, dtype=1, strides=64):
        return h.bp_flash_decode(q, p, p, kv, p, p, lse, wsp, ws_floats, b, 12, hd, 1024,
                                 *([strides] * 12), 12, scale, dtype, null)
    assert flash(dtype=7) == -1
    assert flash(hd=136, strides=136) == -2
    assert flash(hd=60, strides=64) == -2            # 16-byte chunks only
    assert flash(b=0) == -3
    assert flash(q=null) == -3
    assert flash(kv=odd) == -3                       # unaligned
    assert flash(strides=68) == -3
    assert flash(scale=0.0) == -4
    assert flash(scale=float('nan')) == -4
    assert flash(ws_floats=ws - 1) == -9
    assert flash(wsp=null) == -3

    sws = h.bp_sense_decode_ws_floats(1, 16, 768, 1024)
    assert sws > 0 and h.bp_sense_decode_ws_floats(1, 16, 0, 1024) == 0

    def sense(q=p, table=p, idx=p, b=1, k=16, dk=48, dout=768, rows=50264, ws_floats=sws, scale=0.144, dtype=1,
              strides=48):
        return h.bp_sense_decode(q, p, p, table, idx, p, p, p, p, ws_floats, b, k, dk, dout, 1024, rows,
                                 *([strides] * 9), 1024, strides, scale, dtype, null)
    assert sense(dtype=2) == -1                      # fp32 is for the cross entropy only
    assert sense(dk=648) == -2
    assert sense(dk=10) == -2                        # callers pad d_k to a multiple of 8 (ContextSelfAttn.project)
    assert sense(dout=0) == -6
    assert sense(dout=12) == -3
    assert sense(k=65) == -3
    assert sense(rows=0) == -3
    assert sense(idx=null) == -3
    assert sense(table=odd) == -3
    assert sense(strides=44) == -3
    assert sense(scale=-1.0) == -4
    assert sense(ws_floats=sws - 1) == -9


def test_python_wrappers_refuse_host_tensors():
    q = torch.zeros(1, 2, 64, dtype=torch.bfloat16)
    assert not bp_hip.flash_decode_supported(q, torch.zeros(1, 8, 2, 2, 64, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.flash_decode(q, q, q, torch.zeros(1, 8, 2, 2, 64, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.int32))


def _needle_rows(positions, cap=24):
    """Every distinct needle of a case once (at most `cap`, spread evenly, ends kept)."""
    if len(positions) <= cap:
        return positions
    step = (len(positions) - 1) / (cap - 1)
    return sorted({positions[round(i * step)] for i in range(cap)})


def _assert_needles_exact(q, keys, vals, scale, want, dtypes, what, senses=0):
    for ref in (N.attend_fp32, N.attend_splitwise):
        got = ref(q, keys, vals, scale)
        assert torch.equal(got, want), (what, ref.__name__, (got - want).abs().max().item())
    if senses:   # an output row is the sum over its senses AND their keys, the ~1e-20 of the other keys included
        p = torch.softmax(scale * (q @ keys.T), dim=-1)
        for pg, vg, wg in zip(p.split(senses), vals.split(senses), want.split(senses)):
            assert torch.equal(torch.einsum('ln,lnw->w', pg, vg), wg.sum(dim=0)), what
    for dtype in dtypes:   # every operand is exact in both 16-bit types
        for t in (q, keys, vals):
            assert torch.equal(t.to(dtype).float(), t), (what, dtype)


def test_needle_construction_is_exact_in_fp32():
    """The inputs of tests/test_gpu_decode_edges.py section A (tests/decode_needles.py): for every collected case and every
    cache length, on a spread sample of at most 24 of the GPU test's needle positions (ends kept), the plain fp32 softmax
    reference and a split-wise online-softmax restatement both return the needle's value row bit for bit (trunk), and the
    senses' rows sum exactly.  Exactness rests on the score gap and on integer values, not on the position, the column or
    which output row carries a needle: so a sample of positions, the first 32 value columns, and rows dealt round-robin
    (the GPU test deals them with decode_needles.assign) keep this check to a few seconds."""
    h = bp_hip.lib()
    dtypes = (torch.bfloat16, torch.float16)
    checked = 0
    for case in N.TRUNK_CASES:
        d, b, nh, ms = case['d'], case['batch'], case['heads'], case['max_seqlen']
        nsplit = h.bp_flash_decode_ws_floats(b, nh, d, ms) // (b * nh * (d + 2))
        assert nsplit == {'split64': 64, 'split8': 8, 'split1': 1}[case['regime']]
        for L in N.lengths(nsplit, d, ms):
            needles = _needle_rows(N.needle_positions(L, nsplit))
            pos = torch.arange(L + 1)
            keys = N.code(pos, d)
            jstar = torch.tensor(needles)
            rows = torch.arange(len(needles)) % (b * nh)             # (sample, head) of the row carrying each needle
            vals = N.values(N.trunk_value_ids(case, rows[:, None] // nh, rows[:, None] % nh, pos[None]), min(d, 32))
            want = vals[torch.arange(len(needles)), jstar]
            _assert_needles_exact(N.code(jstar, d), keys, vals, N.scale(d), want, dtypes, (case, L))
            checked += len(needles)
    for case in N.SENSE_CASES:
        dkp, dk, k, dout, b, ms = (case[x] for x in ('dkp', 'dk', 'k', 'dout', 'batch', 'max_seqlen'))
        nsplit = h.bp_sense_decode_ws_floats(b, k, dout, ms) // (b * k * (dout + 2))
        w = min(dout, 32)
        for form in ('table', 'cache'):
            for L in N.lengths(nsplit, dk, ms):
                needles = _needle_rows(N.needle_positions(L, nsplit))
                pos = torch.arange(L + 1)
                keys = N.code(pos, dk, dkp)
                jstar = torch.tensor(needles)
                rows = torch.arange(len(needles)) % (b * k)          # (sample, sense) of the row carrying each needle
                table_rows = N.sense_row(case, form, rows[:, None] // k, pos[None])
                vals = N.sense_value(table_rows, rows[:, None] % k, w)
                want = vals[torch.arange(len(needles)), jstar]
                _assert_needles_exact(N.code(jstar, dk, dkp), keys, vals, N.scale(dk), want, dtypes, (case, form, L), senses=k)
                checked += len(needles)
    # the sum over 64 senses of integers up to 8 is an exact fp32 integer (|sum| <= 512 < 2^24) in any order
    assert checked > 3000


@pytest.fixture(scope='module')
def decode_objects():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_resources as KR
    if not KR.tools_available() or not os.path.exists(os.path.join(KR.LLVM, 'llvm-objdump')):
        pytest.skip('LLVM tools not found under /opt/rocm')
    import importlib.util
    spec = importlib.util.spec_from_file_location('bp_build_hip', os.path.join(ROOT, 'backpacks-flash-attn_amd',
                                                                                'build_hip.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()   # no-op when the objects are current
    return [os.path.join(KR.BUILD, o) for o in ('flash_decode.o', 'sense_decode.o')]


def test_decode_kernels_use_no_scratch(decode_objects):
    """Every shipped instantiation of the two decode kernels (each d_k bucket, both dtypes, split and combine)."""
    import kernel_resources as KR
    ks = KR.kernels(decode_objects)
    names = {k['name'] for k in ks}
    assert 'decode_split_kernel<BF16, 8, 1, false>' in names          # Small trunk, d_h = 64
    assert 'decode_split_kernel<BF16, 64, 2, true>' in names          # Mini k = 1, d_k = 640
    assert 'decode_combine_kernel<F16, true>' in names
    assert len(ks) == 2 * (5 + 1) + 2 * (8 + 1)
    for k in ks:   # (SGPR spills of the widest senses go to VGPR lanes, not to memory)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, k


def test_decode_kernels_pass_the_hazard_scanner(decode_objects):
    import mfma_hazard_scan as HS
    hits = []
    for obj in decode_objects:
        for name, ins in HS.functions(HS.disassemble(obj)):
            hits += HS.scan(name, ins)
    assert hits == []
