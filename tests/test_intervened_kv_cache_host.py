"""CPU: KV-cached decoding of the intervened Backpacks (src/models/intervened_models.py) on the eager path, the C ABI of
bp_sense_decode_weighted / bp_sense_rows_dot (argument checks before any device work), and the register account of their
code objects.

Annealed cases: a freshly initialised model has similarity sums far below 6 / 0.1, so with the default scale every score
is sigmoid(6) and a wrong running sum would go unnoticed.  The scale is therefore 6 / (a middle quantile of the fp32
model's sims over every prefix a test compares), and every annealed test asserts that at least half of the scores it compares (before
`upweight_nearby`) lie in [0.1, 0.9].  content_weights are drawn from [0, 3) so that a dropped weight moves the logits."""
import ctypes
import inspect
import os
import sys
from unittest import mock

import pytest
import torch

from conftest import ROOT

import bp_hip
from decode_support import PROMPT, STEPS, _anneal_scale, _assert_scores_in_band
from decode_support import _close_fp32 as _close
from decode_support import _nano_backpack as _backpack
import src.models.backpack as backpack_module
import src.models.intervened_models as IM
from oracle import ref_cpu as R
from src.models.intervened_models import (NegativeWeightedBackpackLMHeadModel, ReplacedWordLMHeadModel,
                                          WeightedBackpackLMHeadModel)
from src.utils.generation import InferenceParams, greedy_decode

VOCAB, K, D = 200, 16, 384
OCFG = dict(n_embd=D, n_head=6, n_layer=2, num_content_vectors=K, layer_norm_epsilon=1e-5,
            scale_attn_by_inverse_layer_idx=True)
VARIANTS = ['weighted', 'weighted-anneal', 'weighted-anneal-flat', 'replaced']


def _wrapper(variant, model, ids, lengths=range(PROMPT, PROMPT + STEPS + 1), replaced=None):
    g = torch.Generator().manual_seed(11)
    if variant == 'replaced':
        words = replaced if replaced is not None else [int(ids[0, 2]), int(ids[1, PROMPT + 5])]
        return ReplacedWordLMHeadModel(model, {w: torch.randn(K, D, generator=g) * 0.5 for w in words}).eval()
    cw = torch.rand(VOCAB, K, generator=g) * 3
    anneal = variant != 'weighted'
    scale = _anneal_scale(model, ids, lengths) if anneal else 0.1
    return WeightedBackpackLMHeadModel(model, cw, None, scale, anneal=anneal,
                                       upweight_nearby=variant != 'weighted-anneal-flat').eval()


def _oracle(wrapper, ids):
    sd = {k: v.detach() for k, v in wrapper.backpack_network.state_dict().items()}
    if isinstance(wrapper, ReplacedWordLMHeadModel):
        return R.replaced_word_logits(sd, OCFG, ids, wrapper.sense_dict)
    return R.weighted_backpack_logits(sd, OCFG, ids, wrapper.content_weights, wrapper.annealing_scale, wrapper.anneal,
                                      wrapper.upweight_nearby)


@pytest.mark.parametrize('variant', VARIANTS)
def test_cached_steps_match_the_full_forward(variant):
    """Prompt 7, then 20 cached steps: the prefill's rows and every step's logits equal the same wrapper's full forward
    on the prefix, and the CPU oracle's."""
    model = _backpack()
    ids = torch.randint(0, VOCAB, (2, PROMPT + STEPS), generator=torch.Generator().manual_seed(1))
    wrapper = _wrapper(variant, model, ids)
    if variant.startswith('weighted-anneal'):
        _assert_scores_in_band(model, ids, wrapper.annealing_scale, range(PROMPT, PROMPT + STEPS + 1))
    if variant == 'replaced':   # a replaced token in the prompt and one among the decoded positions
        assert int(ids[0, 2]) in wrapper.sense_dict and int(ids[1, PROMPT + 5]) in wrapper.sense_dict
    ip = InferenceParams(max_sequence_len=PROMPT + STEPS, max_batch_size=2)
    with torch.inference_mode():
        full = wrapper(ids[:, :PROMPT]).logits
        _close(wrapper(ids[:, :PROMPT], inference_params=ip).logits, full, 'prefill')
        _close(full, _oracle(wrapper, ids[:, :PROMPT]), 'oracle, prompt')
        ip.sequence_len_offset = PROMPT
        for t in range(PROMPT, PROMPT + STEPS):
            got = wrapper(ids[:, t:t + 1], inference_params=ip).logits
            assert got.shape == (2, 1, VOCAB)
            _close(got[:, -1], wrapper(ids[:, :t + 1]).logits[:, -1], f'step {t}')
            _close(got[:, -1], _oracle(wrapper, ids[:, :t + 1])[:, -1], f'oracle, step {t}')
            ip.sequence_len_offset += 1


@pytest.mark.parametrize('variant', VARIANTS)
def test_per_sample_lengths_on_the_device(variant):
    """Two prompts of different lengths prefilled at their own batch_size_offset, then decoded together on
    `lengths_per_sample`."""
    model = _backpack()
    g = torch.Generator().manual_seed(2)
    seqs = [torch.randint(0, VOCAB, (1, 5 + 6), generator=g), torch.randint(0, VOCAB, (1, 9 + 6), generator=g)]
    prompts = [5, 9]
    both = torch.cat([seqs[0], seqs[1][:, :11]])
    wrapper = _wrapper(variant, model, both, lengths=range(6, 12), replaced=[int(seqs[0][0, 1]), int(seqs[1][0, 12])])
    if variant.startswith('weighted-anneal'):
        _assert_scores_in_band(model, both, wrapper.annealing_scale, range(6, 12))
    ip = InferenceParams(max_sequence_len=16, max_batch_size=2)
    ip.lengths_per_sample = torch.zeros(2, dtype=torch.int32)
    with torch.inference_mode():
        for b, (seq, p) in enumerate(zip(seqs, prompts)):
            ip.batch_size_offset, ip.sequence_len_offset = b, 0
            wrapper(seq[:, :p], inference_params=ip)
        ip.batch_size_offset, ip.sequence_len_offset = 0, 1
        ip.lengths_per_sample.copy_(torch.tensor(prompts, dtype=torch.int32))
        for step in range(6):
            tok = torch.cat([seq[:, p + step:p + step + 1] for seq, p in zip(seqs, prompts)])
            got = wrapper(tok, inference_params=ip).logits[:, -1]
            ip.lengths_per_sample += 1
            for b, (seq, p) in enumerate(zip(seqs, prompts)):
                _close(got[b], wrapper(seq[:, :p + step + 1]).logits[0, -1], f'sample {b} step {step}')


@pytest.mark.parametrize('variant', VARIANTS)
def test_greedy_decode_with_kv_cache_equals_the_uncached_loop(variant):
    model = _backpack(seed=7)
    ids = torch.randint(0, VOCAB, (2, PROMPT), generator=torch.Generator().manual_seed(8))
    plain = greedy_decode(ids, model, PROMPT + STEPS).sequences       # the tokens the annealing scale is taken from
    wrapper = _wrapper(variant, model, plain, lengths=range(PROMPT, PROMPT + STEPS), replaced=[int(ids[0, 2]), int(plain[1, PROMPT + 3])])
    want = greedy_decode(ids, wrapper, PROMPT + STEPS)
    got = greedy_decode(ids, wrapper, PROMPT + STEPS, kv_cache=True)
    if variant.startswith('weighted-anneal'):
        _assert_scores_in_band(model, want.sequences, wrapper.annealing_scale, range(PROMPT, PROMPT + STEPS))
    assert got.sequences.shape == (2, PROMPT + STEPS - 1)
    assert torch.equal(got.sequences, want.sequences)
    _close(got.scores[0], want.scores[0], 'first scores')
    assert torch.equal(wrapper.generate(ids, PROMPT + STEPS, kv_cache=True), want.sequences)


def test_negative_weighted_refuses_a_cache():
    model = _backpack()
    wrapper = NegativeWeightedBackpackLMHeadModel(model, torch.rand(VOCAB, K), None, 0.1).eval()
    ids = torch.randint(0, VOCAB, (1, PROMPT))
    with torch.inference_mode():
        assert wrapper(ids).logits.shape == (1, PROMPT, VOCAB)
        with pytest.raises(NotImplementedError, match='without kv_cache'):
            wrapper(ids, inference_params=InferenceParams(max_sequence_len=20, max_batch_size=1))


def test_plain_model_steps_touch_nothing_of_the_intervention_code():
    """No hook installed: one cached step of the plain BackpackLMHeadModel calls _eager_sense_decode exactly once, with
    no key weights, and none of the new helpers."""
    model = _backpack()
    ids = torch.randint(0, VOCAB, (2, PROMPT + 1), generator=torch.Generator().manual_seed(3))
    ip = InferenceParams(max_sequence_len=PROMPT + 1, max_batch_size=2)
    boom = mock.Mock(side_effect=AssertionError('intervention code reached from the plain model'))
    real = backpack_module._eager_sense_decode
    with torch.inference_mode(), \
            mock.patch.object(IM, '_eager_rows_dot', boom), mock.patch.object(IM, '_anneal_weights', boom), \
            mock.patch.object(IM._Intervened, 'edit_rows', boom), \
            mock.patch.object(IM._Intervened, 'prefill_key_weight', boom), \
            mock.patch.object(IM._Intervened, 'step_key_weight', boom), \
            mock.patch.object(bp_hip, 'sense_rows_dot', boom), \
            mock.patch.object(backpack_module, '_eager_sense_decode', side_effect=real) as spy:
        model(ids[:, :PROMPT], inference_params=ip)
        assert spy.call_count == 0
        ip.sequence_len_offset = PROMPT
        got = model(ids[:, PROMPT:], inference_params=ip).logits[:, -1]
        assert spy.call_count == 1
        args, kwargs = spy.call_args
        assert inspect.signature(real).bind(*args, **kwargs).arguments.get('key_weight') is None
        _close(got, model(ids).logits[:, -1], 'plain step')
    assert not boom.called
    assert set(ip.key_value_memory_dict) == {0, 1, 'backpack_sense_k', 'backpack_rows', 'backpack_content'}


def test_weighted_decode_and_rows_dot_reject_bad_arguments_before_any_launch():
    h = bp_hip.lib()
    assert h.bp_abi_version() == 11 == bp_hip.ABI_VERSION
    p = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first
    odd = ctypes.c_void_p(0x1008)
    null = None
    sws = h.bp_sense_decode_ws_floats(1, 16, 768, 1024)

    def weighted(q=p, table=p, idx=p, kw=p, b=1, k=16, dk=48, dout=768, rows=50264, ws_floats=sws, scale=0.144, dtype=1,
                 strides=48, kw_b=16 * 1024, kw_s=1024):
        return h.bp_sense_decode_weighted(q, p, p, table, idx, p, p, kw, p, p, ws_floats, b, k, dk, dout, 1024, rows,
                                          *([strides] * 9), 1024, strides, kw_b, kw_s, scale, dtype, null)
    assert weighted(dtype=2) == -1
    assert weighted(dk=648) == -2
    assert weighted(dk=10) == -2
    assert weighted(dout=0) == -6
    assert weighted(dout=12) == -3
    assert weighted(k=65) == -3
    assert weighted(rows=0) == -3
    assert weighted(idx=null) == -3
    assert weighted(table=odd) == -3
    assert weighted(strides=44) == -3
    assert weighted(kw_s=1023) == -3                  # weight rows of two senses would overlap
    assert weighted(kw_b=512) == -3
    assert weighted(scale=-1.0) == -4
    assert weighted(ws_floats=sws - 1) == -9
    assert weighted(kw=null, kw_s=0, kw_b=0, ws_floats=sws - 1) == -9   # NULL weights: bp_sense_decode's checks

    def dot(table=p, idx=p, new=p, lens=p, vec=p, out=p, b=1, k=16, dout=768, rows=50264, dtype=1, t_row=16 * 768,
            t_sense=768, v_b=768, o_b=16 * 1024, o_s=1024):
        return h.bp_sense_rows_dot(table, idx, new, lens, vec, out, b, k, dout, 1024, rows, t_row, t_sense, 1024, v_b,
                                   o_b, o_s, dtype, null)
    assert dot(dtype=2) == -1
    assert dot(dout=0) == -6
    assert dot(dout=12) == -3
    assert dot(dout=2056) == -3
    assert dot(k=65) == -3
    assert dot(k=0) == -3
    assert dot(b=0) == -3
    assert dot(rows=0) == -3
    for name in ('table', 'idx', 'new', 'lens', 'vec', 'out'):
        assert dot(**{name: null}) == -3, name
    assert dot(table=odd) == -3
    assert dot(vec=odd) == -3
    assert dot(t_sense=772) == -3
    assert dot(v_b=772) == -3
    assert dot(o_s=1023) == -3
    assert dot(o_b=1000) == -3


def test_python_wrappers_refuse_host_tensors():
    table, vec = torch.zeros(8, 2, 64, dtype=torch.bfloat16), torch.zeros(1, 64, dtype=torch.bfloat16)
    assert not bp_hip.sense_rows_dot_supported(table, vec)
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.sense_rows_dot(table, torch.zeros(1, 8, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                              torch.zeros(1, dtype=torch.int32), vec, torch.zeros(1, 2, 8))
    q = torch.zeros(1, 2, 64, dtype=torch.bfloat16)
    assert not bp_hip.sense_decode_weighted_supported(q, torch.zeros(1, 8, 2, 64, dtype=torch.bfloat16), table,
                                                      torch.zeros(1, 2, 8))


@pytest.fixture(scope='module')
def intervened_objects():
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
    return [os.path.join(KR.BUILD, o) for o in ('sense_decode_weighted.o', 'sense_rows_dot.o')]


def test_intervened_decode_kernels_use_no_scratch(intervened_objects):
    """Every instantiation of the weighted split kernel (each d_k bucket, both dtypes; its combine is sense_decode.o's) and
    of the rows-dot kernel (1 .. 4 row chunks per lane, both dtypes)."""
    import kernel_resources as KR
    ks = KR.kernels(intervened_objects)
    names = {k['name'] for k in ks}
    assert 'decode_split_kernel<Weighted<BF16>, 8, 1, true>' in names     # Small, d_k = 48
    assert 'decode_split_kernel<Weighted<F16>, 64, 2, true>' in names     # Mini k = 1, d_k = 640
    assert 'sense_rows_dot_kernel<BF16, 2>' in names                      # d_out = 768
    assert len(ks) == 2 * 8 + 2 * 4
    for k in ks:
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, k
        if k['name'].startswith('decode_split_kernel'):
            assert k['group_segment_fixed_size'] == 10240, k             # one more [2][64] fp32 array than the plain 9728


def test_intervened_decode_kernels_pass_the_hazard_scanner(intervened_objects):
    import mfma_hazard_scan as HS
    hits = []
    for obj in intervened_objects:
        for name, ins in HS.functions(HS.disassemble(obj)):
            hits += HS.scan(name, ins)
    assert hits == []
