"""CPU: the packed prefill (generate / sample with packed_prefill=True, bp_scatter_packed_rows) where no GPU is needed -- the
entry point in the header, the ctypes table and the library, the binding's refusal of host tensors, the argument checks of
the keyword, the refusal of the sense-intervened wrappers, and the fallback to the padded prefill on a model that takes no
packed one (the nano fp32 model: use_flash_attn=False)."""
import ctypes
import re
import warnings

import pytest
import torch

import bp_hip
from conftest import ROOT
from decode_support import _nano_backpack as _backpack
from ragged_support import BATCH, LENGTHS, MAX_LENGTH, S

VOCAB = 200


@pytest.fixture(scope='module')
def nano():
    model = _backpack()
    ids = torch.randint(0, VOCAB, (BATCH, S), generator=torch.Generator().manual_seed(1))
    return model, ids


def test_header_table_and_library_agree_on_the_new_entry_point():
    import os
    text = open(os.path.join(ROOT, 'include', 'bp_hip.h')).read()
    assert re.search(r'#define BP_ABI_VERSION 11\b', text) and bp_hip.ABI_VERSION == 11
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    found = re.findall(r'\bint\s+bp_scatter_packed_rows\s*\(([^)]*)\)\s*;', text)
    assert len(found) == 1
    params = [' '.join(re.sub(r'\w+$', '', p).split()) for p in found[0].split(',')]
    restype, argtypes = bp_hip.SIGNATURES['bp_scatter_packed_rows']
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 13
    for have, c_type in zip(argtypes, params):
        want = ctypes.c_void_p if c_type.endswith('*') or c_type == 'bp_stream_t' else \
            {'int': ctypes.c_int, 'int64_t': ctypes.c_int64}[c_type]
        assert have is want, c_type
    h = bp_hip.lib()
    assert hasattr(h, 'bp_scatter_packed_rows') and h.bp_abi_version() == 11


def test_argument_validation_returns_before_any_launch():
    h = bp_hip.lib()
    p, null = 0x1000, None

    def call(src=(p,), src_stride=(48,), dst=(0x2000,), batch_stride=(4096,), pos_stride=(32,), row_bytes=(32,), nsets=None,
             cu=ctypes.c_void_p(0x3000), batch=2, total=8, max_seqlen=4, max_positions=4, arrays=True):
        n = len(src) if nsets is None else nsets
        args = [(ctypes.c_void_p * len(src))(*src), (ctypes.c_int64 * len(src))(*src_stride),
                (ctypes.c_void_p * len(src))(*dst), (ctypes.c_int64 * len(src))(*batch_stride),
                (ctypes.c_int64 * len(src))(*pos_stride), (ctypes.c_int64 * len(src))(*row_bytes)]
        if arrays is not True:
            args[arrays] = null
        return h.bp_scatter_packed_rows(*args, n, cu, batch, total, max_seqlen, max_positions, null)
    for kw in (dict(nsets=0), dict(nsets=33), dict(batch=0), dict(batch=65536), dict(cu=null), dict(cu=ctypes.c_void_p(0x3002)),
               dict(src=(0,)), dict(dst=(0,)), dict(src=(0x1002,)), dict(dst=(0x2001,)), dict(src_stride=(50,)),
               dict(batch_stride=(4098,)), dict(pos_stride=(34,), row_bytes=(30,)), dict(row_bytes=(0,)), dict(row_bytes=(2,)),
               dict(row_bytes=(-4,)), dict(src_stride=(28,)), dict(pos_stride=(28,)), dict(src_stride=(-48,)),
               dict(batch_stride=(-4096,)), dict(max_seqlen=-1), dict(max_positions=-1), dict(total=-1)):
        assert call(**kw) == -3, kw
    for i in range(6):
        assert call(arrays=i) == -3, i
    # nothing to write: a successful no-op without a launch (the addresses above are not memory)
    assert call(max_seqlen=0) == 0 and call(max_positions=0) == 0


def test_binding_refuses_cpu_tensors_before_loading_anything(monkeypatch):
    monkeypatch.setattr(bp_hip, 'lib', lambda: pytest.fail('the library was touched'))
    src, dst = torch.zeros(5, 2, 8), torch.zeros(2, 4, 2, 8)
    cu = torch.tensor([0, 2, 5], dtype=torch.int32)
    with pytest.raises(RuntimeError, match='must live on the GPU'):
        bp_hip.scatter_packed_rows([(src, dst)], cu, 3)


def test_packed_prefill_needs_prompt_lengths_and_the_cache(nano):
    model, ids = nano
    for call in (model.generate, model.sample):
        with pytest.raises(ValueError, match='packed_prefill'):
            call(ids, MAX_LENGTH, kv_cache=True, packed_prefill=True)
        with pytest.raises(ValueError, match='kv_cache'):
            call(ids, MAX_LENGTH, prompt_lengths=LENGTHS, packed_prefill=True)
        with pytest.raises(ValueError, match='packed_prefill'):
            call(ids, MAX_LENGTH, packed_prefill=True)
    from src.utils.generation import PickOptions, greedy_decode, sample
    assert 'packed_prefill' not in PickOptions.__dataclass_fields__
    for fn in (greedy_decode, sample):
        with pytest.raises(ValueError, match='packed_prefill'):
            fn(ids, model, MAX_LENGTH, kv_cache=True, packed_prefill=True)


def test_intervened_wrappers_refuse(nano):
    from src.models.intervened_models import ReplacedWordLMHeadModel, WeightedBackpackLMHeadModel
    from src.utils.generation import greedy_decode
    model, ids = nano
    k, d = model.config.num_content_vectors, model.config.n_embd
    g = torch.Generator().manual_seed(11)
    weighted = WeightedBackpackLMHeadModel(model, torch.rand(VOCAB, k, generator=g), None, 0.1, anneal=False).eval()
    replaced = ReplacedWordLMHeadModel(model, {int(ids[1, 2]): torch.randn(k, d, generator=g)}).eval()
    for wrapper in (weighted, replaced):
        for call in (wrapper.generate, wrapper.sample):
            with pytest.raises(NotImplementedError, match='packed_prefill'):
                call(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, packed_prefill=True)
        with pytest.raises(NotImplementedError, match='packed_prefill'):
            greedy_decode(ids, wrapper, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, packed_prefill=True)
        # without the keyword: as before
        assert wrapper.generate(ids, S + 3, kv_cache=True, prompt_lengths=LENGTHS).shape == (BATCH, S + 2)


def test_a_model_without_a_packed_prefill_runs_the_padded_one_and_says_so_once():
    from src.utils.generation import packed_prefill_limit
    model = _backpack()
    ids = torch.randint(0, VOCAB, (BATCH, S), generator=torch.Generator().manual_seed(1))
    assert packed_prefill_limit(model, ids, S) == 'use_flash_attn=False' == model.transformer.packed_limit(ids, S)
    want = model.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, return_dict_in_generate=True)
    with warnings.catch_warnings(record=True) as said:
        warnings.simplefilter('always')
        first = model.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, packed_prefill=True,
                               return_dict_in_generate=True)
    assert len(said) == 1 and 'packed_prefill' in str(said[0].message) and 'use_flash_attn=False' in str(said[0].message)
    with warnings.catch_warnings(record=True) as said:
        warnings.simplefilter('always')
        second = model.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, packed_prefill=True,
                                return_dict_in_generate=True)
        state = torch.tensor([1234, 77], dtype=torch.int64)
        drawn = model.sample(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, packed_prefill=True, rng_state=state, top_k=20)
    assert said == []
    for got in (first, second):
        assert torch.equal(got.sequences, want.sequences) and torch.equal(got.lengths, want.lengths)
    assert torch.equal(drawn, model.sample(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, rng_state=state, top_k=20))
    # the model itself: a packed batch with inference_params stays a ValueError where the packed kernels do not run, and a
    # packed call behind the prompt is one everywhere
    from src.utils.generation import InferenceParams
    from src.utils.packing import pack_sequences
    packed, cu, longest = pack_sequences(ids, list(LENGTHS))
    with torch.no_grad():
        with pytest.raises(ValueError, match='inference_params'):
            model(packed, cu_seqlens=cu, max_seqlen=longest, inference_params=InferenceParams(max_sequence_len=S, max_batch_size=BATCH))
        with pytest.raises(ValueError, match='sequence_len_offset'):
            model(packed, cu_seqlens=cu, max_seqlen=longest,
                  inference_params=InferenceParams(max_sequence_len=S, max_batch_size=BATCH, sequence_len_offset=S))
