"""CPU: bp_sense_anneal_step's argument checks, the flag fused_anneal_step on a CPU model, the new code object's registers."""
import ctypes
import os
import sys

import pytest
import torch

from conftest import ROOT

import bp_hip
from decode_support import PROMPT, _nano_backpack
from src.models.intervened_models import WeightedBackpackLMHeadModel
from src.utils.generation import InferenceParams


def test_anneal_step_rejects_bad_arguments_before_any_launch():
    h = bp_hip.lib()
    p, odd, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008), None   # never dereferenced: validation fails first
    ws = h.bp_sense_anneal_step_ws_floats(2, 16, 1000)
    assert ws == 2 * 63 * 16 and h.bp_sense_anneal_step_ws_floats(0, 16, 1000) == 0
    names = ('table', 'idx', 'new', 'lens', 'emb', 'ids', 'new_ids', 'cw', 'sims', 'weight', 'ws')

    def step(b=2, k=16, dout=768, rows=50264, dtype=1, ws_floats=ws, t_sense=768, e_row=768, ids_pos=1, sims_pos=1,
             w_pos=1, sims_s=1000, scale=0.1, **ptrs):
        return h.bp_sense_anneal_step(*(ptrs.get(n, p) for n in names), ws_floats, b, k, dout, 1000, rows, 50264, 50264,
                                      16 * 768, t_sense, 1000, e_row, 1000, ids_pos, 1, k, 16 * 1000, sims_s, sims_pos,
                                      16 * 1000, 1000, w_pos, scale, 1, dtype, null)
    assert step(dtype=2) == -1
    assert step(dout=0) == -6
    assert step(dout=12) == -3 and step(dout=2056) == -3
    assert step(k=65) == -3 and step(k=0) == -3 and step(b=0) == -3 and step(rows=0) == -3
    assert step(k=64, dout=1120, t_sense=1120, e_row=1120) == -3          # the staged block would not fit the LDS
    for name in names:
        assert step(**{name: null}) == -3, name
    assert step(table=odd) == -3 and step(emb=odd) == -3
    assert step(t_sense=772) == -3 and step(e_row=772) == -3
    assert step(ids_pos=2) == -3 and step(sims_pos=2) == -3 and step(w_pos=2) == -3 and step(sims_s=999) == -3
    assert step(scale=float('inf')) == -4
    assert step(ws_floats=ws - 1) == -9


def test_fused_flag_raises_on_a_cpu_step_and_the_default_is_unchanged():
    model = _nano_backpack()
    ids = torch.randint(0, 200, (2, PROMPT + 1), generator=torch.Generator().manual_seed(1))
    cw = torch.rand(200, 16, generator=torch.Generator().manual_seed(2)) * 3
    default, flagged, flat = (WeightedBackpackLMHeadModel(model, cw, None, 40.0, anneal=anneal).eval()
                              for anneal in (True, True, False))
    flagged.fused_anneal_step = flat.fused_anneal_step = True
    assert default.fused_anneal_step is False and list(default.state_dict()) == list(flagged.state_dict())

    def cached(wrapper):
        ip = InferenceParams(max_sequence_len=PROMPT + 1, max_batch_size=2)
        with torch.inference_mode():
            wrapper(ids[:, :PROMPT], inference_params=ip)
            ip.sequence_len_offset = PROMPT
            return wrapper(ids[:, PROMPT:], inference_params=ip).logits[:, -1], ip
    want, ip = cached(default)
    assert 'intervened_dots' in ip.key_value_memory_dict
    with torch.inference_mode():
        assert (want - default(ids).logits[:, -1]).abs().max() <= 1e-4 * want.abs().max()
    with pytest.raises(RuntimeError, match='fused_anneal_step = True needs'):
        cached(flagged)
    assert torch.equal(cached(flat)[0], cached(WeightedBackpackLMHeadModel(model, cw, None, 40.0, anneal=False).eval())[0])


def test_anneal_step_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_resources as KR
    if not KR.tools_available():
        pytest.skip('LLVM tools not found under /opt/rocm')
    ks = KR.kernels([os.path.join(KR.BUILD, 'sense_anneal_step.o')])
    names = {k['name'] for k in ks}
    assert 'sense_anneal_step_kernel<BF16, 2, 1>' in names and 'sense_anneal_step_kernel<F16, 2, 4>' in names
    assert len(ks) == 2 * 4 * 4 + 1
    for k in ks:
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, k
