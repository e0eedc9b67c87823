"""CPU: training with the content network once per distinct token (config.sense_table_train='batch') where no GPU is
needed -- the float64 restatement of bp_segment_sum_rows against a hand-worked case, the entry point in the header, the
ctypes table and the library, its argument checks, the binding's refusal of host tensors, and the order itself on a float64
CPU model (use_flash_attn=False): the same loss and the same gradients as the per-position order, up to summation order."""
import ctypes
import re
import warnings

import numpy as np
import pytest
import torch

import bp_hip
import segment_sum_ref as REF
from conftest import ROOT


def test_reference_on_a_hand_worked_case():
    rows = np.array([[1, 2], [10, 20], [100, 200], [1000, 2000], [-1, -2]], dtype=np.float32)
    # segments: {3, 0}, {}, {1, 2, 4}; order lists them grouped, ascending inside a segment
    order, seg_begin = np.array([0, 3, 1, 2, 4]), np.array([0, 2, 2, 5])
    acc = np.full((3, 2), 7.0)
    out, mags = REF.segment_sum_rows(rows, order, seg_begin, acc, accumulate=False)
    assert out.tolist() == [[1001, 2002], [0, 0], [109, 218]]
    assert mags.tolist() == [[1001, 2002], [0, 0], [111, 222]]
    out, _ = REF.segment_sum_rows(rows, order, seg_begin, acc, accumulate=True)
    assert out.tolist() == [[1008, 2009], [7, 7], [116, 225]]
    # the clamps of the entry point: order unsigned to the last row, seg_begin to [0, n_rows], a decreasing pair is empty
    out, _ = REF.segment_sum_rows(rows, np.array([-1, 99, 0, 0, 0]), np.array([-5, 2, 1, 77]), acc)
    assert out.tolist() == [[-2, -4], [0, 0], [2, 4]]
    order, seg_begin = REF.segments_from_lengths([2, 0, 3])
    assert order.tolist() == [0, 1, 2, 3, 4] and seg_begin.tolist() == [0, 2, 2, 5]
    order, seg_begin = REF.segments_from_lengths([2, 0, 3], np.random.default_rng(0))
    assert sorted(order.tolist()) == [0, 1, 2, 3, 4] and order[:2].tolist() == sorted(order[:2].tolist())


def test_header_table_and_library_agree_on_the_new_entry_point():
    import os
    text = open(os.path.join(ROOT, 'include', 'bp_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    found = re.findall(r'\bint\s+bp_segment_sum_rows\s*\(([^)]*)\)\s*;', text)
    assert len(found) == 1
    params = [' '.join(re.sub(r'\w+$', '', p).split()) for p in found[0].split(',')]
    restype, argtypes = bp_hip.SIGNATURES['bp_segment_sum_rows']
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 12
    for have, c_type in zip(argtypes, params):
        want = ctypes.c_void_p if c_type.endswith('*') or c_type == 'bp_stream_t' else \
            {'int': ctypes.c_int, 'int64_t': ctypes.c_int64}[c_type]
        assert have is want, c_type
    assert hasattr(bp_hip.lib(), 'bp_segment_sum_rows')
    kernels = open(os.path.join(ROOT, 'backpacks-flash-attn_amd', 'csrc', 'bp_kernels.h')).read()
    assert re.search(r'kSegLongRows = %d;' % bp_hip.SEGMENT_LONG_ROWS, kernels)


def test_argument_validation_returns_before_any_launch():
    h = bp_hip.lib()
    null = None

    def call(rows=0x1000, order=0x2000, seg_begin=0x3000, acc=0x4000, n_rows=8, n_segments=3, cols=16, rows_stride=16,
             acc_stride=16, accumulate=0, dtype=1):
        as_ptr = [None if a is None else ctypes.c_void_p(a) for a in (rows, order, seg_begin, acc)]
        return h.bp_segment_sum_rows(*as_ptr, n_rows, n_segments, cols, rows_stride, acc_stride, accumulate, dtype, null)
    for kw in (dict(dtype=2), dict(dtype=7)):
        assert call(**kw) == -1, kw
    for kw in (dict(rows=null), dict(order=null), dict(seg_begin=null), dict(acc=null), dict(rows=0x1008), dict(acc=0x4004),
               dict(order=0x2002), dict(seg_begin=0x3001), dict(cols=12), dict(cols=0), dict(cols=-8), dict(cols=(1 << 24) + 8),
               dict(rows_stride=8), dict(rows_stride=20), dict(acc_stride=8), dict(acc_stride=18), dict(n_rows=-1),
               dict(n_rows=2 ** 31), dict(n_segments=-1), dict(n_segments=2 ** 31), dict(n_segments=2 ** 31 - 1),
               dict(accumulate=2), dict(accumulate=-1)):
        assert call(**kw) == -3, kw
    # nothing to sum into: a successful no-op without a launch (the addresses above are not memory)
    assert call(n_segments=0) == 0


def test_binding_refuses_cpu_tensors_before_loading_anything(monkeypatch):
    monkeypatch.setattr(bp_hip, 'lib', lambda: pytest.fail('the library was touched'))
    rows = torch.zeros(5, 16, dtype=torch.bfloat16)
    order, seg_begin = torch.arange(5, dtype=torch.int32), torch.tensor([0, 2, 5], dtype=torch.int32)
    with pytest.raises(RuntimeError, match='must live on the GPU'):
        bp_hip.segment_sum_rows(rows, order, seg_begin, torch.zeros(2, 16))
    qk = torch.zeros(1, 8, 2, 4, 16, dtype=torch.bfloat16, requires_grad=True)
    with pytest.raises(RuntimeError, match='must live on the GPU'):
        bp_hip.sense_mix_gather_autograd(qk, torch.zeros(3, 4, 32, dtype=torch.bfloat16), torch.zeros(1, 8, dtype=torch.int64))


def test_row_segments_groups_positions_by_row_in_ascending_order():
    index = torch.tensor([[3, 0, 3, 1], [0, 3, 3, 0]])
    order, seg_begin = bp_hip.row_segments(index, 5)
    assert order.dtype == torch.int32 and seg_begin.dtype == torch.int32
    assert order.tolist() == [1, 4, 7, 3, 0, 2, 5, 6] and seg_begin.tolist() == [0, 3, 4, 4, 8, 8]


def test_shape_limits_name_what_the_fused_route_does_not_take():
    assert bp_hip.sense_mix_gather_train_shape_limits(48, 1024) == ''
    assert bp_hip.sense_mix_gather_train_shape_limits(10, 4096) == ''
    assert '> 128' in bp_hip.sense_mix_gather_train_shape_limits(160, 64)
    assert '4096' in bp_hip.sense_mix_gather_train_shape_limits(48, 4097)


# ---- the order itself, float64 on the CPU ---------------------------------------------------------------------------------------

KW = dict(n_embd=128, n_head=2, n_layer=2, num_content_vectors=4, vocab_size=512, n_positions=64, resid_pdrop=0.0,
          embd_pdrop=0.0, attn_pdrop=0.0, scale_attn_by_inverse_layer_idx=True, use_flash_attn=False)


def _model(**more):
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    torch.manual_seed(5)
    model = BackpackLMHeadModel(BackpackConfig(**KW, **more)).double()
    with torch.no_grad():
        model.transformer.contextualization_attn.Wqkv.weight.mul_(6.0)
    return model


def _ids():
    gen = torch.Generator().manual_seed(3)
    tokens = torch.randperm(512, generator=gen)[:20]
    ids = tokens[torch.randint(0, 20, (3, 64), generator=gen)]
    assert all((ids == t).sum() >= 2 for t in ids.unique())     # every token repeats
    return ids


def _step(model, ids):
    model.zero_grad(set_to_none=True)
    logits = model(ids).logits
    loss = torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), torch.roll(ids, -1, 1).reshape(-1))
    loss.backward()
    return loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters()}


def _rows_seen(model, fn):
    seen = []
    hook = model.transformer.content_model.register_forward_hook(lambda mod, args, out: seen.append(tuple(args[0].shape)))
    try:
        return fn(), seen
    finally:
        hook.remove()


def test_batch_order_has_the_loss_and_gradients_of_the_per_position_order():
    """Loss and every parameter gradient to rtol = 1e-9, element by element, no absolute term: float64, the same mathematics,
    another order of summation.  ONE gradient cannot meet that in any implementation, and gets the bound its number format
    gives instead: the content network keeps its residual in fp32 whatever the parameters' dtype (`.float()` in
    BackpackContentModule.forward, the reference's residual_in_fp32), so the gradient that reaches the word embedding through
    it is ROUNDED to fp32 on the way -- once per occurrence g_i of a token in the per-position order, once per token, after
    the sum, in the table order.  sum_i round(g_i) and round(sum_i g_i) differ by at most 2^-24 sum|g_i| + 2^-24 |sum g_i|
    <= 2^-23 sum_i |g_i| per element (measured here: up to 0.92 of that bound, 4.1e-10 absolute at max|grad| = 1.0e-2, i.e.
    4e-8 relative: fp32 rounding, not float64).  The g_i are read by a backward hook in the per-position model (as rounded,
    hence the factor 1 + 2^-23); the trunk's part of that gradient is the same in both orders."""
    ids = _ids()
    off, batch = _model().train(), _model(sense_table_train='batch').train()
    assert off.transformer.sense_table_train == 'off' and batch.transformer.sense_table_train == 'batch'
    batch.load_state_dict(off.state_dict())
    rounded = []
    hook = off.transformer.content_model.emb_drop.register_full_backward_hook(lambda mod, gin, gout: rounded.append(gout[0]))
    (l_off, g_off), seen_off = _rows_seen(off, lambda: _step(off, ids))
    hook.remove()
    (l_batch, g_batch), seen_batch = _rows_seen(batch, lambda: _step(batch, ids))
    assert seen_off == [(3, 64)] and seen_batch == [(1, 20)]        # the content network ran over the distinct ids
    torch.testing.assert_close(l_batch, l_off, rtol=1e-9, atol=0)
    assert sorted(g_batch) == sorted(g_off)
    embedding = 'transformer.gpt2_model.embeddings.word_embeddings.weight'
    for name, want in g_off.items():
        if name != embedding:
            torch.testing.assert_close(g_batch[name], want, rtol=1e-9, atol=0, msg=name)
    (g_pos,) = rounded
    assert g_pos.shape == (3, 64, 128) and torch.equal(g_pos, g_pos.float().double())      # fp32 values: the cast is there
    magnitude = torch.zeros_like(g_off[embedding]).index_add_(0, ids.reshape(-1), g_pos.abs().reshape(-1, 128))
    bound = 2.0 ** -23 * (1 + 2.0 ** -23) * magnitude + 1e-9 * g_off[embedding].abs()
    err = (g_batch[embedding] - g_off[embedding]).abs()
    print('word embedding gradient: max err %.3e, max err / bound %.3f' % (err.max().item(), (err / (bound + 1e-300)).max().item()))
    assert (err <= bound).all()


def test_batch_order_changes_nothing_in_eval_or_without_gradients():
    ids = _ids()
    off, batch = _model(), _model(sense_table_train='batch')
    batch.load_state_dict(off.state_dict())
    for prepare in (lambda m: m.eval(), lambda m: m.train()):
        prepare(off), prepare(batch)
        with torch.no_grad():
            want = off(ids).logits
            got, seen = _rows_seen(batch, lambda: batch(ids).logits)
        assert torch.equal(got, want) and seen == [(3, 64)]          # the per-position order, bit for bit
    batch.eval()
    got, seen = _rows_seen(batch, lambda: batch(ids).logits)          # eval() with gradients enabled: per position too
    assert seen == [(3, 64)] and got.requires_grad


def test_an_unknown_value_raises():
    with pytest.raises(ValueError, match='sense_table_train'):
        _model(sense_table_train='cached')
    model = _model().train()
    model.transformer.sense_table_train = 'on'
    with pytest.raises(ValueError, match='sense_table_train'):
        model(_ids())


def test_dropout_in_the_content_network_is_said_once():
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    kw = dict(KW, resid_pdrop=0.1)
    torch.manual_seed(5)
    model = BackpackLMHeadModel(BackpackConfig(sense_table_train='batch', **kw)).train()
    ids = _ids()
    with warnings.catch_warnings(record=True) as said:
        warnings.simplefilter('always')
        model(ids), model(ids)
    said = [w for w in said if 'sense_table_train' in str(w.message)]
    assert len(said) == 1 and 'share' in str(said[0].message)
    assert model.transformer.sense_table_train_chunk_samples == bp_hip.SENSE_TABLE_TRAIN_CHUNK_SAMPLES == 8
