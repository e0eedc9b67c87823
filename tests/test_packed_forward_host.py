"""CPU: packed (variable-length) batches -- the three bp_sense_*_varlen entry points in the header, the ctypes table and the
library, their refusals before any launch, the helpers of src/utils/packing.py, and the packed forward of the eager fp32
model (which pads and runs: equal to the padded forward's real rows by construction) through the scoring utilities."""
import ctypes

import pytest
import torch

import bp_hip
from decode_support import _nano_backpack
from src.utils import scoring
from src.utils.packing import pack_sequences, packed_position_ids, unpack_rows
from test_abi import declared_prototypes

VARLEN = ('bp_sense_lse_varlen', 'bp_sense_mix_varlen', 'bp_sense_mix_gather_varlen')


def test_header_table_and_library_agree_on_the_three_entries():
    protos, handle = declared_prototypes(), bp_hip.lib()
    for name in VARLEN:
        assert name in protos and name in bp_hip.SIGNATURES and hasattr(handle, name), name
        ret, params = protos[name]
        assert ret == 'int' and len(params) == len(bp_hip.SIGNATURES[name][1])
        assert 'const int32_t *' in params and 'int64_t' in params
    # the fixed-length signatures with cu_seqlens in front of batch, no batch strides, no idx_batch_stride
    for name, fixed, dropped in (('bp_sense_lse_varlen', 'bp_sense_lse', 1), ('bp_sense_mix_varlen', 'bp_sense_mix', 3),
                                 ('bp_sense_mix_gather_varlen', 'bp_sense_mix_gather', 3)):
        assert len(protos[name][1]) == len(protos[fixed][1]) + 1 - dropped
    assert bp_hip.ABI_VERSION == 11 and handle.bp_abi_version() == 11


def test_refusals_come_before_any_launch():
    h = bp_hip.lib()
    p, null = ctypes.c_void_p(0x1000), None   # never dereferenced: validation fails first

    def lse(dtype=1, d_k=16, cu=p, batch=1, max_seqlen=16, qk=p, out=p, strides=(64, 32, 16)):
        return h.bp_sense_lse_varlen(qk, out, cu, batch, max_seqlen, 4, d_k, *strides, 0.25, dtype, null)

    def mix(dtype=1, d_k=16, d_out=64, cu=p, max_seqlen=16, queue=null, out=p, scale=0.25, strides=(128, 64, 16, 256, 64, 64)):
        return h.bp_sense_mix_varlen(p, p, out, p, 0, cu, 1, max_seqlen, 4, d_k, d_out, *strides, scale, dtype, queue, null)

    def gather(dtype=1, d_k=16, d_out=64, cu=p, max_seqlen=16, rows=100, index=p, queue=null):
        return h.bp_sense_mix_gather_varlen(p, p, index, p, p, 0, cu, 1, max_seqlen, 4, d_k, d_out, rows,
                                            128, 64, 16, 256, 64, 64, 0.25, dtype, queue, null)

    for call in (lse, mix, gather):
        assert call(dtype=7) == -1                       # BP_ERR_DTYPE
        assert call(d_k=136) == -2                       # BP_ERR_HEAD_DIM: no packed wide kernels
        assert call(d_k=12) == -2                        # ... nor an element-wise loader
        assert call(cu=null) == -3                       # BP_ERR_SHAPE
        assert call(max_seqlen=0) == -3
    assert lse(out=null) == -3 and lse(batch=0) == -3
    assert lse(strides=(64, 32, 12)) == -3               # a stride that is no multiple of 8
    assert mix(d_out=20) == -6 and gather(d_out=20) == -6    # BP_ERR_DOUT
    assert mix(queue=ctypes.c_void_p(0x1004)) == -3 and gather(queue=ctypes.c_void_p(0x1004)) == -3
    assert mix(out=null) == -3
    assert mix(scale=0.0) == -4
    assert mix(max_seqlen=65537) == -3
    assert mix(strides=(128, 64, 16, 252, 64, 64)) == -3
    assert gather(max_seqlen=4097) == -3 and gather(rows=65537) == -3 and gather(rows=0) == -3
    assert gather(index=null) == -3


def test_binding_refuses_cpu_tensors_and_bad_layouts():
    qk = torch.randn(8, 2, 4, 16).bfloat16()
    cu = torch.tensor([0, 3, 8], dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.sense_lse_varlen(qk, cu, 5)
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.sense_mix_varlen(qk, torch.randn(8, 4, 32).bfloat16(), cu, 5)
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.sense_mix_gather_varlen(qk, torch.randn(10, 4, 32).bfloat16(), torch.zeros(8, dtype=torch.int32), cu, 5)
    table = torch.randn(10, 4, 32).bfloat16()
    assert not bp_hip.sense_mix_varlen_supported(qk, table, 5)          # CPU tensors
    assert 'GPU' in bp_hip.sense_mix_varlen_limits(qk, table, 5)
    wide = torch.randn(8, 2, 4, 160).bfloat16()
    assert '> 128' in bp_hip.sense_mix_gather_varlen_limits(wide, table, 5)
    assert '4096' in bp_hip.sense_mix_gather_varlen_limits(qk, table, 5000)
    assert '4096' not in bp_hip.sense_mix_varlen_limits(qk, table, 5000)


def test_pack_and_unpack_round_trip():
    seqs = [[5, 6, 7], [8], [], [9, 10, 11, 12]]
    ids, cu, longest = pack_sequences(seqs)
    assert ids.tolist() == [5, 6, 7, 8, 9, 10, 11, 12] and ids.dtype == torch.int64
    assert cu.tolist() == [0, 3, 4, 4, 8] and cu.dtype == torch.int32 and longest == 4
    padded = unpack_rows(ids, cu, longest, fill=-1)
    assert padded.tolist() == [[5, 6, 7, -1], [8, -1, -1, -1], [-1, -1, -1, -1], [9, 10, 11, 12]]
    again = pack_sequences(padded, [3, 1, 0, 4])
    assert torch.equal(again[0], ids) and torch.equal(again[1], cu) and again[2] == longest
    assert pack_sequences([torch.tensor([1, 2]), [3]])[0].tolist() == [1, 2, 3]
    values = torch.arange(16.).reshape(8, 2)
    wide = unpack_rows(values, cu, 6, fill=0.5)
    assert wide.shape == (4, 6, 2) and torch.equal(wide[3, :4], values[4:]) and (wide[3, 4:] == 0.5).all() and (wide[2] == 0.5).all()
    assert packed_position_ids(cu, 8).tolist() == [0, 1, 2, 0, 0, 1, 2, 3]


def test_packing_helpers_check_their_input():
    for bad, lengths in (([], None), ([[], []], None), (torch.zeros(2, 3, dtype=torch.int64), [1, -1]),
                         (torch.zeros(2, 3, dtype=torch.int64), [1, 4]), (torch.zeros(2, 3, dtype=torch.int64), [1]),
                         (torch.zeros(2, 3, dtype=torch.int64), None), ([[1, 2]], [2]), (torch.zeros(2, 3, dtype=torch.int64), [0, 0])):
        with pytest.raises(ValueError):
            pack_sequences(bad, lengths)
    cu = torch.tensor([0, 3, 4], dtype=torch.int32)
    with pytest.raises(ValueError):
        unpack_rows(torch.zeros(5), cu, 3)          # cu ends at 4
    with pytest.raises(ValueError):
        unpack_rows(torch.zeros(4), cu, 2)          # a sequence of 3 in a width of 2
    with pytest.raises(ValueError):
        unpack_rows(torch.zeros(4), cu[:1], 2)


@pytest.fixture(scope='module')
def nano():
    return _nano_backpack(seed=3)


def _padded_case(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 200, (len(lengths), max(lengths)), generator=g)
    for b, n in enumerate(lengths):
        ids[b, n:] = 0
    return ids, torch.tensor(lengths)


@pytest.mark.parametrize('lengths', [(1, 7, 3, 6), (5, 5, 5), (4, 0, 2)])
def test_packed_forward_equals_the_padded_forwards_real_rows(nano, lengths):
    ids, lens = _padded_case(lengths, seed=sum(lengths))
    packed, cu, longest = pack_sequences(ids, lens)
    with torch.no_grad():
        want = nano(ids).logits
        got = nano(packed, cu_seqlens=cu, max_seqlen=longest).logits
        hidden = nano.transformer(packed, cu_seqlens=cu, max_seqlen=longest)
        wider = nano(packed, cu_seqlens=cu, max_seqlen=longest + 3).logits
    assert got.shape == (sum(lengths), want.shape[-1]) and hidden.shape == (sum(lengths), 384)
    for b, n in enumerate(lengths):
        assert torch.equal(got[int(cu[b]):int(cu[b + 1])], want[b, :n]), b
    # the pads' ids do not matter, and a larger max_seqlen changes nothing that fp32 sees beyond BLAS shapes
    torch.testing.assert_close(wider, got, rtol=1e-5, atol=1e-5)
    out = torch.empty_like(got)
    with torch.no_grad():
        assert nano(packed, cu_seqlens=cu, max_seqlen=longest, logits_out=out).logits is out
    assert torch.equal(out, got)


def test_default_positions_restart_in_every_sequence(nano):
    ids, lens = _padded_case((3, 6, 2), seed=11)
    packed, cu, longest = pack_sequences(ids, lens)
    pos = packed_position_ids(cu, packed.shape[0])
    assert pos.tolist() == [0, 1, 2, 0, 1, 2, 3, 4, 5, 0, 1]
    with torch.no_grad():
        default = nano(packed, cu_seqlens=cu, max_seqlen=longest).logits
        explicit = nano(packed, position_ids=pos, cu_seqlens=cu, max_seqlen=longest).logits
        running = nano(packed, position_ids=torch.arange(packed.shape[0]), cu_seqlens=cu, max_seqlen=longest).logits
    assert torch.equal(default, explicit)
    assert torch.equal(running[:3], default[:3]) and not torch.equal(running[3:], default[3:])


def test_packed_forward_refuses_what_it_does_not_take(nano):
    from src.models.intervened_models import ScaledSenseLMHeadModel, WeightedBackpackLMHeadModel
    from src.utils.generation import InferenceParams
    packed, cu, longest = pack_sequences([[1, 2, 3], [4, 5]])
    with pytest.raises(RuntimeError, match='inference-only'):
        nano(packed, cu_seqlens=cu, max_seqlen=longest)
    with torch.no_grad():
        with pytest.raises(ValueError, match='inference_params'):
            nano(packed, cu_seqlens=cu, max_seqlen=longest, inference_params=InferenceParams(max_sequence_len=8, max_batch_size=2))
        with pytest.raises(ValueError):
            nano(packed, cu_seqlens=cu)                              # no max_seqlen
        with pytest.raises(ValueError):
            nano(packed.unsqueeze(0), cu_seqlens=cu, max_seqlen=longest)
        with pytest.raises(ValueError):
            nano(packed, cu_seqlens=cu.long(), max_seqlen=longest)
        wrappers = (ScaledSenseLMHeadModel(nano, [5], 0, 0.5),
                    WeightedBackpackLMHeadModel(nano, torch.ones(200, 16), torch.zeros(384), 1.0, anneal=False))
        for wrapper in wrappers:
            with pytest.raises(NotImplementedError, match='packed'):
                wrapper(packed, cu_seqlens=cu, max_seqlen=longest)
            with pytest.raises(NotImplementedError, match='packed'):
                scoring.score_tokens(wrapper, torch.ones(2, 3, dtype=torch.int64), lengths=[3, 2], packed=True)
        with pytest.raises(ValueError, match='lengths'):
            scoring.score_tokens(nano, torch.ones(2, 3, dtype=torch.int64), packed=True)


def test_scoring_packed_equals_padded_exactly(nano):
    ids, lens = _padded_case((9, 2, 6, 1, 12), seed=21)
    a = scoring.score_tokens(nano, ids, lengths=lens)
    b = scoring.score_tokens(nano, ids, lengths=lens, packed=True)
    assert torch.equal(a.mask, b.mask) and a.mask.sum() == sum(n - 1 for n in (9, 2, 6, 1, 12))
    for field in ('logprobs', 'ranks', 'top1', 'entropy', 'lse'):
        assert torch.equal(getattr(a, field), getattr(b, field)), field
    batches = [(ids, None, lens), {'input_ids': ids[:2, :9], 'lengths': lens[:2]}, ids[:, :5]]
    assert scoring.evaluate_lm(nano, batches) == scoring.evaluate_lm(nano, batches, packed=True)
    context, choices = [3, 4, 5], [[6], [7, 8, 9, 10], [11, 12]]
    for normalize in (False, True):
        order_a, scores_a = scoring.rank_choices(nano, context, choices, normalize=normalize)
        order_b, scores_b = scoring.rank_choices(nano, context, choices, normalize=normalize, packed=True)
        assert torch.equal(order_a, order_b) and torch.equal(scores_a, scores_b)
    examples = [([1, 2, 3, 4], [5, 6]), ([7], [8]), ([9, 10, 11, 12, 13, 14], [15])]
    assert scoring.last_word_eval(nano, examples) == scoring.last_word_eval(nano, examples, packed=True)
    good, bad = [[1, 2, 3], [4, 5, 6, 7, 8]], [[1, 2, 9], [4, 5]]
    pa, pb = scoring.pair_accuracy(nano, good, bad), scoring.pair_accuracy(nano, good, bad, packed=True)
    assert pa['accuracy'] == pb['accuracy'] and torch.equal(pa['good'], pb['good']) and torch.equal(pa['bad'], pb['bad'])
