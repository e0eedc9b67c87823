"""CPU: sense attribution (src/utils/sense_attribution.py) against the float64 restatement of tests/sense_attribution_ref.py
-- the torch twin of bp_sense_attribute on drawn operands, the Python layer on the nano Backpack in fp32 (the shares sum to
the model's logit, the weights are the row of alpha), the two localize statistics, the ranking -- and, without a GPU, the
C ABI of bp_sense_attribute (every refusal, before any launch) and the register account of its code object."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import bp_hip
import sense_attribution_ref as R
from decode_support import _close_fp32, _nano_backpack
from src.utils import sense_attribution as SA
from test_abi import ctypes_of, declared_prototypes

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}


def _drawn(batch, seqlen, k, dk, d, rows, nq, nvec, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    qk = (torch.randn(batch, seqlen, 2, k, dk, generator=g) * 1.5).to(dtype)
    table = torch.randn(rows, k, d, generator=g).to(dtype)
    index = torch.randint(0, rows, (batch, seqlen), generator=g, dtype=torch.int32)
    index[0, 0], index[-1, -1] = rows + 5, -1                  # beyond the table: the last row
    sample = torch.randint(0, batch, (nq,), generator=g, dtype=torch.int32)
    pos = torch.randint(0, seqlen, (nq,), generator=g, dtype=torch.int32)
    pos[0], pos[-1] = 0, seqlen - 1
    vec = torch.randn(nq, nvec, d, generator=g)
    return qk, table, index, sample, pos, vec


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('shape', [(3, 21, 4, 16, 64, 11, 6, 2), (2, 9, 16, 8, 24, 40, 5, 4), (1, 1, 1, 8, 8, 1, 1, 1)])
def test_eager_sense_attribute_matches_the_restatement(shape, dtype):
    batch, seqlen, k, dk, d, rows, nq, nvec = shape
    qk, table, index, sample, pos, vec = _drawn(*shape, DTYPES[dtype], seed=seqlen)
    scale = dk ** -0.5
    out, probs = SA._eager_sense_attribute(qk, table, index, sample, pos, vec, scale, want_probs=True)
    assert out.shape == (nq, nvec, k, seqlen) and out.dtype == torch.float32 and probs.shape == (nq, k, seqlen)
    want, want_p, unit = R.sense_attribute(qk, table, index, sample, pos, vec, scale)
    factor = R.fp32_factor(qk, sample, pos, scale, d)
    err = np.abs(out.double().numpy() - want)
    print(f'eager fp32 {shape} {dtype}: largest error / allowed = {(err / (factor * unit + 1e-300)).max():.3f}')
    assert (err <= factor * unit).all()
    assert (np.abs(probs.double().numpy() - want_p) <= factor * want_p).all()
    behind = np.arange(seqlen)[None, :] > np.asarray(pos)[:, None]
    assert (out.numpy()[np.broadcast_to(behind[:, None, None, :], out.shape)] == 0).all() and (want_p[:, 0][behind] == 0).all()
    assert SA._eager_sense_attribute(qk, table, index, sample, pos, vec, scale)[1] is None


def test_eager_clamps_queries_and_reads_nothing_behind_them():
    qk, table, index, sample, pos, vec = _drawn(2, 12, 4, 8, 16, 30, 4, 1, torch.bfloat16, seed=1)
    sample[:], pos[:] = torch.tensor([0, 1, 1, 0]), torch.tensor([5, 11, 3, 0])
    index.clamp_(0, 29)                                        # (the table grows by a row below: no entry may lean on the clamp)
    scale = 8 ** -0.5
    base = SA._eager_sense_attribute(qk, table, index, sample, pos, vec, scale, True)
    wild = SA._eager_sense_attribute(qk, table, index, torch.tensor([-1, 2, 1, 0], dtype=torch.int32),
                                     torch.tensor([5, 12, 3, -1], dtype=torch.int32), vec, scale, True)
    assert torch.equal(base[0], wild[0]) and torch.equal(base[1], wild[1])
    poisoned = qk.clone()
    poisoned[0, 6:, 1] = float('nan')                          # keys behind query 0 (sample 0, position 5)
    table2 = torch.cat([table, torch.full((1, 4, 16), float('nan'), dtype=table.dtype)])
    index2 = index.clone()
    index2[0, 6:] = 30                                         # ... and its rows
    got = SA._eager_sense_attribute(poisoned, table2, index2, sample[:1], pos[:1], vec[:1], scale, True)
    assert torch.equal(got[0], base[0][:1]) and torch.equal(got[1], base[1][:1])


# ---- the Python layer on the nano Backpack (fp32, eager path) -------------------------------------------------------------------------------

S = 24


@pytest.fixture(scope='module')
def nano():
    model = _nano_backpack()
    ids = torch.randint(0, 200, (2, S), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        logits = model(ids).logits
        hidden = model.transformer.gpt2_model(ids)
        alpha = model.transformer.contextualization_attn(hidden)       # (B, k, S, S)
    return model, ids, logits, alpha


def test_the_shares_sum_to_the_models_logit(nano):
    model, ids, logits, alpha = nano
    pairs = [(0, 0), (1, 0), (0, S // 2), (1, S // 2), (0, S - 1), (1, S - 1)]
    targets = torch.tensor([[3, 77, 199]] * len(pairs))
    res = SA.sense_contributions(model, ids, pairs, target_ids=targets, return_probs=True)
    assert res.contributions.shape == (len(pairs), 3, 16, S) and res.contributions.dtype == torch.float32
    assert res.logits.shape == (len(pairs), 3) and res.samples.tolist() == [0, 1] * 3
    want = torch.stack([logits[b, i, targets[0]] for b, i in pairs])
    _close_fp32(res.logits, want, 'sum over (k, S) against the logit')
    for n, (b, i) in enumerate(pairs):
        assert (res.contributions[n, :, :, i + 1:] == 0).all()
        torch.testing.assert_close(res.probs[n], alpha[b, :, i, :], rtol=1e-4, atol=1e-6)
        assert (res.probs[n, :, i + 1:] == 0).all()
    # one position per sample; one target per query; given vectors  (calls of other shapes: the CPU BLAS may round a dot's
    # last bits differently, so a few ulps of the share)
    per_sample = SA.sense_contributions(model, ids, [S // 2, S - 1], target_ids=[77, 3])
    torch.testing.assert_close(per_sample.contributions[0, 0], res.contributions[2, 1], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(per_sample.contributions[1, 0], res.contributions[5, 0], rtol=1e-5, atol=1e-7)
    assert per_sample.probs is None and per_sample.contributions.shape == (2, 1, 16, S)
    given = SA.sense_contributions(model, ids, pairs, vectors=model.lm_head.weight[targets].float())
    assert torch.equal(given.contributions, res.contributions)
    many = SA.sense_contributions(model, ids, pairs[:2], target_ids=torch.arange(12).view(2, 6))    # more than four vectors
    _close_fp32(many.logits, torch.stack([logits[0, 0, :6], logits[1, 0, 6:12]]), 'six targets per query')


def test_arguments_are_checked(nano):
    model, ids, _, _ = nano
    with pytest.raises(ValueError, match='one of them'):
        SA.sense_contributions(model, ids, [0, 1])
    with pytest.raises(ValueError, match='one of them'):
        SA.sense_contributions(model, ids, [0, 1], target_ids=[1, 2], vectors=torch.zeros(2, 1, 384))
    with pytest.raises(ValueError, match='outside'):
        SA.sense_contributions(model, ids, [0, S], target_ids=[1, 2])
    with pytest.raises(ValueError, match='positions'):
        SA.sense_contributions(model, ids, [0, 1, 2], target_ids=[1, 2, 3])
    with pytest.raises(ValueError, match='target_ids'):
        SA.sense_contributions(model, ids, [0, 1], target_ids=[1, 2, 3])
    with pytest.raises(ValueError, match='two ids'):
        SA.contextual_localize(model, [[4]], 7)


def test_a_right_padded_row_equals_the_row_alone(nano):
    model, ids, _, _ = nano
    short = ids[:1, :9]
    alone = SA.sense_contributions(model, short, [8], target_ids=[5])
    padded = SA.sense_contributions(model, torch.cat([short, torch.zeros(1, S - 9, dtype=torch.long)], dim=1), [8], target_ids=[5])
    assert (padded.contributions[..., 9:] == 0).all()
    torch.testing.assert_close(padded.contributions[..., :9], alone.contributions, rtol=1e-4, atol=1e-6)


def test_contextual_localize_equals_the_restatement(nano):
    model, _, _, _ = nano
    g = torch.Generator().manual_seed(9)
    contexts = [torch.randint(0, 200, (n,), generator=g).tolist() for n in (3, 9, 20)]
    contexts[1][2] = contexts[2][4] = contexts[2][11] = contexts[0][0]           # one token in several places and contexts
    target = 41
    tr = model.transformer

    def qk_of(ctx):
        with torch.no_grad():
            return tr.contextualization_attn.project(tr.gpt2_model(torch.as_tensor(ctx)[None]))[0]

    with torch.no_grad():
        senses = tr.content_model(torch.arange(model.lm_head.weight.shape[0])[None])[0].transpose(0, 1)      # (V, k, d)
    emb = model.lm_head.weight.detach()
    scale = tr.contextualization_attn.scale()
    want_plus, want_minus, unit_plus, unit_minus = R.contextual_localize(contexts, target, qk_of, senses, emb, scale)
    plus, minus = SA.contextual_localize(model, contexts, target)
    assert plus.shape == minus.shape == (emb.shape[0], 16) and plus.dtype == minus.dtype == torch.float32
    seen = sorted({t for c in contexts for t in c[:-1]})
    assert (plus[[t for t in range(emb.shape[0]) if t not in seen]] == 0).all() and (plus[seen] != 0).any(dim=1).all()
    # twice the first-order fp32 bound (sense_attribution_ref.fp32_factor; the padded batch and the contexts alone also differ
    # in how the fp32 GEMMs of the trunk round their rows), the vocabulary's fp32 embedding sum included, and half an fp32 ulp
    # of the result's own rounding
    qk_all = torch.stack([torch.nn.functional.pad(qk_of(c), (0, 0, 0, 0, 0, 0, 0, 20 - len(c))) for c in contexts])
    factor = 2 * R.fp32_factor(qk_all, [0, 1, 2], [len(c) - 2 for c in contexts], scale, emb.shape[1], extra=emb.shape[0])
    for name, got, want, unit in (('plus', plus, want_plus, unit_plus), ('minus', minus, want_minus, unit_minus)):
        err = np.abs(got.double().numpy() - want)
        allowed = factor * unit + 2.0 ** -24 * np.abs(want)
        print(f'contextual_localize {name}: largest error / allowed = {(err[unit > 0] / allowed[unit > 0]).max():.3f}')
        assert (err <= allowed).all(), name


def test_top_contributions_equals_a_stable_sort(nano):
    model, ids, _, _ = nano
    res = SA.sense_contributions(model, ids, [(0, 0), (1, S - 1), (0, 7)], target_ids=[[3, 9], [77, 1], [5, 5]])
    for count in (1, 10, 64):
        top = SA.top_contributions(res, count)
        want = R.top_contributions(res.contributions.numpy(), count)
        got = (top.top_positions, top.top_senses, top.top_values, top.bottom_positions, top.bottom_senses, top.bottom_values)
        for g, w, name in zip(got, want, ('top_pos', 'top_sense', 'top_val', 'bot_pos', 'bot_sense', 'bot_val')):
            assert g.shape == (3, 2, count)
            if 'val' in name:
                assert g.dtype == torch.float32 and (R.bits_of(g.numpy()) == R.bits_of(w)).all(), (count, name)
            else:
                assert g.dtype == torch.int64 and (g.numpy() == w).all(), (count, name)
    # query (0, 0) sees one position: 16 non-zero shares, then exact zeros by ascending (sense, position)
    top = SA.top_contributions(res, 64)
    assert (top.top_positions[0, 0][top.top_values[0, 0] != 0] == 0).all()
    with pytest.raises(ValueError):
        SA.top_contributions(res, 65)
    text = SA.format_contributions(SA.top_contributions(res, 3), input_ids=ids, samples=res.samples)
    assert text.count('~~~Positive~~~') == 6 and 'position 0 sense' in text
    assert SA.format_contributions(SA.top_contributions(res, 3)).count('sense') == 6 * 6


# ---- C ABI and code object ---------------------------------------------------------------------------------------------------------------

def test_sense_attribute_signature_and_the_header_agree():
    i32, i64, f32, ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    assert bp_hip.SIGNATURES['bp_sense_attribute'] == (i32, [ptr] * 9 + [i64] + [i32] * 7 + [i64] + [i64] * 14 + [f32, i32, ptr])
    assert bp_hip.SIGNATURES['bp_sense_attribute_ws_floats'] == (i64, [i32] * 2)
    protos = declared_prototypes()
    for name in ('bp_sense_attribute', 'bp_sense_attribute_ws_floats'):
        ret, params = protos[name]
        assert bp_hip.SIGNATURES[name] == (ctypes_of(ret), [ctypes_of(c) for c in params]), name
    header = open(os.path.join(ROOT, 'include', 'bp_hip.h')).read()
    assert '#define BP_ABI_VERSION 11 ' in header and '#define BP_ATTRIBUTE_MAX_VECS 4 ' in header
    assert bp_hip.ABI_VERSION == 11 and bp_hip.ATTRIBUTE_MAX_VECS == 4


def test_sense_attribute_refuses_before_any_launch():
    h = bp_hip.lib()
    p, null = ctypes.c_void_p(0x1000), None
    odd = ctypes.c_void_p(0x1008)      # 8-byte aligned only
    byte = ctypes.c_void_p(0x1002)
    assert h.bp_sense_attribute_ws_floats(3, 16) == 96 and h.bp_sense_attribute_ws_floats(0, 16) == 0

    def call(qk=p, table=p, index=p, qs=p, qp=p, vec=p, out=p, probs=p, ws=p, ws_floats=2 * 3 * 16,
             batch=2, seqlen=100, k=16, dk=48, dout=768, nq=3, nvec=2, rows=1000,
             qk_bs=100 * 1536, qk_rs=1536, qk_two=768, qk_ss=48, t_rs=16 * 768, t_ss=768, idx_bs=100,
             v_qs=2 * 768, v_vs=768, o_qs=2 * 16 * 100, o_vs=16 * 100, o_ss=100, p_qs=16 * 100, p_ss=100,
             scale=0.144, dtype=1):
        return h.bp_sense_attribute(qk, table, index, qs, qp, vec, out, probs, ws, ws_floats, batch, seqlen, k, dk, dout,
                                    nq, nvec, rows, qk_bs, qk_rs, qk_two, qk_ss, t_rs, t_ss, idx_bs, v_qs, v_vs,
                                    o_qs, o_vs, o_ss, p_qs, p_ss, scale, dtype, null)

    assert call(dtype=2) == -1 and call(dtype=-1) == -1                                        # BP_ERR_DTYPE
    assert call(dk=0) == -2 and call(dk=44) == -2 and call(dk=648) == -2                       # BP_ERR_HEAD_DIM
    assert call(dout=0) == -6 and call(dout=-8) == -6 and call(dout=12) == -6 and call(dout=2056) == -6     # BP_ERR_DOUT
    for bad in (dict(nq=0), dict(nq=65536), dict(nvec=0), dict(nvec=5), dict(k=0), dict(k=65), dict(seqlen=0), dict(batch=0),
                dict(rows=0), dict(rows=2 ** 31)):
        assert call(**bad) == -3, bad                                                          # BP_ERR_SHAPE
    for name in ('qk', 'table', 'index', 'qs', 'qp', 'vec', 'out', 'ws'):
        assert call(**{name: null}) == -3, name
    for name in ('qk', 'table', 'vec'):
        assert call(**{name: odd}) == -3, name
    for name in ('index', 'qs', 'qp', 'out', 'probs', 'ws'):
        assert call(**{name: byte}) == -3, name
    for name in ('qk_bs', 'qk_rs', 'qk_two', 'qk_ss', 't_rs', 't_ss'):
        assert call(**{name: 1540}) == -3, name
    assert call(v_qs=1538) == -3 and call(v_vs=770) == -3
    assert call(o_ss=99) == -3 and call(o_vs=1599) == -3 and call(o_qs=3199) == -3
    assert call(p_ss=99) == -3 and call(p_qs=1599) == -3
    assert call(scale=0.0) == -4 and call(scale=float('nan')) == -4 and call(scale=-1.0) == -4  # BP_ERR_SCALE
    assert call(ws_floats=95) == -9                                                            # BP_ERR_WORKSPACE
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.sense_attribute(torch.zeros(1, 4, 2, 2, 8, dtype=torch.bfloat16), torch.zeros(3, 2, 8, dtype=torch.bfloat16),
                               torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                               torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1, 8), 1.0)
    assert not bp_hip.sense_attribute_supported(torch.zeros(1, 4, 2, 2, 8, dtype=torch.bfloat16),
                                                torch.zeros(3, 2, 8, dtype=torch.bfloat16), torch.zeros(1, 4, dtype=torch.int32),
                                                torch.zeros(1, 1, 8))


sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import kernel_resources as KR  # noqa: E402

STATS = ['sense_attribute_stats_kernel<%s>' % t for t in ('BF16', 'F16')]
SHARES = ['sense_attribute_kernel<%s, %d, %d>' % (t, nch, nv) for t in ('BF16', 'F16') for nch in (1, 2, 3, 4) for nv in (1, 2, 4)]


def test_sense_attribute_kernels_use_no_scratch_and_hold_the_vectors_in_registers():
    if not KR.tools_available():
        pytest.skip('llvm-objcopy / clang-offload-bundler / llvm-readelf not found under /opt/rocm')
    import importlib.util
    spec = importlib.util.spec_from_file_location('bp_build_hip', os.path.join(ROOT, 'backpacks-flash-attn_amd', 'build_hip.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()   # no-op when the objects are current
    table = {k['name']: k for k in KR.kernels([os.path.join(KR.BUILD, 'sense_attribute.o')])}
    assert sorted(table) == sorted(STATS + SHARES), 'the object holds these kernels and no other'
    for name in STATS + SHARES:
        k = table[name]
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, k
        assert k['max_flat_workgroup_size'] == 256, k
    for name in STATS:
        assert table[name]['vgpr_count'] <= 64 and table[name]['group_segment_fixed_size'] == 640 * 2 + 16, table[name]
    for name in SHARES:
        nch, nv = (int(x) for x in name[:-1].split(', ')[1:])
        # the vectors (nv * nch * 8 fp32) and one row's chunks (nch * 4) live in registers, next to at most 48 others
        assert nv * nch * 8 <= table[name]['vgpr_count'] <= nv * nch * 8 + nch * 4 + 48, table[name]
        assert table[name]['group_segment_fixed_size'] == (nv + 1) * 64 * 4 * 4, table[name]
