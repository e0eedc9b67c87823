"""CPU: the vocabulary projections of sense vectors (src/utils/sense_vocab.py) against the numpy restatement of
tests/sense_vocab_ref.py -- the torch twin of bp_row_extremes bit for bit, the Python layer on the nano configuration in
fp32 within the first-order bound of sense_vocab_ref.localize_bound, the three-line pipeline into
WeightedBackpackLMHeadModel -- and, without a GPU, the C ABI of bp_row_extremes (argument checks before any launch) and
the register account of its code object."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import bp_hip
import sense_vocab_ref as R
from src.models.backpack import BackpackConfig, BackpackLMHeadModel
from src.models.intervened_models import WeightedBackpackLMHeadModel
from src.utils import sense_vocab as SV

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
COLS = [1, 7, 8, 9, 63, 64, 65, 1000]
VOCAB, K, D = 96, 4, 64


def _ns(cols):
    return sorted({n for n in (1, 2, 10, 20, 64, cols) if 1 <= n <= min(cols, 64)})


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ('top_val', 'top_idx', 'bot_val', 'bot_idx')):
        g = g.cpu().numpy()
        if 'val' in name:
            assert g.dtype == np.float32 and (R.bits_of(g) == R.bits_of(w)).all(), (what, name)
        else:
            assert g.dtype == np.int32 and (g == w).all(), (what, name)


def _rows(kind, rows, cols, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'drawn':
        x = torch.randn(rows, cols, generator=g) * 3
    elif kind == 'constant':
        x = torch.full((rows, cols), -1.625)
    elif kind == 'two-valued':
        x = torch.where(torch.rand(rows, cols, generator=g) < 0.5, 0.75, -2.5)
    else:   # signed zeros and infinities among a few numbers
        pool = torch.tensor([0.0, -0.0, float('inf'), -float('inf'), 1.0, -1.0])
        x = pool[torch.randint(0, len(pool), (rows, cols), generator=g)]
    return x.to(dtype)


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('cols', COLS)
def test_eager_row_extremes_matches_the_restatement_bit_for_bit(cols, dtype):
    for kind in ('drawn', 'constant', 'two-valued', 'zeros-and-infs'):
        x = _rows(kind, 5, cols, DTYPES[dtype], seed=cols)
        for n in _ns(cols):
            got = SV._eager_row_extremes(x, n)
            _assert_same(got, R.row_extremes(x, n), (kind, cols, n, dtype))
            if kind == 'constant':
                want = np.tile(np.arange(n, dtype=np.int32), (5, 1))
                assert (got[1].numpy() == want).all() and (got[3].numpy() == want).all(), 'both ends: columns 0 .. n - 1'


def test_eager_row_extremes_orders_signed_zeros_and_skips_an_end():
    x = torch.tensor([[0.0, -0.0, 0.0, -0.0, 1.0]])
    tv, ti, bv, bi = SV._eager_row_extremes(x, 3)
    assert ti.tolist() == [[4, 0, 2]] and bi.tolist() == [[1, 3, 0]]
    assert np.signbit(bv.numpy()).tolist() == [[True, True, False]]
    assert SV._eager_row_extremes(x, 2, smallest=False)[2:] == (None, None)
    assert SV._eager_row_extremes(x, 2, largest=False)[:2] == (None, None)
    with pytest.raises(RuntimeError):
        SV._eager_row_extremes(x, 6)
    with pytest.raises(RuntimeError):
        SV._eager_row_extremes(x, 0)


# ---- the Python layer on the nano configuration -----------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def nano():
    torch.manual_seed(3)
    cfg = BackpackConfig(n_embd=D, n_head=2, n_layer=2, num_content_vectors=K, vocab_size=VOCAB, n_positions=32,
                         scale_attn_by_inverse_layer_idx=True, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
                         use_flash_attn=False, pad_vocab_size_multiple=8)
    model = BackpackLMHeadModel(cfg).eval()
    with torch.no_grad():
        senses = model.transformer.content_model(torch.arange(VOCAB).unsqueeze(0))[0].transpose(0, 1)   # (V, k, d)
    target = torch.zeros(VOCAB)
    target[[3, 17, 40, 95]] = 1.0
    return model, senses.double().numpy(), model.lm_head.weight.detach().double().numpy(), target


def test_localize_stays_within_the_first_order_bound(nano):
    model, senses, emb, target = nano
    want = R.non_contextual_localize(senses, emb, target.numpy())
    bound = 2 * R.localize_bound(senses, emb, target.numpy(), torch.float32)
    for chunk_rows in (8192, 100, 7):                      # one chunk; partial last chunks; chunks that split a token
        got = SV.non_contextual_localize(target, model, chunk_rows=chunk_rows)
        assert got.shape == (VOCAB, K) and got.dtype == torch.float32
        ratio = (np.abs(got.double().numpy() - want) / bound).max()
        print(f'localize fp32 cpu chunk_rows={chunk_rows}: largest error / allowed = {ratio:.3f}')
        assert ratio <= 1.0
    assert torch.equal(SV.non_contextual_localize(target, model, nv=K, vocsize=VOCAB), SV.non_contextual_localize(target, model))


def test_localize_without_a_sense_table_runs_the_content_network_in_chunks(nano, monkeypatch):
    model, senses, emb, target = nano
    with_table = SV.non_contextual_localize(target, model, chunk_rows=50)
    monkeypatch.setattr(type(model.transformer), 'sense_table', lambda self, verify=False: None)
    want = R.non_contextual_localize(senses, emb, target.numpy())
    bound = 2 * R.localize_bound(senses, emb, target.numpy(), torch.float32)
    got = SV.non_contextual_localize(target, model, chunk_rows=50)
    assert (np.abs(got.double().numpy() - want) <= bound).all()
    assert (np.abs((got - with_table).double().numpy()) <= 2 * bound).all()
    ext = SV.sense_extremes(model, count=5, chunk_rows=50)
    monkeypatch.undo()
    assert torch.equal(ext.top_ids, SV.sense_extremes(model, count=5, chunk_rows=50).top_ids)


def test_rows_from_last_token_id_on_are_zero(nano):
    model, senses, emb, target = nano
    got = SV.non_contextual_localize(target, model, last_token_id=90)
    assert (got[90:] == 0).all() and (got[:90] != 0).any(dim=1).all()
    assert torch.equal(got[:90], SV.non_contextual_localize(target, model)[:90])
    want = R.non_contextual_localize(senses, emb, target.numpy(), last_token_id=90)
    assert (want[90:] == 0).all()
    assert (SV.non_contextual_localize(target, model, last_token_id=0) == 0).all()


def test_nv_and_vocsize_must_match_the_model(nano):
    model, _, _, target = nano
    with pytest.raises(ValueError, match='nv'):
        SV.non_contextual_localize(target, model, nv=K + 1)
    with pytest.raises(ValueError, match='vocsize'):
        SV.non_contextual_localize(target, model, vocsize=VOCAB + 8)
    with pytest.raises(ValueError, match='target_vector'):
        SV.non_contextual_localize(target[:-1], model)


def test_sense_extremes_whole_vocabulary_token_ids_and_contents_agree(nano):
    model, senses, emb, _ = nano
    whole = SV.sense_extremes(model, count=6, chunk_rows=100)
    assert whole.top_ids.shape == (VOCAB, K, 6) and whole.top_ids.dtype == torch.int64
    assert whole.bottom_logits.shape == (VOCAB, K, 6) and whole.top_logits.dtype == torch.float32
    # against the restatement on the logits the fp32 model computes (one GEMM, the same rows)
    with torch.no_grad():
        table = model.transformer.sense_table().reshape(-1, D)
        logits = table @ model.lm_head.weight.t()
    tv, ti, bv, bi = R.row_extremes(logits, 6)
    rows = [5, 17, 95, 5]
    some = SV.sense_extremes(model, token_ids=rows, count=6)
    given = SV.sense_extremes(model, contents=torch.from_numpy(senses[rows]).float(), count=6, chunk_rows=5)
    one = SV.sense_extremes(model, contents=torch.from_numpy(senses[17]).float(), count=6)
    # (the row counts of these GEMMs differ, so the CPU BLAS may round a logit's last bits differently: ids are held exactly
    # -- fp32 logits of drawn weights are nowhere that close -- and logits to a few ulps)
    for name in ('top_ids', 'bottom_ids'):
        assert torch.equal(getattr(some, name), getattr(whole, name)[rows]), name
        assert torch.equal(getattr(given, name), getattr(whole, name)[rows]), name
        assert torch.equal(getattr(one, name), getattr(whole, name)[17:18]), name
    assert (whole.top_ids.numpy() == ti.reshape(VOCAB, K, 6)).all() and (whole.bottom_ids.numpy() == bi.reshape(VOCAB, K, 6)).all()
    for name in ('top_logits', 'bottom_logits'):
        torch.testing.assert_close(getattr(some, name), getattr(whole, name)[rows], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(getattr(given, name), getattr(whole, name)[rows], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(whole.top_logits, torch.from_numpy(tv).view(VOCAB, K, 6), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(whole.bottom_logits, torch.from_numpy(bv).view(VOCAB, K, 6), rtol=1e-5, atol=1e-6)
    text = SV.format_sense_extremes(some, token_ids=rows)
    assert text.count('~~~Positive~~~') == len(rows) * K and str(int(some.top_ids[0, 0, 0])) in text


def test_weights_from_scores_equals_the_restatement():
    perm = torch.randperm(800, generator=torch.Generator().manual_seed(0)).float().view(50, 16)
    for w in ((1.4, 1.2, 1.0, 0.8), [5, 5, 4, 1]):
        got = SV.weights_from_scores(perm, w)
        want = R.weights_from_scores(perm.numpy(), w)
        assert got.shape == (50, 16) and (got.double().numpy() == np.asarray(want, dtype=np.float32).astype(np.float64)).all()
    got = SV.weights_from_scores(perm)
    # quantiles 759.05 / 639.2 / 479.4: 40 scores above the first, 120 and 160 between, 480 below
    assert [(got == torch.tensor(v)).sum().item() for v in (1.4, 1.2, 1.0, 0.8)] == [40, 120, 160, 480]


def test_a_score_equal_to_a_quantile_keeps_the_multiplier_one():
    # plateaus of five equal scores centred on the quantile positions 95 / 80 / 60 of 0 .. 100: whichever neighbours the
    # interpolation takes, the quantiles are exactly 19, 16 and 12 in fp32 and in float64, and fifteen scores equal one
    scores = ((torch.arange(101) + 2) // 5).float().view(101, 1)
    w = (3.0, 2.0, 1.5, 0.5)
    got = SV.weights_from_scores(scores, w)
    assert (got.double().numpy() == R.weights_from_scores(scores.numpy(), w)).all()
    for value, mult in ((20, 3.0), (19, 1.0), (18, 2.0), (17, 2.0), (16, 1.0), (15, 1.5), (13, 1.5), (12, 1.0), (11, 0.5), (0, 0.5)):
        assert (scores == value).any() and (got[scores == value] == mult).all(), (value, mult)


def test_the_three_line_pipeline_builds_a_weighted_model_whose_forward_runs(nano):
    model, _, _, target = nano
    w = (1.4, 1.2, 1.0, 0.8)
    weighted = WeightedBackpackLMHeadModel(model, SV.weights_from_scores(SV.non_contextual_localize(target, model), w), target,
                                           max(w) / 7.5).eval()
    ids = torch.randint(0, VOCAB, (2, 12), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        logits = weighted(ids).logits
        plain = model(ids).logits
    assert logits.shape == plain.shape and torch.isfinite(logits).all()
    assert not torch.equal(logits, plain)


# ---- C ABI and code object ---------------------------------------------------------------------------------------------------------------

def test_row_extremes_signature_and_argument_validation():
    i32, i64, ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert bp_hip.SIGNATURES['bp_row_extremes'] == (i32, [ptr] * 5 + [i32] * 2 + [i64] + [i32] * 2 + [ptr])
    h = bp_hip.lib()
    p, null = ctypes.c_void_p(0x1000), None

    def call(logits=p, tv=p, ti=p, bv=p, bi=p, rows=4, cols=100, stride=100, n=5, dtype=1):
        return h.bp_row_extremes(logits, tv, ti, bv, bi, rows, cols, stride, n, dtype, null)

    assert call(dtype=3) == -1 and call(dtype=-1) == -1
    assert call(n=0) == -3 and call(n=65) == -3 and call(n=101, cols=100) == -3 and call(cols=3, stride=3, n=4) == -3
    assert call(cols=0, stride=0) == -3 and call(cols=2 ** 31 - 8, stride=2 ** 31, n=1) == -3
    assert call(rows=-1) == -3 and call(stride=99) == -3
    assert call(logits=null) == -3
    assert call(logits=ctypes.c_void_p(0x1001)) == -3 and call(logits=ctypes.c_void_p(0x1002), dtype=2) == -3
    assert call(tv=ctypes.c_void_p(0x1002)) == -3 and call(bi=ctypes.c_void_p(0x1001)) == -3
    assert call(rows=0) == 0 and call(rows=0, logits=null) == 0          # a successful no-op
    assert call(tv=null, ti=null, bv=null, bi=null) == 0                 # nothing asked for: no launch
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.row_extremes(torch.zeros(2, 8), 2)
    assert not bp_hip.row_extremes_supported(torch.zeros(2, 8), 2)


sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import kernel_resources as KR  # noqa: E402

KERNELS = ['row_extremes_kernel<float>', 'row_extremes_kernel<BF16>', 'row_extremes_kernel<F16>']


def test_row_extremes_kernels_use_no_scratch_and_at_most_128_registers():
    if not KR.tools_available():
        pytest.skip('llvm-objcopy / clang-offload-bundler / llvm-readelf not found under /opt/rocm')
    import importlib.util
    spec = importlib.util.spec_from_file_location('bp_build_hip', os.path.join(ROOT, 'backpacks-flash-attn_amd', 'build_hip.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()   # no-op when the objects are current
    table = {k['name']: k for k in KR.kernels([os.path.join(KR.BUILD, 'row_extremes.o')])}
    assert sorted(table) == sorted(KERNELS), 'the object holds these kernels and no other'
    for name in KERNELS:
        k = table[name]
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, k
        assert k['vgpr_count'] <= 128 and k['max_flat_workgroup_size'] == 1024, k
