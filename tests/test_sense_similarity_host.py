"""CPU: lexical similarity of sense vectors (src/utils/sense_similarity.py) against the float64 restatement of
tests/sense_similarity_ref.py -- the torch twin of bp_sense_similarity within the first-order bound, NaN propagation, every
function of the layer on the nano configuration, Spearman's rho, the four dataset formats -- and, without a GPU, the C ABI of
bp_sense_similarity (every refusal before any launch) and the register account of its code object."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import bp_hip
import sense_similarity_ref as R
from src.models.backpack import BackpackConfig, BackpackLMHeadModel
from src.utils import sense_similarity as SS

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
OUTPUTS = bp_hip.SIMILARITY_OUTPUTS


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('d', [8, 24, 768])
@pytest.mark.parametrize('k', [1, 3, 4, 16])
def test_the_twin_stays_within_the_first_order_bound(k, d, dtype):
    g = torch.Generator().manual_seed(k * 1000 + d)
    table = torch.randn(37, k, d, generator=g).to(DTYPES[dtype])
    query = torch.randn(5, k, d, generator=g).to(DTYPES[dtype])
    query[1] = table[20]
    index = torch.tensor([3, 3, 36, -1, 10 ** 6, 0, 20], dtype=torch.int32)
    a, b = query.double().numpy(), table.double().numpy()
    for idx, rows in ((None, np.arange(37)), (index, np.array([3, 3, 36, 36, 36, 0, 20]))):
        got = SS._eager_sense_similarity(table, query, cand_index=idx)
        want, bound = R.measures(a, b[rows]), R.bounds(a, b[rows])
        assert sorted(got) == sorted(OUTPUTS)
        worst = {n: R.worst_ratio(got[n].numpy(), want[n], bound[n]) for n in OUTPUTS}
        print(f'twin {dtype} k={k} d={d}: largest error / allowed = ' + ', '.join(f'{n} {v:.3f}' for n, v in worst.items()))
        assert got['flat'].dtype == torch.float32 and got['per_sense'].shape == (5, k, len(rows))
        assert max(worst.values()) <= 1.0, worst
    some = SS._eager_sense_similarity(table, query, cand_index=index, want=('max_all', 'per_sense'))
    assert sorted(some) == ['max_all', 'per_sense'] and torch.equal(some['max_all'], got['max_all'])


def test_the_twin_works_in_chunks(monkeypatch):
    g = torch.Generator().manual_seed(0)
    table, query = torch.randn(50, 4, 16, generator=g), torch.randn(3, 4, 16, generator=g)
    whole = SS._eager_sense_similarity(table, query)
    monkeypatch.setattr(SS, '_EAGER_CHUNK', 7)
    parts = SS._eager_sense_similarity(table, query)
    for n in OUTPUTS:
        torch.testing.assert_close(parts[n], whole[n], rtol=1e-6, atol=1e-6)


def test_a_zero_vector_is_nan_in_exactly_the_measures_that_contain_it():
    g = torch.Generator().manual_seed(1)
    table, query = torch.randn(6, 4, 8, generator=g), torch.randn(3, 4, 8, generator=g)
    table[2, 1] = 0                                      # sense 1 of candidate 2
    query[1, 3] = 0                                      # sense 3 of query 1
    got = {n: torch.isnan(t).numpy() for n, t in SS._eager_sense_similarity(table, query).items()}
    want = {n: np.isnan(v) for n, v in R.measures(query.numpy(), table.numpy()).items()}
    for n in OUTPUTS:
        assert (got[n] == want[n]).all(), n
    pair = np.zeros((3, 6), dtype=bool)
    pair[1, :] = True
    pair[:, 2] = True
    sense = np.zeros((3, 4, 6), dtype=bool)
    sense[1, 3, :] = True
    sense[:, 1, 2] = True
    assert not got['flat'].any() and (got['per_sense'] == sense).all()
    for n in ('min_pair', 'max_pair', 'min_all', 'max_all'):
        assert (got[n] == pair).all(), n
    # a zero query sense meets every candidate in min_all, but only its own sense in min_pair: here both hold it
    table[2, 1] = 1.0
    query[1, 3] = 1.0
    assert not any(torch.isnan(t).any() for t in SS._eager_sense_similarity(table, query).values())


# ---- the layer on the nano configuration --------------------------------------------------------------------------------------------------

VOCAB, K, D = 93, 4, 64           # 96 embedding rows: three of them are padding


@pytest.fixture(scope='module')
def nano():
    torch.manual_seed(3)
    cfg = BackpackConfig(n_embd=D, n_head=2, n_layer=2, num_content_vectors=K, vocab_size=VOCAB, n_positions=32,
                         scale_attn_by_inverse_layer_idx=True, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
                         use_flash_attn=False, pad_vocab_size_multiple=8)
    model = BackpackLMHeadModel(cfg).eval()
    with torch.no_grad():
        senses = model.transformer.content_model(torch.arange(96).unsqueeze(0))[0].transpose(0, 1)   # (96, k, d)
    return model, senses


def test_sense_and_softmax_vectors_pool_multi_token_words(nano, monkeypatch):
    model, senses = nano
    words = [5, [17], [17, 40, 3], 92]
    vec = SS.sense_vectors(model, words)
    assert vec.shape == (4, K, D) and vec.dtype == torch.float32
    torch.testing.assert_close(vec[0], senses[5], rtol=1e-5, atol=1e-6)
    assert torch.equal(vec[1], SS.sense_vectors(model, [17])[0])
    torch.testing.assert_close(vec[2], senses[[17, 40, 3]].mean(0), rtol=1e-5, atol=1e-6)
    first = SS.sense_vectors(model, words, use_first=True)
    assert torch.equal(first[2], vec[1]) and torch.equal(first[0], vec[0])
    monkeypatch.setattr(type(model.transformer), 'sense_table', lambda self, verify=False: None)
    torch.testing.assert_close(SS.sense_vectors(model, words), vec, rtol=1e-5, atol=1e-6)
    monkeypatch.undo()
    soft = SS.softmax_vectors(model, words)
    weight = model.lm_head.weight.detach()
    assert soft.shape == (4, 1, D) and torch.equal(soft[0, 0], weight[5])
    torch.testing.assert_close(soft[2, 0], weight[[17, 40, 3]].mean(0))
    assert torch.equal(SS.softmax_vectors(model, words, use_first=True)[2, 0], weight[17])
    with pytest.raises(ValueError):
        SS.sense_vectors(model, [[]])


def test_paired_scores_are_the_all_pairs_scores_gathered(nano):
    model, senses = nano
    g = torch.Generator().manual_seed(2)
    first = torch.randint(0, VOCAB, (70,), generator=g).tolist()          # repeated words, several query groups (16 a group)
    second = torch.randint(0, VOCAB, (70,), generator=g).tolist()
    a, b = SS.sense_vectors(model, first), SS.sense_vectors(model, second)
    got = SS.sense_similarity(a, b)
    assert list(got) == ['Cos', 'MinPair', 'MaxPair', 'MinAll', 'MaxAll'] + [f'CosSense{l}' for l in range(K)]
    every = SS._eager_sense_similarity(b, a)                              # (70, 70): a[i] against b[j]
    pick = torch.arange(70)
    a64, b64 = a.double().numpy(), b.double().numpy()
    want, bound = R.measures(a64, b64), R.bounds(a64, b64)
    for name in got:
        output, sense = SS._output_of(name, K)
        sel = (pick, pick) if sense is None else (pick, sense, pick)
        assert got[name].shape == (70,) and got[name].dtype == torch.float32
        torch.testing.assert_close(got[name], every[output][sel], rtol=1e-5, atol=1e-6)
        assert R.worst_ratio(got[name].numpy(), want[output][sel], bound[output][sel]) <= 1.0, name
    one = SS.sense_similarity(a, b, measures=['CosSense2', 'MinAll'])
    assert list(one) == ['CosSense2', 'MinAll'] and torch.equal(one['MinAll'], got['MinAll'])
    assert SS.sense_similarity(a[:0], b[:0])['Cos'].shape == (0,)
    with pytest.raises(ValueError):
        SS.sense_similarity(a, b, measures=['CosSense4'])
    with pytest.raises(ValueError):
        SS.sense_similarity(a, b[:3])


def test_neighbors_are_a_stable_sort_of_the_score_matrix(nano):
    model, senses = nano
    table = model.transformer.sense_table()
    assert table.shape == (96, K, D)
    words = [5, [17, 40], 92] + list(range(20, 40))                       # two query groups
    queries = SS.sense_vectors(model, words)
    for measure in ('MinPair', 'Cos', 'MaxAll', 'CosSense1'):
        output, sense = SS._output_of(measure, K)
        block = SS._eager_sense_similarity(table[:VOCAB], queries, want=(output,))[output]
        block = block if sense is None else block[:, sense]
        for largest in (True, False):
            for count in (1, 10, 64, 80):
                ids, scores = SS.sense_neighbors(model, words, count=count, measure=measure, largest=largest)
                assert ids.shape == (len(words), count) and ids.dtype == torch.int64 and scores.dtype == torch.float32
                assert int(ids.max()) < VOCAB, 'the padded embedding rows are no words'
                order = torch.sort(block, dim=1, descending=largest, stable=True).indices[:, :count]
                assert torch.equal(ids, order), (measure, largest, count)
                torch.testing.assert_close(scores, torch.gather(block, 1, order), rtol=1e-5, atol=1e-6)
    ids, scores = SS.sense_neighbors(model, [5], count=1, measure='Cos')
    assert ids.tolist() == [[5]] and scores[0, 0] == pytest.approx(1.0, abs=1e-6)
    some = [90, 5, 17, 95, 5]                                             # a list may name padded rows and repeat itself
    ids, scores = SS.sense_neighbors(model, [5, 17], count=3, measure='MinPair', candidates=some)
    assert ids[0, :2].tolist() == [5, 5] and ids[1, 0] == 17 and set(ids.reshape(-1).tolist()) <= set(some)
    with pytest.raises(ValueError):
        SS.sense_neighbors(model, [5], count=6, candidates=some)
    with pytest.raises(ValueError):
        SS.sense_neighbors(model, [5], measure='Nearest')


def test_evaluate_similarity_is_spearman_of_the_paired_scores(nano):
    model, _ = nano
    g = torch.Generator().manual_seed(4)
    first = torch.randint(0, VOCAB, (30,), generator=g).tolist()
    second = torch.randint(0, VOCAB, (30,), generator=g).tolist()
    second[4] = [second[4], 11]
    sims = SS.sense_similarity(SS.sense_vectors(model, first), SS.sense_vectors(model, second))
    gold = (-2.0 * sims['MaxAll'].double()).tolist()                      # a decreasing function of MaxAll
    examples = [SS.SimilarityExample(x, y, s) for x, y, s in zip(first, second, gold)]
    rho = SS.evaluate_similarity(model, examples)
    assert set(rho) == set(SS.measure_names(K)) and rho['MaxAll'] == -1.0
    for name in rho:
        assert rho[name] == SS.spearman(sims[name], gold) == pytest.approx(R.spearman(sims[name].numpy(), gold), abs=1e-12)
    soft = SS.evaluate_similarity(model, examples, use_softmax=True)
    assert list(soft) == ['Cos']
    a, b = SS.softmax_vectors(model, first), SS.softmax_vectors(model, second)
    cos = torch.nn.functional.cosine_similarity(a[:, 0].double(), b[:, 0].double())
    flat = SS.sense_similarity(a, b, measures=['Cos'])['Cos']
    torch.testing.assert_close(flat.double(), cos, rtol=1e-5, atol=1e-6)
    assert soft['Cos'] == SS.spearman(flat, gold)
    heads = [SS.SimilarityExample(x, y[0] if isinstance(y, list) else y, s) for x, y, s in examples]
    assert SS.evaluate_similarity(model, examples, use_first=True) == SS.evaluate_similarity(model, heads)

    class Tok:                                                             # words as strings: tokenized with a leading space
        def __call__(self, text):
            assert text.startswith(' ')
            return {'input_ids': [int(t) for t in text.split()]}
    text = [SS.SimilarityExample(' '.join(map(str, x if isinstance(x, list) else [x])),
                                 ' '.join(map(str, y if isinstance(y, list) else [y])), s) for x, y, s in examples]
    assert SS.evaluate_similarity(model, text, tokenizer=Tok()) == rho
    assert len(SS.tokenize_examples(text, Tok(), single_token_only=True)) == 29


def test_spearman_with_ties():
    g = np.random.default_rng(0)
    cases = [(g.normal(size=50), g.normal(size=50)), (g.integers(0, 5, 40), g.integers(0, 3, 40)),
             (np.arange(10.0), np.arange(10.0) ** 3), (np.arange(10.0), -np.arange(10.0)), ([1, 1, 2, 2, 3], [5, 5, 5, 6, 7])]
    for x, y in cases:
        assert SS.spearman(x, y) == pytest.approx(R.spearman(x, y), abs=1e-12)
    assert SS.spearman(np.arange(10.0), np.arange(10.0) ** 3) == 1.0 and SS.spearman(torch.arange(5.), -torch.arange(5.)) == -1.0
    assert np.isnan(SS.spearman([1, 1, 1], [1, 2, 3])) and np.isnan(SS.spearman([1, float('nan'), 2], [1, 2, 3]))
    with pytest.raises(ValueError):
        SS.spearman([1, 2], [1, 2, 3])
    stats = pytest.importorskip('scipy.stats')
    for x, y in cases:
        assert SS.spearman(x, y) == pytest.approx(stats.spearmanr(x, y)[0], abs=1e-12)


def test_the_four_dataset_formats(tmp_path):
    files = {
        'simlex999': 'word1\tword2\tPOS\tSimLex999\tconc(w1)\nold\tnew\tA\t1.58\t2.72\nsmart\tintelligent\tA\t9.2\t1.75\n',
        'simverb3500': 'take\tremove\tV\t6.81\tSYNONYMS\nwalk\ttrail\tV\t4.81\tCOHYPONYMS\n',
        'rg65': 'cord;smile;0.02\nrooster;voyage;0.04\n\n',
        'ws353': 'Word 1,Word 2,Human (mean)\nlove,sex,6.77\ntiger,cat,7.35\n',
    }
    want = {'simlex999': [('old', 'new', 1.58), ('smart', 'intelligent', 9.2)],
            'simverb3500': [('take', 'remove', 6.81), ('walk', 'trail', 4.81)],
            'rg65': [('cord', 'smile', 0.02), ('rooster', 'voyage', 0.04)],
            'ws353': [('love', 'sex', 6.77), ('tiger', 'cat', 7.35)]}
    for kind, text in files.items():
        path = tmp_path / (kind + '.txt')
        path.write_text(text)
        got = SS.load_similarity_file(str(path), kind)
        assert [tuple(ex) for ex in got] == want[kind] and got[0].gold_score == want[kind][0][2], kind
    with pytest.raises(ValueError):
        SS.load_similarity_file(str(path), 'men')


# ---- C ABI and code object ---------------------------------------------------------------------------------------------------------------

def test_sense_similarity_signature_and_every_refusal():
    i32, i64, ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert bp_hip.SIGNATURES['bp_sense_similarity'] == (i32, [ptr] * 9 + [i64] + [i32] * 3 + [i64] + [i64] * 7 + [i32, ptr])
    assert bp_hip.SIMILARITY_MAX_QUERY_ROWS == 64
    h = bp_hip.lib()
    p, null = ctypes.c_void_p(0x1000), None

    def call(table=p, index=p, query=p, outs=(p,) * 6, ncand=100, k=16, d=768, nq=4, rows=1000, t_rs=16 * 768, t_gs=768,
             q_qs=16 * 768, q_gs=768, o_qs=100, ps_qs=1600, ps_gs=100, dtype=1):
        return h.bp_sense_similarity(table, index, query, *outs, ncand, k, d, nq, rows, t_rs, t_gs, q_qs, q_gs, o_qs, ps_qs,
                                     ps_gs, dtype, null)

    DTYPE, SHAPE, DOUT = -1, -3, -6
    assert call(dtype=2) == DTYPE and call(dtype=-1) == DTYPE
    assert call(d=0) == DOUT and call(d=12) == DOUT and call(d=2056) == DOUT
    assert call(k=0) == SHAPE and call(k=65) == SHAPE and call(k=128) == SHAPE
    assert call(k=3) == SHAPE and call(k=24) == SHAPE                         # no power of two
    assert call(nq=0) == SHAPE and call(nq=5) == SHAPE and call(k=1, nq=65) == SHAPE and call(k=64, nq=2) == SHAPE
    assert call(nq=2 ** 30) == SHAPE
    assert call(ncand=-1) == SHAPE and call(ncand=2 ** 31) == SHAPE and call(rows=0) == SHAPE and call(rows=2 ** 31) == SHAPE
    assert call(outs=(null,) * 6) == SHAPE
    assert call(index=null, ncand=1001, o_qs=1001, ps_gs=1001, ps_qs=16 * 1001) == SHAPE   # row c must exist
    assert call(table=null) == SHAPE and call(query=null) == SHAPE
    assert call(table=ctypes.c_void_p(0x1008)) == SHAPE and call(query=ctypes.c_void_p(0x1002)) == SHAPE
    assert call(index=ctypes.c_void_p(0x1002)) == SHAPE
    for i in range(6):
        assert call(outs=tuple(ctypes.c_void_p(0x1002) if j == i else p for j in range(6))) == SHAPE
    assert call(t_rs=16 * 768 + 4) == SHAPE and call(t_gs=772) == SHAPE and call(q_qs=16 * 768 + 1) == SHAPE and call(q_gs=770) == SHAPE
    assert call(o_qs=99) == SHAPE and call(ps_gs=99) == SHAPE and call(ps_qs=1599) == SHAPE
    assert call(ncand=0) == 0 and call(ncand=0, table=null, query=null) == 0   # a successful no-op
    assert call(ncand=0, outs=(null,) * 6) == SHAPE
    t, q = torch.zeros(8, 4, 16, dtype=torch.bfloat16), torch.zeros(2, 4, 16, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.sense_similarity(t, q)
    assert not bp_hip.sense_similarity_supported(t, q)


sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import kernel_resources as KR  # noqa: E402

KERNELS = ['sense_similarity_kernel<BF16, 1>', 'sense_similarity_kernel<BF16, 2>', 'sense_similarity_kernel<F16, 1>',
           'sense_similarity_kernel<F16, 2>']


def test_sense_similarity_kernels_use_no_scratch_and_do_not_spill():
    if not KR.tools_available():
        pytest.skip('llvm-objcopy / clang-offload-bundler / llvm-readelf not found under /opt/rocm')
    import importlib.util
    spec = importlib.util.spec_from_file_location('bp_build_hip', os.path.join(ROOT, 'backpacks-flash-attn_amd', 'build_hip.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()   # no-op when the objects are current
    table = {k['name']: k for k in KR.kernels([os.path.join(KR.BUILD, 'sense_similarity.o')])}
    assert sorted(table) == sorted(KERNELS), 'the object holds these kernels and no other'
    for name in KERNELS:
        k = table[name]
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, k
        assert k['max_flat_workgroup_size'] == 256 and k['waves_per_simd'] >= 2, k
