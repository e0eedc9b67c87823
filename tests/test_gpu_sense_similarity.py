"""GPU: bp_sense_similarity (csrc/sense_similarity.hip) and src/utils/sense_similarity.py on the HIP path.

  (a) exact needles   every sense vector is a signed unit spike, or a signed sum of four spikes in an aligned block with a
                      Hadamard sign pattern (norm 2), times a power of two 2^-3 .. 2^3; a word's senses share kind and
                      scale.  Every product, partial sum, squared norm (k is a power of four, so sum_l A[l] too), square
                      root and quotient is then exact and every cosine is one of -1, -1/2, 0, 1/2, 1: the float64
                      restatement (tests/sense_similarity_ref.py) rounded to fp32 IS the answer, and all six outputs are
                      compared bit for bit (a zero's sign aside: the contract leaves it open)
  (b) drawn parity    every output within twice the first-order bound of the restatement
  (c) repeatability   two calls, and a captured graph replayed with cand_index rewritten on the device
  (d) the layer       sense_neighbors, paired scores and evaluate_similarity on Small- and Mini-k4-shaped random models"""
import numpy as np
import pytest
import torch

import sense_similarity_ref as R
from decode_support import DEV, _bp

pytestmark = pytest.mark.gpu

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
OUTPUTS = ('flat', 'min_pair', 'max_pair', 'min_all', 'max_all', 'per_sense')
KS = [1, 4, 16, 64]
DS = [8, 16, 24, 264, 768, 2048]
ROW_TARGETS = [1, 31, 32, 33, 63, 64, 65, 4097]          # ncand * k reaches (or just passes) each of these
HADAMARD = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, 1, -1], [1, -1, -1, 1]], dtype=np.float32)
CANARY = 0x7fc0beef                                        # a NaN no arithmetic produces


def _blocks(d):
    """The aligned blocks of four columns the needles live in: both ends of a row, its middle, the chunk boundaries."""
    return sorted({0, 1, (d // 4) // 2, d // 4 - 1} | ({63, 64} if d > 260 else set()))


def needle_words(rng, n, k, d, distinct=False):
    """(n, k, d) fp32 needle words.  `distinct`: sense l sits alone in column l (needs d >= k), positive, for planted cases."""
    out = np.zeros((n, k, d), dtype=np.float32)
    blocks = _blocks(d)
    for w in range(n):
        scale = np.float32(2.0 ** int(rng.integers(-3, 4)))
        quad = int(rng.integers(2))
        for l in range(k):
            if distinct:
                out[w, l, l] = scale
            elif quad:
                b = blocks[int(rng.integers(len(blocks)))]
                out[w, l, 4 * b:4 * b + 4] = HADAMARD[int(rng.integers(4))] * scale * (1 - 2 * int(rng.integers(2)))
            else:
                b = blocks[int(rng.integers(len(blocks)))]
                out[w, l, 4 * b + int(rng.integers(4))] = scale * (1 - 2 * int(rng.integers(2)))
    return out


def related_words(rng, words, n):
    """n words, each a word of `words` with some of its senses negated."""
    src = words[rng.integers(len(words), size=n)].copy()
    flips = 1 - 2 * rng.integers(2, size=src.shape[:2]).astype(np.float32)
    return src * flips[:, :, None]


def _dev(x, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)
    assert torch.equal(t.float().cpu(), torch.from_numpy(np.ascontiguousarray(x))), 'needles are exact in 16 bits'
    return t


def _no_signed_zero(x):
    return np.where(x == 0, np.float32(0), x.astype(np.float32))


def assert_exact(got, want, what):
    for name in got:
        g, w = got[name].cpu().numpy(), _no_signed_zero(want[name])
        assert g.dtype == np.float32 and g.shape == w.shape, (what, name, g.shape, w.shape)
        same = R.bits_of(_no_signed_zero(g)) == R.bits_of(w)
        assert same.all(), (what, name, int((~same).sum()), g[~same][:4], w[~same][:4])


def _nqs(k):
    top = 64 // k
    return sorted({1, 2, 3, top // 2, top - 1, top} & set(range(1, top + 1)))


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('k', KS)
def test_needles_are_exact_at_every_shape(k, dtype):
    bp = _bp()
    rng = np.random.default_rng(100 + k)
    nqs = _nqs(k)
    cases = [(d, ROW_TARGETS[i % len(ROW_TARGETS)], nqs[i % len(nqs)]) for i, d in enumerate(DS)]
    cases += [(DS[(i + 2) % len(DS)], t, nqs[(i + 1) % len(nqs)]) for i, t in enumerate(ROW_TARGETS)]
    cases += [(768, 64, nq) for nq in nqs] + [(24, 33, 64 // k), (2048, 65, 64 // k)]
    seen = set()
    for d, target, nq in cases:
        ncand = -(-target // k)
        if (d, ncand, nq) in seen:
            continue
        seen.add((d, ncand, nq))
        q = needle_words(rng, nq, k, d)
        cand = np.concatenate([related_words(rng, q, ncand - ncand // 2), needle_words(rng, ncand // 2, k, d)])[:ncand]
        cand = cand[rng.permutation(ncand)]
        got = bp.sense_similarity(_dev(cand, DTYPES[dtype]), _dev(q, DTYPES[dtype]))
        want = R.measures(q, cand)
        assert np.isin(want['per_sense'], [-1, -.5, 0, .5, 1]).all()
        assert_exact(got, want, (k, d, ncand, nq, dtype))
    torch.cuda.synchronize()


def test_needle_values_cover_all_five_cosines_and_the_fraction_of_agreeing_senses():
    """The planted flat measure: a candidate that negates j of the k senses of the query has Cos = (k - 2 j) / k."""
    bp = _bp()
    rng = np.random.default_rng(5)
    for k in KS:
        d = max(8, k)
        q = needle_words(rng, 1, k, d, distinct=True)
        cand = np.repeat(q, k + 1, axis=0)
        for j in range(k + 1):
            cand[j, :j] *= -1
        for dtype in DTYPES.values():
            got = bp.sense_similarity(_dev(cand, dtype), _dev(q, dtype))
            want = np.array([(k - 2 * j) / k for j in range(k + 1)], dtype=np.float32)
            assert (got['flat'].cpu().numpy()[0] == want).all(), (k, got['flat'])
            assert_exact(got, R.measures(q, cand), ('flat', k))
            if k > 1:
                assert got['min_pair'][0, 1:k].eq(-1).all() and got['max_pair'][0, 1:k].eq(1).all()
                assert got['min_all'][0, 1:k].eq(-1).all() and got['max_all'][0, 0] == 1 and got['min_all'][0, 0] == 0


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('k', KS)
def test_one_matched_sense_moves_the_pair_measures(k, dtype):
    """One matched sense at -1, the rest at 1 (and the mirror image): walked over every sense in one call."""
    bp = _bp()
    d = {1: 8, 4: 24, 16: 264, 64: 768}[k]
    q = needle_words(np.random.default_rng(k), 1, k, d, distinct=True)
    cand = np.repeat(q, 2 * k, axis=0)
    for l in range(k):
        cand[l, l] *= -1                 # candidate l: sense l at -1, the rest at 1
        cand[k + l] *= -1                # candidate k + l: sense l at 1, the rest at -1
        cand[k + l, l] *= -1
    got = {n: t.cpu().numpy() for n, t in bp.sense_similarity(_dev(cand, DTYPES[dtype]), _dev(q, DTYPES[dtype])).items()}
    assert_exact({n: torch.from_numpy(v) for n, v in got.items()}, R.measures(q, cand), (k, dtype))
    rest = 1.0 if k > 1 else -1.0
    assert (got['min_pair'][0, :k] == -1).all() and (got['min_all'][0, :k] == -1).all() and (got['max_pair'][0, :k] == rest).all()
    assert (got['max_pair'][0, k:] == 1).all() and (got['max_all'][0, k:] == 1).all() and (got['min_pair'][0, k:] == -rest).all()
    assert (got['per_sense'][0, :, :k] == 1 - 2 * np.eye(k)).all() and (got['per_sense'][0, :, k:] == 2 * np.eye(k) - 1).all()


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('k', [4, 16, 64])
def test_one_off_diagonal_pair_moves_min_all_and_not_min_pair(k, dtype):
    """Query t has sense l' = -(sense l), everything else orthogonal; against itself the diagonal is all ones and
    cos[l', l] = cos[l, l'] = -1: min_all moves, min_pair does not.  Against its negation: the mirror image for max.
    Walked over every ordered pair (l', l), one single-query call with two gathered candidates each."""
    bp = _bp()
    d = {4: 8, 16: 24, 64: 264}[k]
    pairs = [(lq, l) for lq in range(k) for l in range(k) if lq != l]
    base = needle_words(np.random.default_rng(k), 1, k, d, distinct=True)[0]
    words = np.repeat(base[None], len(pairs), axis=0)
    for t, (lq, l) in enumerate(pairs):
        words[t, l] = -words[t, lq]
    table = _dev(np.concatenate([words, -words]), DTYPES[dtype])
    index = torch.stack([torch.arange(len(pairs)), torch.arange(len(pairs)) + len(pairs)], 1).to(DEV, torch.int32)
    names = ('min_pair', 'max_pair', 'min_all', 'max_all')
    out = {n: torch.empty((len(pairs), 1, 2), dtype=torch.float32, device=DEV) for n in names}
    for t in range(len(pairs)):
        bp.sense_similarity(table, table[t:t + 1], cand_index=index[t], want=names, out={n: out[n][t] for n in names})
    got = {n: out[n][:, 0].cpu().numpy() for n in names}
    assert (got['min_all'][:, 0] == -1).all() and (got['min_pair'][:, 0] == 1).all() and (got['max_all'][:, 0] == 1).all()
    assert (got['max_all'][:, 1] == 1).all() and (got['max_pair'][:, 1] == -1).all() and (got['min_all'][:, 1] == -1).all()


@pytest.mark.parametrize('dtype', sorted(DTYPES))
def test_gathered_candidates_strided_views_canaries_and_null_outputs(dtype):
    """Candidates by index (repeated, out of range and negative ones clamp as unsigned numbers to the last row), table and
    query as strided views, NaN in every table row no candidate names and in the padding of every row, canaries behind
    every output, a zero sense row whose NaNs land in exactly its own column, and subsets of the outputs."""
    bp = _bp()
    k, d, rows, nq = 4, 24, 40, 5
    rng = np.random.default_rng(11)
    q = needle_words(rng, nq, k, d)
    words = np.concatenate([related_words(rng, q, rows // 2), needle_words(rng, rows - rows // 2, k, d)])
    words[7, 2] = 0                                                    # a zero sense vector
    named = [3, 3, 10 ** 6, -1, 0, 7, 2 ** 31 - 1, -2 ** 31, 21, 7, 39, 12]
    rows_read = [min(i % 2 ** 32, rows - 1) for i in named]
    t_buf = torch.full((rows, k + 1, d + 8), float('nan'), dtype=DTYPES[dtype], device=DEV)
    table = t_buf[:, :k, :d]
    for r in set(rows_read):
        table[r] = _dev(words[r], DTYPES[dtype])
    q_buf = torch.full((nq, k + 2, d + 16), float('nan'), dtype=DTYPES[dtype], device=DEV)
    query = q_buf[:, 1:k + 1, 8:d + 8]
    query.copy_(_dev(q, DTYPES[dtype]))
    assert not table.is_contiguous() and not query.is_contiguous()
    index = torch.tensor(named, dtype=torch.int64).to(torch.int32).to(DEV)
    ncand = len(named)
    want, bound = R.measures(q, words[rows_read]), R.bounds(q, words[rows_read])
    canary = torch.tensor([CANARY], dtype=torch.int32).view(torch.float32).item()
    for subset in (OUTPUTS, ('min_pair',), ('per_sense',), ('flat', 'max_all'), ('min_all', 'per_sense')):
        pair_buf = torch.full((5, nq, ncand + 3), canary, dtype=torch.float32, device=DEV)
        ps_buf = torch.full((nq, k, ncand + 5), canary, dtype=torch.float32, device=DEV)
        out = {n: pair_buf[i, :, :ncand] for i, n in enumerate(OUTPUTS[:5]) if n in subset}
        if 'per_sense' in subset:
            out['per_sense'] = ps_buf[:, :, :ncand]
        got = bp.sense_similarity(table, query, cand_index=index, want=subset, out=out)
        assert sorted(got) == sorted(subset)
        for n in subset:
            g, w = got[n].cpu().numpy(), want[n]
            assert (np.isnan(g) == np.isnan(w)).all(), (n, subset)
            live = ~np.isnan(w)
            if n == 'flat':     # a word with a zero sense has sum_l B[l] = 3 s^2: its square root is no fp32 number
                assert (np.abs(g - w)[:, [5, 9]] <= 2 * bound['flat'][:, [5, 9]]).all()
                live[:, [5, 9]] = False
            assert (R.bits_of(_no_signed_zero(g))[live] == R.bits_of(_no_signed_zero(w))[live]).all(), (n, subset)
        bits = pair_buf.view(torch.int32)
        assert (bits[:, :, ncand:] == CANARY).all() and (ps_buf.view(torch.int32)[:, :, ncand:] == CANARY).all()
        for i, n in enumerate(OUTPUTS[:5]):
            if n not in subset:
                assert (bits[i] == CANARY).all(), n
        if 'per_sense' not in subset:
            assert (ps_buf.view(torch.int32) == CANARY).all()
    # the zero row (table row 7, sense 2: candidates 5 and 9): NaN in its own sense, in the four min / max measures of its
    # candidates, and nowhere else -- the flat cosine of a word with one zero sense is a number
    nan = {n: np.isnan(v) for n, v in want.items()}
    cols = np.zeros(ncand, dtype=bool)
    cols[[5, 9]] = True
    for n in ('min_pair', 'max_pair', 'min_all', 'max_all'):
        assert (nan[n] == cols[None, :]).all(), n
    assert not nan['flat'].any() and nan['per_sense'][:, 2][:, cols].all() and nan['per_sense'].sum() == nq * 2


DRAWN = [(16, 768, 300, 4), (4, 640, 129, 16), (64, 384, 33, 1), (1, 768, 1000, 64)]


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('shape', DRAWN, ids=[f'k{s[0]}-d{s[1]}-c{s[2]}-q{s[3]}' for s in DRAWN])
def test_drawn_operands_stay_within_twice_the_first_order_bound(shape, dtype):
    bp = _bp()
    k, d, ncand, nq = shape
    g = torch.Generator().manual_seed(k * 1000 + d)
    table = torch.randn(ncand, k, d, generator=g).to(DTYPES[dtype])
    query = torch.randn(nq, k, d, generator=g).to(DTYPES[dtype])
    query[0] = table[ncand // 2]                                       # one identical word: cosines at 1
    a, b = query.double().numpy(), table.double().numpy()
    want, bound = R.measures(a, b), R.bounds(a, b)
    got = bp.sense_similarity(table.to(DEV), query.to(DEV))
    worst = {n: R.worst_ratio(got[n].cpu().numpy(), want[n], bound[n], factor=2.0) for n in OUTPUTS}
    print(f'sense_similarity {dtype} k={k} d={d} ncand={ncand} nq={nq}: largest error / allowed = '
          + ', '.join(f'{n} {v:.3f}' for n, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_two_calls_and_graph_replays_agree_bit_for_bit():
    bp = _bp()
    k, d, rows, nq, ncand = 16, 768, 500, 4, 300
    g = torch.Generator().manual_seed(3)
    table = torch.randn(rows, k, d, generator=g).to(DEV, torch.bfloat16)
    query = torch.randn(nq, k, d, generator=g).to(DEV, torch.bfloat16)
    lists = [torch.randint(0, rows, (ncand,), generator=g).to(DEV, torch.int32) for _ in range(3)]
    first = bp.sense_similarity(table, query, cand_index=lists[0])
    again = bp.sense_similarity(table, query, cand_index=lists[0])
    for n in OUTPUTS:
        assert torch.equal(first[n].view(torch.int32), again[n].view(torch.int32)), n
    index = lists[0].clone()
    out = {n: torch.empty_like(first[n]) for n in OUTPUTS}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        bp.sense_similarity(table, query, cand_index=index, out=out)   # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bp.sense_similarity(table, query, cand_index=index, out=out)
    for lst in lists[::-1]:
        index.copy_(lst)                                               # rewritten on the device: the host never read it
        graph.replay()
        torch.cuda.synchronize()
        eager = bp.sense_similarity(table, query, cand_index=lst)
        for n in OUTPUTS:
            assert torch.equal(out[n].view(torch.int32), eager[n].view(torch.int32)), n


# ---- the layer ---------------------------------------------------------------------------------------------------------------------------

SHAPES = {'small': dict(n_embd=768, n_head=12, num_content_vectors=16), 'mini_k4': dict(n_embd=640, n_head=8, num_content_vectors=4)}
VOCAB = 300                       # padded to 304 rows


@pytest.fixture(scope='module', params=sorted(SHAPES))
def model(request):
    import warnings
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    _bp()
    torch.manual_seed(7)
    cfg = BackpackConfig(n_layer=2, vocab_size=VOCAB, n_positions=32, scale_attn_by_inverse_layer_idx=True, resid_pdrop=0.0,
                         embd_pdrop=0.0, attn_pdrop=0.0, use_flash_attn=True, pad_vocab_size_multiple=8, **SHAPES[request.param])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return BackpackLMHeadModel(cfg).to(DEV, torch.bfloat16).eval()


def test_neighbors_are_the_row_extremes_of_the_block_the_kernel_produced(model):
    from src.utils import sense_similarity as SS
    bp = _bp()
    table = model.transformer.sense_table()
    k = table.shape[1]
    assert table.shape[0] == 304 and bp.sense_similarity_supported(table, table[:2])
    words = [5, [17, 40], 299, 5] + list(range(60, 60 + 64 // k))       # more than one query group
    queries = SS.sense_vectors(model, words)
    assert torch.equal(queries[0], table[5]) and torch.equal(queries[1], table[[17, 40]].float().mean(0).to(table.dtype))
    for measure, output, sense in (('MinPair', 'min_pair', None), ('Cos', 'flat', None), (f'CosSense{k - 1}', 'per_sense', k - 1)):
        for largest in (True, False):
            ids, scores = SS.sense_neighbors(model, words, count=10, measure=measure, largest=largest)
            assert ids.shape == (len(words), 10) and ids.dtype == torch.int64 and scores.dtype == torch.float32
            assert int(ids.max()) < VOCAB, 'the padded rows are no words'
            step = 64 // k
            for q0 in range(0, len(words), step):
                block = bp.sense_similarity(table[:VOCAB], queries[q0:q0 + step], want=(output,))[output]
                block = block if sense is None else block[:, sense]
                tv, ti, bv, bi = bp.row_extremes(block.contiguous(), 10)
                assert torch.equal(ids[q0:q0 + step], (ti if largest else bi).long())
                assert torch.equal(scores[q0:q0 + step], tv if largest else bv)
    ids, scores = SS.sense_neighbors(model, [5], count=3, measure='MinPair')
    assert ids[0, 0] == 5 and abs(float(scores[0, 0]) - 1.0) < 1e-5       # a word is its own nearest neighbour
    some = [290, 5, 17, 100, 5]
    ids, _ = SS.sense_neighbors(model, [5], count=2, candidates=some)
    assert ids[0].tolist() == [5, 5]
    far, _ = SS.sense_neighbors(model, [5, 17], count=100, measure='MaxAll')   # beyond the kernel's 64 per end: a stable sort
    near, _ = SS.sense_neighbors(model, [5, 17], count=64, measure='MaxAll')
    assert far.shape == (2, 100) and torch.equal(far[:, :64], near)


def test_scores_stay_within_the_bound_of_the_cpu_twin_and_rho_is_one(model, monkeypatch):
    from src.utils import sense_similarity as SS
    table = model.transformer.sense_table()
    k = table.shape[1]
    g = torch.Generator().manual_seed(1)
    first = torch.randint(0, VOCAB, (40,), generator=g).tolist()
    second = torch.randint(0, VOCAB, (40,), generator=g).tolist()
    second[3] = [second[3], 7]                                            # a word of two tokens
    a, b = SS.sense_vectors(model, first), SS.sense_vectors(model, second)
    got = SS.sense_similarity(a, b)
    twin = SS._eager_sense_similarity(b.cpu(), a.cpu())                   # every a against every b
    a64, b64 = a.double().cpu().numpy(), b.double().cpu().numpy()
    want, bound = R.measures(a64, b64), R.bounds(a64, b64)
    pick = np.arange(40)
    worst = 0.0
    for name in SS.measure_names(k):
        output, sense = SS._output_of(name, k)
        w = want[output][pick, pick] if sense is None else want[output][pick, sense, pick]
        bd = bound[output][pick, pick] if sense is None else bound[output][pick, sense, pick]
        tw = twin[output][pick, pick] if sense is None else twin[output][pick, sense, pick]
        worst = max(worst, R.worst_ratio(got[name].cpu().numpy(), w, bd, factor=2.0))
        assert R.worst_ratio(got[name].cpu().numpy(), tw.numpy(), bd, factor=4.0) <= 1.0, name   # both within 2 x of exact
    print(f'layer k={k}: paired scores, largest error / allowed = {worst:.3f}')
    assert worst <= 1.0
    # gold scores that are a monotone function of MinPair: rho = 1 exactly, on the kernel and with the twin forced
    gold = torch.exp(3 * got['MinPair'].double()).cpu().tolist()
    assert len(set(gold)) == len(gold)
    examples = [(x, y, s) for x, y, s in zip(first, second, gold)]
    rho = SS.evaluate_similarity(model, examples)
    assert rho['MinPair'] == 1.0 and set(rho) == set(SS.measure_names(k))
    monkeypatch.setattr(SS, '_force_eager', True)
    rho_twin = SS.evaluate_similarity(model, examples)
    monkeypatch.undo()
    assert rho_twin == rho and rho_twin['MinPair'] == 1.0
    soft = SS.evaluate_similarity(model, examples, use_softmax=True)
    assert list(soft) == ['Cos'] and -1.0 <= soft['Cos'] <= 1.0
