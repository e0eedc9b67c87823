"""CPU: the limited token pick (n-gram blocking, frequency / presence penalties, suppressed ids) -- _eager_pick against the numpy
restatement of tests/pick_lim_ref.py, the generation options on the nano model, the argument checks of bp_pick_token_lim (no
launch, no GPU) and the resources of its kernels."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import bp_hip
import pick_lim_ref as L
import pick_ref as R
from decode_support import PROMPT
from decode_support import _nano_backpack as _backpack
from src.utils.generation import _eager_pick

INF, NAN = float('inf'), float('nan')
SEED, OFFSET = 1234, 77
VOCAB = 200


def _state(seed=SEED, offset=OFFSET):
    return torch.tensor([seed, offset], dtype=torch.int64)


# ---- _eager_pick against the numpy restatement ---------------------------------------------------------------------------------------

def _check(x, seq, counters, **kw):
    """_eager_pick on the rows against L.pick row by row; returns the tokens."""
    batch, vocab = x.shape
    got = _eager_pick(torch.tensor(x), kw.get('do_sample', False), kw.get('temperature', 1.0), kw.get('top_k', 0),
                      kw.get('top_p', 1.0), _state(), torch.tensor(counters), kw.get('repetition_penalty', 1.0),
                      kw.get('eos_token_id'), None, kw.get('min_length', 0), None, None if seq is None else torch.tensor(seq),
                      kw.get('no_repeat_ngram_size', 0), kw.get('frequency_penalty', 0.0), kw.get('presence_penalty', 0.0),
                      kw.get('penalty_begin', 0), kw.get('suppress_tokens')).tolist()
    exact = 0
    for b in range(batch):
        token, z, keep, u, _ = L.pick(x[b], seed=SEED, offset=OFFSET, row=b, counter=int(counters[b]),
                                      seq_row=None if seq is None else seq[b], **kw)
        if keep is None:
            assert got[b] == token, (b, kw, got[b], token)
        else:
            R.assert_draw(got[b], z, keep, u, 1e-9, what=(b, kw))
        exact += got[b] == token
    assert exact >= batch - 1
    return got


def _ngram_rows(n, vocab, cols=40):
    """Histories that hold repeated n-grams, with every edge of the contract: (x, sequences, counters)."""
    rng = np.random.default_rng(100 * n + vocab)
    lengths = [0, n - 1, n, n + 1, cols, cols, cols - 1, cols + 9, 3 * n, cols, -2, cols]
    batch = len(lengths)
    x = (2.0 * rng.standard_normal((batch, vocab))).astype(np.float32)
    seq = rng.integers(0, min(vocab, 3), size=(batch, cols)).astype(np.int64)        # three ids: every n-gram recurs
    seq[1] = seq[2] = seq[3] = 1                                                     # all equal at Lh = n - 1, n, n + 1
    seq[5] = 2                                                                       # an all-equal history
    seq[6, ::2] = vocab + 5                                                          # ids outside the vocabulary inside the n-grams
    seq[6, 1::4] = -3
    seq[7, :] = rng.integers(0, vocab, size=cols)                                    # c > cols: the clamped history
    if n > 1:
        seq[7, cols - (n - 1):] = seq[7, :n - 1]                                     # its last n - 1 ids are its first: a match at i = 0
    seq[9, :] = np.arange(cols) % vocab                                              # row 9: nothing repeats (vocab > cols) or all does
    seq[11, :] = 2 ** 40 + (np.arange(cols) % 2)                                     # only ids outside the vocabulary
    return x, seq, np.array(lengths, dtype=np.int32)


@pytest.mark.parametrize('vocab', [7, 200])
@pytest.mark.parametrize('n', [1, 2, 3, 5])
def test_ngram_blocking_matches_the_numpy_restatement(n, vocab):
    x, seq, counters = _ngram_rows(n, vocab)
    for kw in (dict(), dict(do_sample=True, temperature=0.8, top_k=3), dict(do_sample=True, top_p=0.7),
               dict(repetition_penalty=1.3, eos_token_id=1, min_length=50)):
        _check(x, seq, counters, no_repeat_ngram_size=n, **kw)
    # what the cases are there for
    h = L.clamped_history(seq[1], counters[1])
    assert len(h) == n - 1 and L.ngram_set(h, n, vocab) == set()
    assert L.ngram_set(L.clamped_history(seq[2], counters[2]), n, vocab) == {1}
    assert L.ngram_set(L.clamped_history(seq[5], counters[5]), n, vocab) == {2}
    assert L.ngram_set(L.clamped_history(seq[11], counters[11]), n, vocab) == set()
    if n > 1:
        assert len(L.clamped_history(seq[7], counters[7])) == seq.shape[1]
        assert int(seq[7, n - 1]) in L.ngram_set(L.clamped_history(seq[7], counters[7]), n, vocab)
    if n == 3:      # row 6 ends on (-3, vocab + 5): ids outside the vocabulary match each other, and what followed them is banned
        assert int(seq[6, 3]) in L.ngram_set(L.clamped_history(seq[6], counters[6]), n, vocab)


def test_ngram_set_by_hand():
    assert L.ngram_set([1, 2, 3, 1, 2], 3, 10) == {3}
    assert L.ngram_set([1, 2, 3, 1, 2], 2, 10) == {3}
    assert L.ngram_set([1, 2, 3, 1, 2], 1, 10) == {1, 2, 3}
    assert L.ngram_set([5, 5, 5], 2, 10) == {5} and L.ngram_set([5, 5, 5], 3, 10) == {5} and L.ngram_set([5, 5, 5], 4, 10) == set()
    assert L.ngram_set([1, 2, 9, 1, 3], 3, 10) == set()                       # differs in the last compared position
    assert L.ngram_set([4, 2, 9, 1, 2], 3, 10) == set()                       # in the first
    assert L.ngram_set([99, -1, 3, 99, -1], 3, 10) == {3} and L.ngram_set([99, -1, 30, 99, -1], 3, 10) == set()
    x = np.zeros((1, 10), dtype=np.float32)
    x[0, 3], x[0, 7] = 2.0, 1.0
    seq = np.array([[1, 2, 3, 1, 2, 0]], dtype=np.int64)
    assert _check(x, seq, np.array([5], dtype=np.int32), no_repeat_ngram_size=3) == [7]
    assert _check(x, seq, np.array([4], dtype=np.int32), no_repeat_ngram_size=3) == [3]      # the history ends one early
    assert _check(x, seq, np.array([5], dtype=np.int32), no_repeat_ngram_size=4) == [3]


PENALTIES = [(0.5, 0.25), (0.5, 0.0), (0.0, 0.75), (-0.5, -0.25), (1.5, -0.5)]


@pytest.mark.parametrize('vocab', [7, 200])
@pytest.mark.parametrize('penalties', PENALTIES, ids=str)
def test_count_penalties_match_the_numpy_restatement(penalties, vocab):
    fp, pp = penalties
    rng = np.random.default_rng(vocab)
    batch, cols = 10, 48
    x = (2.0 * rng.standard_normal((batch, vocab))).astype(np.float32)
    x[3, 2] = NAN                                      # a NaN and infinities pass through
    x[4, 1], x[4, 3] = INF, -INF
    seq = rng.integers(0, min(vocab, 12), size=(batch, cols)).astype(np.int64)
    seq[:, 7], seq[:, 8], seq[:, 9] = -1, vocab, 2 ** 40
    counters = np.array([0, 1, 20, 48, 48, 60, 20, 20, 33, 5], dtype=np.int32)
    for begin in (0, 10, 20, 48, 1000):                # at 0, in the middle, at Lh (rows 2, 6, 7), at and beyond every Lh
        for kw in (dict(), dict(do_sample=True, temperature=0.9, top_k=4), dict(repetition_penalty=1.25, do_sample=True, top_p=0.8)):
            _check(x, seq, counters, frequency_penalty=fp, presence_penalty=pp, penalty_begin=begin, **kw)
    # by hand: the id seen twice loses 2 a_f + a_p, the one in front of penalty_begin nothing
    y = np.array([[3.0, 3.0, 3.0, 3.0]], dtype=np.float32)
    hand = np.array([[0, 1, 1, 2]], dtype=np.int64)
    z = L.values(y[0], None, hand[0], 4, 4, frequency_penalty=0.5, presence_penalty=0.25, penalty_begin=1)
    assert z.tolist() == [3.0, 3.0 - 1.25, 3.0 - 0.75, 3.0]
    assert _check(y, hand, np.array([4], dtype=np.int32), frequency_penalty=0.5, presence_penalty=0.25, penalty_begin=1) == [0]
    assert _check(y, hand, np.array([4], dtype=np.int32), frequency_penalty=-0.5, presence_penalty=0.0, penalty_begin=1) == [1]


def test_suppressed_ids_and_rows_with_nothing_left():
    rng = np.random.default_rng(5)
    x = (2.0 * rng.standard_normal((6, VOCAB))).astype(np.float32)
    best = [int(np.argmax(r)) for r in x]
    suppress = [best[0], best[0], best[1], -1, VOCAB, 2 ** 31 - 1, best[2]]          # duplicates and ids outside the vocabulary
    counters = np.zeros(6, dtype=np.int32)
    for kw in (dict(), dict(do_sample=True), dict(do_sample=True, top_k=2), dict(do_sample=True, top_p=0.3)):
        for st in (suppress, torch.tensor(suppress, dtype=torch.int32)):
            got = _check(x, None, counters, suppress_tokens=st, **kw)
            assert not set(got) & {best[0], best[1], best[2]}
    # every id banned: nothing finite is left, the greedy answer of a row of -inf is index 0 -- a banned id
    assert _check(x, None, counters, suppress_tokens=list(range(VOCAB))) == [0] * 6
    assert _check(x, None, counters, suppress_tokens=list(range(VOCAB)), do_sample=True, top_k=3) == [0] * 6
    small = (2.0 * rng.standard_normal((2, 5))).astype(np.float32)
    seq = np.array([[0, 1, 2, 3, 4], [0, 1, 2, 3, 3]], dtype=np.int64)
    got = _check(small, seq, np.array([5, 5], dtype=np.int32), no_repeat_ngram_size=1, do_sample=True)
    assert got[0] == 0 and got[1] == 4
    # everything at once
    seq = rng.integers(0, 6, size=(6, 30)).astype(np.int64)
    _check(x, seq, np.full(6, 30, dtype=np.int32), suppress_tokens=suppress, no_repeat_ngram_size=2, frequency_penalty=0.5,
           presence_penalty=0.25, penalty_begin=7, repetition_penalty=1.2, eos_token_id=3, min_length=40, do_sample=True, top_k=20,
           top_p=0.9, temperature=0.7)


def test_the_restated_hash_plants_collisions():
    for cols in (1, 5, 1024, 8191):
        slots = L.table_slots(cols)
        assert slots >= 2 * cols and slots & (slots - 1) == 0 and (slots == 2 or slots < 4 * cols)
        ids = L.colliding_ids(cols, 2 ** 19, 4)
        assert len({L.table_slot(t, cols) for t in ids}) == 1 and len(set(ids)) == 4
        assert all(0 <= L.table_slot(t, cols) < slots for t in range(0, 2 ** 19, 4099))
    assert L.lds_bytes(50264, 1024, repetition_penalty=1.2, no_repeat_ngram_size=3, frequency_penalty=0.5) == 68112 + 2 * 6288 + 8192


# ---- generation on the nano model ----------------------------------------------------------------------------------------------------

NEW = 40


def _repeated_ngrams(row, n):
    seen, again = set(), []
    for i in range(len(row) - n + 1):
        gram = tuple(row[i:i + n])
        if gram in seen:
            again.append(gram)
        seen.add(gram)
    return again


@pytest.fixture(scope='module')
def nano():
    model = _backpack()
    ids = torch.randint(0, VOCAB, (3, PROMPT), generator=torch.Generator().manual_seed(1))
    free = model.generate(ids, PROMPT + NEW, kv_cache=True)
    return model, ids, free


def _teacher_forced(model, out, **limits):
    """Every greedy pick of `out` against the restatement on the logits of the full forward; a pick is checked where the two
    best values are further apart than the rounding of a 384-term fp32 dot product.  Returns the number of checked picks."""
    with torch.no_grad():
        logits = model(out).logits.float().numpy()
    checked = 0
    for b in range(out.shape[0]):
        row = out[b].tolist()
        for t in range(PROMPT, out.shape[1]):
            v = L.values(logits[b, t - 1], None, row, t, VOCAB, penalty_begin=PROMPT, **limits)
            top2 = np.sort(v)[-2:]
            if top2[1] - top2[0] > 384 * 2.0 ** -23 * np.abs(logits[b, t - 1]).max():
                assert int(out[b, t]) == int(np.argmax(v)), (b, t, limits)
                checked += 1
    return checked


def test_no_repeat_ngram_size_removes_the_repeated_bigrams(nano):
    model, ids, free = nano
    n = PROMPT + NEW
    assert free.shape == (3, n - 1)
    assert sum(len(_repeated_ngrams(r.tolist(), 2)) for r in free) >= 3, 'the free run repeats no bigram: a weak test'
    out = model.generate(ids, n, kv_cache=True, no_repeat_ngram_size=2)
    assert out.shape == free.shape and torch.equal(out[:, :PROMPT], ids)
    assert all(not _repeated_ngrams(r.tolist(), 2) for r in out)
    assert _teacher_forced(model, out, no_repeat_ngram_size=2) >= 3 * (NEW - 1) - 3
    tri = model.generate(ids, n, kv_cache=True, no_repeat_ngram_size=3)
    assert all(not _repeated_ngrams(r.tolist(), 3) for r in tri)
    drawn = model.sample(ids, n, kv_cache=True, no_repeat_ngram_size=2, rng_state=_state(), top_k=5)
    assert all(not _repeated_ngrams(r.tolist(), 2) for r in drawn)


def test_suppressed_tokens_never_appear(nano):
    model, ids, free = nano
    n = PROMPT + NEW
    common = [int(t) for t in torch.bincount(free[:, PROMPT:].reshape(-1), minlength=VOCAB).topk(4).indices]
    for st in (common, torch.tensor(common)):
        out = model.generate(ids, n, kv_cache=True, suppress_tokens=st)
        assert not np.isin(out[:, PROMPT:].numpy(), common).any() and torch.equal(out[:, :PROMPT], ids)
        drawn = model.sample(ids, n, kv_cache=True, suppress_tokens=st, rng_state=_state(), temperature=0.9)
        assert not np.isin(drawn[:, PROMPT:].numpy(), common).any()
    assert _teacher_forced(model, out, suppress_tokens=common) >= 3 * (NEW - 1) - 3


def test_frequency_and_presence_penalties_change_the_tokens_as_the_restatement_says(nano):
    model, ids, free = nano
    n = PROMPT + NEW
    for fp, pp in ((0.5, 0.25), (2.0, 0.0), (0.0, 1.5)):
        out = model.generate(ids, n, kv_cache=True, frequency_penalty=fp, presence_penalty=pp)
        assert not torch.equal(out, free), 'the penalties changed nothing: a weak test'
        assert _teacher_forced(model, out, frequency_penalty=fp, presence_penalty=pp) >= 3 * (NEW - 1) - 3
    # the prompt is not counted: a prompt token is as likely as before until it has been generated once
    first = model.generate(ids, PROMPT + 2, kv_cache=True, frequency_penalty=100.0, presence_penalty=100.0)
    assert torch.equal(first, free[:, :PROMPT + 1])


def test_intervened_wrapper_takes_the_limits(nano):
    from src.models.intervened_models import WeightedBackpackLMHeadModel
    model, ids, _ = nano
    cw = torch.rand(VOCAB, model.config.num_content_vectors, generator=torch.Generator().manual_seed(11)) * 3
    wrapper = WeightedBackpackLMHeadModel(model, cw, None, 0.1, anneal=False, upweight_nearby=True).eval()
    n = PROMPT + NEW
    free = wrapper.generate(ids, n, kv_cache=True, device_pick=True)
    banned = [int(free[0, PROMPT]), int(free[1, PROMPT + 1])]
    out = wrapper.generate(ids, n, kv_cache=True, no_repeat_ngram_size=2, suppress_tokens=banned, frequency_penalty=0.5)
    assert all(not _repeated_ngrams(r.tolist(), 2) for r in out) and not np.isin(out[:, PROMPT:].numpy(), banned).any()
    s = wrapper.sample(ids, n, kv_cache=True, no_repeat_ngram_size=2, suppress_tokens=banned, rng_state=_state(), top_k=4)
    assert all(not _repeated_ngrams(r.tolist(), 2) for r in s) and not np.isin(s[:, PROMPT:].numpy(), banned).any()


def test_the_limits_need_the_kv_cache_and_sane_values(nano):
    model, ids, _ = nano
    for kw in (dict(no_repeat_ngram_size=2), dict(frequency_penalty=0.5), dict(presence_penalty=0.5), dict(suppress_tokens=[3])):
        for cg in (False, True):
            with pytest.raises(ValueError, match='kv_cache'):
                model.generate(ids, PROMPT + 2, cg=cg, **kw)
            with pytest.raises(ValueError, match='kv_cache'):
                model.sample(ids, PROMPT + 2, cg=cg, **kw)
        with pytest.raises(ValueError, match='beam_search takes no'):
            model.beam_search(ids, PROMPT + 2, 2, **kw)
    for kw in (dict(no_repeat_ngram_size=-1), dict(frequency_penalty=NAN), dict(presence_penalty=INF), dict(frequency_penalty=-INF)):
        with pytest.raises(ValueError):
            model.generate(ids, PROMPT + 2, kv_cache=True, **kw)
        with pytest.raises(ValueError):
            model.sample(ids, PROMPT + 2, kv_cache=True, **kw)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------

def test_pick_token_lim_rejects_bad_arguments_before_any_launch():
    h = bp_hip.lib()
    assert h.bp_abi_version() == 11
    p, null = ctypes.c_void_p(0x1000), None

    def call(logits=p, tokens=p, sequences=p, stats=null, rng=p, counters=null, finished=p, batch=2, vocab=100, row_stride=100,
             tokens_stride=1, seq_stride=8, seq_cols=8, do_sample=1, temperature=1.0, top_k=0, top_p=1.0, theta=1.2, eos=7,
             pad=7, min_length=0, ngram=3, fp=0.5, pp=0.25, begin=2, suppress=p, n_suppress=4, dtype=1):
        return h.bp_pick_token_lim(logits, tokens, sequences, stats, rng, counters, finished, batch, vocab, row_stride,
                                   tokens_stride, seq_stride, seq_cols, do_sample, temperature, top_k, top_p, theta, eos, pad,
                                   min_length, ngram, fp, pp, begin, suppress, n_suppress, dtype, null)
    # everything bp_pick_token and bp_pick_token_ctl reject, with their codes
    assert call(dtype=3) == -1 and call(dtype=-1) == -1
    for kw in (dict(batch=0), dict(vocab=0), dict(vocab=2 ** 23 + 1, row_stride=2 ** 24), dict(row_stride=99),
               dict(tokens_stride=0), dict(logits=null), dict(tokens=null),
               dict(sequences=p, seq_cols=0, seq_stride=8), dict(sequences=p, seq_cols=8, seq_stride=7),
               dict(logits=ctypes.c_void_p(0x1001)), dict(logits=ctypes.c_void_p(0x1002), dtype=2),
               dict(tokens=ctypes.c_void_p(0x1004)), dict(stats=ctypes.c_void_p(0x1002)),
               dict(counters=ctypes.c_void_p(0x1002)), dict(rng=ctypes.c_void_p(0x1004))):
        assert call(**kw) == -3, kw
    for bad in (0.0, -1.0, NAN, INF, 1e-45):
        assert call(temperature=bad) == -4, bad
        assert call(temperature=bad, do_sample=0) == -4, bad
    for bad in (0.0, -0.5, 1.0000001, NAN):
        assert call(top_p=bad) == -10, bad
    assert call(rng=null) == -10
    for bad in (0.0, -1.0, NAN, INF, -INF):
        assert call(theta=bad) == -10, bad
    assert call(sequences=null, seq_stride=0, seq_cols=0, ngram=0, fp=0.0, pp=0.0) == -10     # theta != 1 without a history
    assert call(finished=null) == -10
    for kw in (dict(eos=100), dict(eos=2 ** 20), dict(pad=-1), dict(pad=100), dict(min_length=-1),
               dict(finished=ctypes.c_void_p(0x1002)), dict(vocab=2 ** 19 + 1, row_stride=2 ** 20)):
        assert call(**kw) == -3, kw
    # its own: BP_ERR_SAMPLING
    for bad in (NAN, INF, -INF):
        assert call(fp=bad) == -10 and call(pp=bad) == -10 and call(fp=bad, do_sample=0) == -10, bad
    no_seq = dict(sequences=null, seq_stride=0, seq_cols=0, theta=1.0)
    assert call(ngram=3, fp=0.0, pp=0.0, **no_seq) == -10
    assert call(ngram=0, fp=0.5, pp=0.0, **no_seq) == -10
    assert call(ngram=0, fp=0.0, pp=-0.5, **no_seq) == -10
    assert call(suppress=null) == -10 and call(suppress=ctypes.c_void_p(0x1002)) == -10
    # BP_ERR_SHAPE
    only_ban = dict(theta=1.0, fp=0.0, pp=0.0)
    for kw in (dict(ngram=-1), dict(ngram=65), dict(n_suppress=-1), dict(begin=-1),
               dict(vocab=2 ** 19 + 1, row_stride=2 ** 20, ngram=0, n_suppress=1, **only_ban),
               dict(vocab=2 ** 19 + 1, row_stride=2 ** 20, ngram=2, n_suppress=0, **only_ban),
               dict(vocab=2 ** 19 + 1, row_stride=2 ** 20, ngram=0, n_suppress=0, theta=1.0, fp=0.0, pp=0.5),
               dict(seq_cols=8192, seq_stride=8192), dict(seq_cols=8192, seq_stride=8192, fp=0.0, do_sample=0),
               # LDS: at 2^19 entries one bitmap fits (132.1 KB in all), two do not, nor does one next to a large table
               dict(vocab=2 ** 19, row_stride=2 ** 19, fp=0.0, pp=0.0),
               dict(vocab=2 ** 19, row_stride=2 ** 19, ngram=0, n_suppress=0, theta=1.0, seq_cols=4096, seq_stride=4096)):
        assert call(**kw) == -3, kw
        assert L.lds_bytes(kw.get('vocab', 100), kw.get('seq_cols', 8), kw.get('theta', 1.2), kw.get('ngram', 3), kw.get('fp', 0.5),
                           kw.get('pp', 0.25), kw.get('n_suppress', 4)) > L.MAX_LDS_BYTES or kw.get('vocab', 100) != 2 ** 19
    assert L.lds_bytes(2 ** 19, 8, no_repeat_ngram_size=3) <= L.MAX_LDS_BYTES
    text = h.bp_strerror(-10).decode()
    assert 'top_p' in text and 'repetition_penalty' in text and 'suppress_ids' in text and 'frequency' in text
    # the binding refuses host tensors
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.pick_token(torch.zeros(2, 8), no_repeat_ngram_size=2, sequences=torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.pick_token(torch.zeros(2, 8), suppress_tokens=torch.zeros(2, dtype=torch.int32))


# ---- the code object -----------------------------------------------------------------------------------------------------------------

def test_limited_pick_kernels_use_no_scratch_spill_nothing_and_fit_the_lds_of_a_cu():
    import importlib.util
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_resources as KR
    if not KR.tools_available():
        pytest.skip('LLVM tools not found under /opt/rocm')
    spec = importlib.util.spec_from_file_location('bp_build_hip', os.path.join(ROOT, 'backpacks-flash-attn_amd', 'build_hip.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()   # no-op when the objects are current
    ks = KR.kernels([os.path.join(KR.BUILD, 'pick_token_lim.o')])
    assert {k['name'].replace(' ', '') for k in ks} == {'pick_token_kernel<Limited<BF16>>', 'pick_token_kernel<Limited<F16>>',
                                                        'pick_token_kernel<Limited<float>>'}
    for k in ks:
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
        assert k['group_segment_fixed_size'] == L.STATIC_LDS and k['max_flat_workgroup_size'] == 1024, k
        assert k['vgpr_count'] <= 128, k                      # 16 waves a workgroup: four per SIMD, 512 / 4 registers each
    # everything on at GPT-2 size and 1024 columns: 68 112 + 2 x 6 288 + 8 192 bytes
    assert L.lds_bytes(50264, 1024, 1.2, 3, 0.5, 0.5, 16) == 88880
