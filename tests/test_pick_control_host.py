"""CPU: the controlled token pick (repetition penalty, EOS below min_length, finished rows) -- _eager_pick against the numpy
restatement of tests/pick_ctl_ref.py, the generation options on the nano model (early stop, trimming, `lengths`), and the
argument checks of bp_pick_token_ctl (no launch, no GPU)."""
import ctypes

import numpy as np
import pytest
import torch

import bp_hip
import pick_ctl_ref as C
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

def _rows(batch, vocab, seed):
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((batch, vocab))).astype(np.float32)
    x[1] = np.round(x[1])                      # ties
    x[2] = -np.abs(x[2]) - 0.5                 # all negative: the penalty multiplies by theta
    x[3] = np.abs(x[3]) + 0.5                  # all positive: by 1 / theta
    return x


def _histories(batch, vocab, cols, seed):
    """(sequences (batch, cols) int64 with duplicates and ids outside the vocabulary, counters): history lengths 0, 1, 40."""
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, vocab, size=(batch, cols)).astype(np.int64)
    seq[:, 5] = seq[:, 4]                      # a duplicate
    seq[:, 7] = -1
    seq[:, 8] = vocab
    seq[:, 9] = 2 ** 40
    counters = np.array([(0, 1, 40)[b % 3] for b in range(batch)], dtype=np.int32)
    return seq, counters


def _check(x, seq, counters, finished=None, **kw):
    """_eager_pick on the rows against C.pick row by row; returns the tokens."""
    batch, vocab = x.shape
    fin = None if finished is None else torch.tensor(finished, dtype=torch.int32)
    got = _eager_pick(torch.tensor(x), kw.get('do_sample', False), kw.get('temperature', 1.0), kw.get('top_k', 0),
                      kw.get('top_p', 1.0), _state(), torch.tensor(counters), kw.get('repetition_penalty', 1.0),
                      kw.get('eos_token_id'), kw.get('pad_token_id'), kw.get('min_length', 0), fin,
                      None if seq is None else torch.tensor(seq)).tolist()
    exact = 0
    for b in range(batch):
        token, z, keep, u, _ = C.pick(x[b], seed=SEED, offset=OFFSET, row=b, counter=int(counters[b]),
                                      seq_row=None if seq is None else seq[b],
                                      finished=bool(finished[b]) if finished is not None else False, **kw)
        if keep is None:
            assert got[b] == token, (b, kw, got[b], token)
        else:
            R.assert_draw(got[b], z, keep, u, 1e-9, what=(b, kw))
        exact += got[b] == token
    assert exact >= batch - 1
    return got


@pytest.mark.parametrize('vocab', [7, 200])
@pytest.mark.parametrize('kw', [
    dict(repetition_penalty=1.3), dict(repetition_penalty=0.7), dict(repetition_penalty=1.3, do_sample=True),
    dict(repetition_penalty=2.0, do_sample=True, temperature=0.7, top_k=3), dict(repetition_penalty=1.2, do_sample=True, top_p=0.8),
    dict(repetition_penalty=1.0, do_sample=True, top_k=4), dict(repetition_penalty=1.5, eos_token_id=2, min_length=30),
    dict(repetition_penalty=1.5, eos_token_id=2, min_length=30, do_sample=True, temperature=1.3, top_k=5, top_p=0.9),
], ids=str)
def test_eager_pick_matches_the_numpy_restatement(vocab, kw):
    x = _rows(12, vocab, seed=vocab)
    x[4, 2] = x[4].max() + 3.0                 # the EOS column is the argmax of row 4
    x[5, 1] = NAN                              # degenerate rows take the (penalised) greedy answer
    x[6, :] = -INF
    seq, counters = _histories(12, vocab, 48, seed=vocab + 1)
    _check(x, seq, counters, **kw)
    _check(x, None, counters, **{**kw, 'repetition_penalty': 1.0})       # no history without sequences


def test_the_penalty_moves_the_argmax_and_only_for_members_of_the_history():
    x = np.array([[4.0, 3.9, -1.0, -1.1, 0.0]], dtype=np.float32)
    seq = np.array([[0, 0, 2, 99, -5]], dtype=np.int64)
    for counter, want in ((0, 0), (1, 1), (3, 1)):
        got = _check(x, seq, np.array([counter], dtype=np.int32), repetition_penalty=1.2)
        assert got == [want]
    # negative logits move AWAY from zero: -1.0 * 1.2 < -1.1, so among {2, 3} the unpenalised 3 wins once 2 is in the history
    y = np.array([[-1.0, -1.1]], dtype=np.float32)
    assert _check(y, np.array([[0]], dtype=np.int64), np.array([1], dtype=np.int32), repetition_penalty=1.2) == [1]
    assert _check(y, np.array([[0]], dtype=np.int64), np.array([0], dtype=np.int32), repetition_penalty=1.2) == [0]
    # theta < 1 rewards repetition
    assert _check(x, seq, np.array([1], dtype=np.int32), repetition_penalty=0.5) == [0]
    # the two roundings of the restatement, spelled out once
    t, rt = np.float32(1.3), np.float32(1.0) / np.float32(1.3)
    z = C.pen(np.array([2.5, -2.5, 0.0, 7.0], dtype=np.float32), {0, 1, 2}, 1.3)
    assert z.tolist() == [np.float32(2.5) * rt, np.float32(-2.5) * t, 0.0, 7.0]


def test_eos_is_masked_below_min_length_everywhere():
    x = _rows(8, VOCAB, seed=4)
    x[:, 17] = x.max() + 5.0                   # the EOS id dominates every row
    counters = np.array([3, 9, 10, 11, 0, 9, 10, 50], dtype=np.int32)
    for kw in (dict(), dict(do_sample=True), dict(do_sample=True, top_k=1), dict(do_sample=True, top_p=0.2)):
        got = _check(x, None, counters, eos_token_id=17, min_length=10, **kw)
        for b, c in enumerate(counters):
            if c < 10:
                assert got[b] != 17, (kw, b)
        for b in (2, 3, 6, 7):
            if kw != dict(do_sample=True):
                assert got[b] == 17, (kw, b)
    # a row whose only finite logit is the masked EOS: the greedy answer of a row of -inf
    y = np.full((1, 9), -INF, dtype=np.float32)
    y[0, 4] = 1.0
    assert _check(y, None, np.array([0], dtype=np.int32), eos_token_id=4, min_length=5, do_sample=True) == [0]
    assert _check(y, None, np.array([5], dtype=np.int32), eos_token_id=4, min_length=5, do_sample=True) == [4]


def test_finished_rows_give_the_pad_and_keep_their_flag():
    x = _rows(6, VOCAB, seed=8)
    counters = np.arange(6, dtype=np.int32)
    finished = [0, 1, 0, 7, 0, 1]
    for kw in (dict(eos_token_id=3), dict(eos_token_id=3, pad_token_id=11), dict(eos_token_id=3, pad_token_id=11, do_sample=True)):
        got = _check(x, None, counters, finished=finished, **kw)
        pad = kw.get('pad_token_id', 3)
        assert [got[b] for b in (1, 3, 5)] == [pad] * 3
    # _Picker owns the flags: set by the pick that returns the EOS id, kept afterwards
    from src.utils.generation import PickOptions, _Picker
    picker = _Picker(PickOptions(eos_token_id=5, pad_token_id=9), None, torch.device('cpu'))
    logits = torch.zeros(3, 12)
    logits[0, 5] = logits[1, 6] = logits[2, 5] = 1.0
    sequences = torch.full((3, 4), -1, dtype=torch.int64)
    first = picker(logits, torch.zeros(3, dtype=torch.int32), sequences=sequences)
    assert first.tolist() == [5, 6, 5] and picker.finished.tolist() == [1, 0, 1]
    logits[1, 6], logits[1, 5] = 0.0, 1.0
    second = picker(logits, torch.ones(3, dtype=torch.int32), sequences=sequences)
    assert second.tolist() == [9, 5, 9] and picker.finished.tolist() == [1, 1, 1]
    assert sequences[:, :2].tolist() == [[5, 9], [6, 5], [5, 9]] and (sequences[:, 2:] == -1).all()


# ---- generation on the nano model ----------------------------------------------------------------------------------------------------

NEW = 12


@pytest.fixture(scope='module')
def nano():
    model = _backpack()
    ids = torch.randint(0, VOCAB, (3, PROMPT), generator=torch.Generator().manual_seed(3))
    return model, ids


def _expected(free, eos, pad):
    """(sequences, lengths) the contract makes of a free run: every row cut behind its first EOS at a column >= PROMPT."""
    free = free.clone()
    width = free.shape[1]
    lengths = []
    for b in range(free.shape[0]):
        hits = [t for t in range(PROMPT, width) if int(free[b, t]) == eos]
        end = hits[0] + 1 if hits else width
        free[b, end:] = pad
        lengths.append(end)
    return free[:, :max(lengths)], lengths


@pytest.mark.parametrize('decode', ['generate', 'sample'])
def test_rows_stop_at_an_eos_that_provably_occurs(nano, decode):
    model, ids = nano
    n = PROMPT + NEW
    kw = dict(kv_cache=True, device_pick=True)
    if decode == 'sample':
        kw['rng_state'] = _state()                 # the draw of (b, t) is a pure function of logits, state, row and position
    run = getattr(model, decode)
    free = run(ids, n, **kw)
    assert free.shape == (3, n - 1)
    eos = int(free[0, PROMPT + 3])
    for pad in (None, 0 if eos != 0 else 1):
        want, lengths = _expected(free, eos, eos if pad is None else pad)
        assert lengths[0] <= PROMPT + 4 and want.shape[1] == max(lengths)
        outs = []
        for every in (1, 3, 1000, None):
            out = run(ids, n, eos_token_id=eos, pad_token_id=pad, stop_check_every=every, return_dict_in_generate=True, **kw)
            assert out.sequences.dtype == ids.dtype and out.lengths.dtype == torch.int64
            assert out.lengths.tolist() == lengths, (every, pad)
            assert torch.equal(out.sequences, want), (every, pad)
            outs.append(out.sequences)
        assert all(torch.equal(o, outs[0]) for o in outs)
    # without return_dict_in_generate: the sequences alone; without an EOS id: no lengths
    assert torch.equal(run(ids, n, eos_token_id=eos, **kw), _expected(free, eos, eos)[0])
    assert run(ids, n, return_dict_in_generate=True, **kw).lengths is None
    assert run(ids, n, repetition_penalty=1.1, return_dict_in_generate=True, **kw).lengths is None


def test_an_eos_that_never_occurs_changes_nothing(nano):
    model, ids = nano
    n = PROMPT + NEW
    free = model.generate(ids, n, kv_cache=True)
    unused = next(t for t in range(VOCAB) if not (free[:, PROMPT:] == t).any())
    out = model.generate(ids, n, kv_cache=True, eos_token_id=unused, stop_check_every=2, return_dict_in_generate=True)
    assert torch.equal(out.sequences, free) and out.lengths.tolist() == [n - 1] * 3


def test_min_length_keeps_the_eos_out_and_the_draw_obeys_the_masked_top_k(nano):
    model, ids = nano
    n = PROMPT + NEW
    free = model.generate(ids, n, kv_cache=True, device_pick=True)
    eos = int(free[0, PROMPT + 3])
    out = model.generate(ids, n, kv_cache=True, eos_token_id=eos, min_length=PROMPT + 8, return_dict_in_generate=True)
    assert not (out.sequences[:, PROMPT:PROMPT + 8] == eos).any()
    assert all(length >= PROMPT + 9 or length == out.sequences.shape[1] for length in out.lengths.tolist())
    seq = model.sample(ids, n, rng_state=_state(), top_k=3, temperature=0.9, kv_cache=True, eos_token_id=eos,
                       min_length=PROMPT + 8, pad_token_id=eos)
    assert not (seq[:, PROMPT:PROMPT + 8] == eos).any()
    with torch.no_grad():
        logits = model(seq).logits.float().numpy()
    ended = [False] * 3
    for t in range(PROMPT, seq.shape[1]):
        for b in range(3):
            if ended[b]:
                assert int(seq[b, t]) == eos                      # the pad
                continue
            z = C.scaled_values(logits[b, t - 1], 0.9, set(), 1.0, t, eos, PROMPT + 8)
            keep = R.kept_set(z, top_k=3)
            assert t >= PROMPT + 8 or not keep[eos]
            R.assert_draw(int(seq[b, t]), z, keep, R.uniform(SEED, OFFSET, b, t), R.epsilon(VOCAB), what=(b, t))
            ended[b] = int(seq[b, t]) == eos


def test_penalised_generation_obeys_the_contract_on_the_teacher_forced_logits(nano):
    model, ids = nano
    n = PROMPT + NEW
    theta = 1.3
    greedy = model.generate(ids, n, kv_cache=True, repetition_penalty=theta)
    drawn = model.sample(ids, n, kv_cache=True, repetition_penalty=theta, rng_state=_state(), top_k=5, temperature=0.8)
    assert greedy.shape == drawn.shape == (3, n - 1)
    assert not torch.equal(greedy, model.generate(ids, n, kv_cache=True)), 'the penalty changed nothing: a weak test'
    checked = 0
    with torch.no_grad():
        lg, ld = model(greedy).logits.float().numpy(), model(drawn).logits.float().numpy()
    for b in range(3):
        for t in range(PROMPT, n - 1):
            hist = C.history(greedy[b].tolist(), t, VOCAB)
            v = C.greedy_values(lg[b, t - 1], hist, theta, t, None, 0)
            top2 = np.sort(v)[-2:]
            # the cached step and the full forward round differently: a dot product of 384 fp32 terms per logit
            if top2[1] - top2[0] > 384 * 2.0 ** -23 * np.abs(lg[b, t - 1]).max():
                assert int(greedy[b, t]) == int(np.argmax(v)), (b, t)
                checked += 1
            hist = C.history(drawn[b].tolist(), t, VOCAB)
            z = C.scaled_values(ld[b, t - 1], 0.8, hist, theta, t, None, 0)
            R.assert_draw(int(drawn[b, t]), z, R.kept_set(z, top_k=5), R.uniform(SEED, OFFSET, b, t), R.epsilon(VOCAB), what=(b, t))
    assert checked >= 3 * (NEW - 1) - 3


def test_intervened_wrapper_takes_the_controls(nano):
    from src.models.intervened_models import WeightedBackpackLMHeadModel
    model, ids = nano
    cw = torch.rand(VOCAB, model.config.num_content_vectors, generator=torch.Generator().manual_seed(11)) * 3
    wrapper = WeightedBackpackLMHeadModel(model, cw, None, 0.1, anneal=False, upweight_nearby=True).eval()
    n = PROMPT + NEW
    free = wrapper.generate(ids, n, kv_cache=True, device_pick=True, repetition_penalty=1.2)
    eos = int(free[0, PROMPT + 3])
    out = wrapper.generate(ids, n, kv_cache=True, repetition_penalty=1.2, eos_token_id=eos, return_dict_in_generate=True)
    want, lengths = _expected(free, eos, eos)
    assert torch.equal(out.sequences, want) and out.lengths.tolist() == lengths
    s = wrapper.sample(ids, n, kv_cache=True, repetition_penalty=1.2, eos_token_id=eos, rng_state=_state(), top_k=4)
    assert s.shape[1] <= n - 1 and torch.equal(s[:, :PROMPT], ids)


def test_the_controls_need_the_kv_cache_and_sane_values(nano):
    model, ids = nano
    for kw in (dict(repetition_penalty=1.2), dict(eos_token_id=5), dict(pad_token_id=5), dict(min_length=3)):
        for cg in (False, True):
            with pytest.raises(ValueError, match='kv_cache'):
                model.generate(ids, PROMPT + 2, cg=cg, **kw)
            with pytest.raises(ValueError, match='kv_cache'):
                model.sample(ids, PROMPT + 2, cg=cg, **kw)
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError):
            model.generate(ids, PROMPT + 2, kv_cache=True, repetition_penalty=bad)
        with pytest.raises(ValueError):
            model.sample(ids, PROMPT + 2, kv_cache=True, repetition_penalty=bad)
    with pytest.raises(ValueError):
        model.generate(ids, PROMPT + 2, kv_cache=True, eos_token_id=5, stop_check_every=0)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------

def test_pick_token_ctl_rejects_bad_arguments_before_any_launch():
    h = bp_hip.lib()
    assert h.bp_abi_version() == 11
    p, null = ctypes.c_void_p(0x1000), None

    def call(logits=p, tokens=p, sequences=p, stats=null, rng=p, counters=null, finished=p, batch=2, vocab=100, row_stride=100,
             tokens_stride=1, seq_stride=8, seq_cols=8, do_sample=1, temperature=1.0, top_k=0, top_p=1.0, theta=1.2, eos=7,
             pad=7, min_length=0, dtype=1):
        return h.bp_pick_token_ctl(logits, tokens, sequences, stats, rng, counters, finished, batch, vocab, row_stride,
                                   tokens_stride, seq_stride, seq_cols, do_sample, temperature, top_k, top_p, theta, eos, pad,
                                   min_length, dtype, null)
    # everything bp_pick_token rejects, with its codes
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
    # its own: BP_ERR_SAMPLING
    for bad in (0.0, -1.0, NAN, INF, -INF):
        assert call(theta=bad) == -10, bad
        assert call(theta=bad, do_sample=0) == -10, bad
    assert call(sequences=null, seq_stride=0, seq_cols=0) == -10          # a penalty without a history to read
    assert call(finished=null) == -10                                      # an EOS id without flags
    # BP_ERR_SHAPE
    for kw in (dict(eos=100), dict(eos=2 ** 20), dict(pad=-1), dict(pad=100), dict(min_length=-1),
               dict(finished=ctypes.c_void_p(0x1002)), dict(vocab=2 ** 19 + 1, row_stride=2 ** 20),
               dict(vocab=2 ** 19 + 1, row_stride=2 ** 20, do_sample=0)):
        assert call(**kw) == -3, kw
    assert 'top_p' in h.bp_strerror(-10).decode() and 'repetition_penalty' in h.bp_strerror(-10).decode()
    # the binding refuses host tensors
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.pick_token(torch.zeros(2, 8), repetition_penalty=1.2, sequences=torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.pick_token(torch.zeros(2, 8), eos_token_id=3, finished=torch.zeros(2, dtype=torch.int32))


def test_controlled_pick_kernels_use_no_scratch_and_fit_the_lds_of_a_cu():
    import importlib.util
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_resources as KR
    if not KR.tools_available():
        pytest.skip('LLVM tools not found under /opt/rocm')
    spec = importlib.util.spec_from_file_location('bp_build_hip', os.path.join(ROOT, 'backpacks-flash-attn_amd', 'build_hip.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()   # no-op when the objects are current
    ks = KR.kernels([os.path.join(KR.BUILD, 'pick_token_ctl.o')])
    assert {k['name'].replace(' ', '') for k in ks} == {'pick_token_kernel<Controlled<BF16>>', 'pick_token_kernel<Controlled<F16>>',
                                                        'pick_token_kernel<Controlled<float>>'}
    bitmap = (2 ** 19 // 32 + 1) * 4               # dynamic LDS at the largest vocabulary a penalty takes
    for k in ks:
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, k
        assert k['group_segment_fixed_size'] + bitmap <= 160 * 1024 and k['max_flat_workgroup_size'] == 1024, k
