"""CPU: beam search -- _eager_beam_pick against the numpy restatement of tests/beam_ref.py, the slot rule on hand-made
cases, beam_search on the nano model (scores recomputed by a full forward, W = 1 against greedy, EOS stopping), the
refusals, and the argument checks of bp_beam_pick / bp_beam_copy_rows (no launch, no GPU).

On CPU tensors the Backpack's prefill always takes the content form (the table form needs the cached sense table, which
the model only builds on the GPU), so the model tests here run the content form; test_gpu_beam_search.py runs both."""
import ctypes

import numpy as np
import pytest
import torch

import beam_ref as R
import bp_hip
from decode_support import _nano_backpack
from src.utils.generation import _eager_beam_copy_rows, _eager_beam_pick, beam_search

INF = float('inf')
PROMPT = 5


def _eager(x, s, fin, W, eos=None, pad=None):
    out = _eager_beam_pick(torch.tensor(x), torch.tensor(s), None if fin is None else torch.tensor(fin), W, eos, pad)
    return [None if t is None else t.numpy() for t in out]


def _assert_self_parent(parent):
    parent = np.asarray(parent)
    assert (parent[parent] == parent).all(), parent


_compare = R.check


@pytest.mark.parametrize('vocab', [8, 64, 257])
@pytest.mark.parametrize('W', [1, 2, 3, 8])
def test_eager_beam_pick_matches_the_reference(vocab, W):
    groups = 24
    x, s, fin = R.draw(groups, W, vocab, seed=100 * vocab + W, finished_share=0.25)
    s[W:2 * W] = -INF                                                   # the -inf start in one group
    s[W] = 0.0
    fin[W:2 * W] = 0
    x[2 * W] = np.nan                                                   # degenerate rows: all their candidates at -inf
    x[3 * W, 0] = INF
    x[4 * W] = -INF
    eos, pad = 3, 1
    ref = R.beam_pick(x, s, fin, W, eos=eos, pad=pad)
    undecided = _compare(_eager(x, s, fin, W, eos, pad), ref, W, vocab)
    assert undecided <= R.UNDECIDED_CAP * groups, undecided
    # without flags: every row live, no flags returned
    ref = R.beam_pick(x, s, None, W)
    got = _eager(x, s, None, W)
    assert got[3] is None
    _compare(got, ref, W, vocab, check_finished=False)


_group = R.logprob_group


def test_slot_rule_on_hand_made_cases():
    W, V = 3, 16
    zero = np.zeros(W, dtype=np.float32)
    # a swap that must not happen: beam 2's best beats beam 0's best; both keep their slots
    x = _group(W, V, {(2, 5): -0.1, (0, 4): -0.7, (1, 9): -1.3})
    parent, tokens, scores, _ = _eager(x, zero, None, W)
    assert parent.tolist() == [0, 1, 2] and tokens.tolist() == [4, 9, 5]
    # fan-out from one parent: the best continuation keeps slot 1, the others fill the free slots 0 and 2 in rank order
    x = _group(W, V, {(1, 3): -0.9, (1, 7): -1.4, (1, 2): -2.0})
    parent, tokens, scores, _ = _eager(x, np.array([-9.0, 0.0, -9.0], dtype=np.float32), None, W)
    assert parent.tolist() == [1, 1, 1] and tokens.tolist() == [7, 3, 2]
    _assert_self_parent(parent)
    ref = R.beam_pick(x, np.array([-9.0, 0.0, -9.0]), None, W)
    assert ref['parent'].tolist() == [1, 1, 1] and ref['tokens'].tolist() == [7, 3, 2]
    # two survivors and one fork: ranks (2, a) (0, b) (2, c): slots 2 and 0 are kept, (2, c) takes the free slot 1
    x = _group(W, V, {(2, 1): -0.2, (0, 6): -0.6, (2, 8): -1.9})
    parent, tokens, _, _ = _eager(x, np.array([0.0, -30.0, 0.0], dtype=np.float32), None, W)
    assert parent.tolist() == [0, 2, 2] and tokens.tolist() == [6, 8, 1]
    _assert_self_parent(parent)
    # all rows finished: every hypothesis is frozen where it is, with the pad and its score
    s = np.array([-3.0, -1.0, -2.0], dtype=np.float32)
    parent, tokens, scores, fin = _eager(x, s, np.ones(W, dtype=np.int32), W, 2, 11)
    assert parent.tolist() == [0, 1, 2] and tokens.tolist() == [11, 11, 11] and fin.tolist() == [1, 1, 1]
    assert scores.tolist() == s.tolist()
    # a pick of the EOS sets the flag of its SLOT: beam 1 forks, its EOS continuation lands in slot 0
    x = _group(W, V, {(1, 3): -0.5, (1, 2): -1.0, (2, 4): -1.2})
    parent, tokens, _, fin = _eager(x, np.array([-30.0, 0.0, 0.0], dtype=np.float32), np.zeros(W, dtype=np.int32), W, 2, 0)
    assert parent.tolist() == [1, 1, 2] and tokens.tolist() == [2, 3, 4] and fin.tolist() == [1, 0, 0]
    # all logits and scores equal: winners (0, 0 .. W - 1)
    parent, tokens, _, _ = _eager(np.zeros((W, V), dtype=np.float32), zero, None, W)
    assert parent.tolist() == [0, 0, 0] and sorted(tokens.tolist()) == [0, 1, 2] and tokens[0] == 0


@pytest.mark.parametrize('dtype', [None, torch.float16, torch.bfloat16])
def test_the_draw_leaves_few_groups_undecided(dtype):
    """The condition of test_gpu_beam_pick.py, on the reference alone: at most 5 % of the drawn groups are undecided."""
    for vocab in R.DRAWN_VOCABS:
        for W in (1, 2, 3, 8):
            groups = 40
            x, s, fin = R.draw(groups, W, vocab, seed=10 * vocab + W, dtype=dtype, finished_share=0.2)
            ref = R.beam_pick(x, s, fin, W, eos=1, pad=0)
            undecided = sum(not R.decided(r, vocab) for r in ref['ranking'])
            assert undecided <= R.UNDECIDED_CAP * groups, (vocab, W, undecided)


def test_eager_copy_rows_matches_the_reference():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1000, size=(6, 9, 2, 3)).astype(np.int64)
    b = rng.standard_normal((6, 9)).astype(np.float32)
    parent = np.array([0, 0, 2, 2, 2, 5], dtype=np.int32)
    lengths = np.array([9, 7, 4, 3, 12, 0], dtype=np.int32)
    want = R.copy_rows([a, b], parent, lengths, 3)
    ta, tb = torch.tensor(a), torch.tensor(b)
    _eager_beam_copy_rows([ta, tb], torch.tensor(parent), torch.tensor(lengths), 3)
    assert (ta.numpy() == want[0]).all() and (tb.numpy() == want[1]).all()
    assert not (want[0] == a).all()


# ---- beam_search on the nano model -----------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def nano():
    return _nano_backpack()


def _prompts(batch, seed=0):
    return torch.randint(0, 200, (batch, PROMPT), generator=torch.Generator().manual_seed(seed))


def _sum_logprobs(model, row, length):
    """Sum of log-probabilities of row[PROMPT:length] by one full fp32 forward without a cache."""
    with torch.no_grad():
        logp = torch.log_softmax(model(row[None, :length]).logits[0].double(), dim=-1)
    at = torch.arange(PROMPT - 1, length - 1)
    return logp[at, row[PROMPT:length]].sum().item()


def _search_with_caches(model, *args, **kw):
    seen = []
    handle = model.register_forward_pre_hook(lambda mod, a, k: seen.append(k.get('inference_params')), with_kwargs=True)
    try:
        out = beam_search(*args, **kw)
    finally:
        handle.remove()
    return out, seen[0]


@pytest.mark.parametrize('W', [1, 3, 8])
def test_beam_scores_are_the_log_probabilities_of_the_returned_tokens(nano, W):
    ids = _prompts(2, seed=W)
    out, ip = _search_with_caches(nano, ids, nano, 14, W)
    assert out.beam_sequences.shape == (2, W, 13) and out.beam_scores.dtype == torch.float32
    assert (out.beam_sequences[:, :, :PROMPT] == ids[:, None]).all()
    for b in range(2):
        for w in range(W):
            want = _sum_logprobs(nano, out.beam_sequences[b, w], 13)
            assert abs(out.beam_scores[b, w].item() - want) <= 1e-4 * abs(want), (b, w, out.beam_scores[b, w].item(), want)
        best = int(out.beam_scores[b].argmax())
        assert torch.equal(out.sequences[b], out.beam_sequences[b, best]) and out.scores[b] == out.beam_scores[b, best]
        if W > 1:
            assert len({tuple(r.tolist()) for r in out.beam_sequences[b]}) == W       # distinct hypotheses
    assert (out.beam_lengths == 13).all() and (out.lengths == 13).all()
    # content form: the row index stays a pointer into the row's own content
    caches = ip.key_value_memory_dict
    assert 'backpack_content' in caches
    rows = caches['backpack_rows']
    want = torch.arange(2 * W)[:, None] * ip.max_sequence_len + torch.arange(ip.max_sequence_len)[None, :]
    assert torch.equal(rows[:, :12].long(), want[:, :12])
    assert torch.equal(nano.beam_search(ids, 14, W), out.sequences)
    again = nano.beam_search(ids, 14, W, return_dict_in_generate=True)
    assert torch.equal(again.beam_scores, out.beam_scores) and torch.equal(again.beam_sequences, out.beam_sequences)


def test_one_beam_is_greedy_decoding(nano):
    ids = _prompts(3, seed=7)
    want = nano.generate(ids, 16, kv_cache=True, device_pick=True)
    out = beam_search(ids, nano, 16, 1)
    assert torch.equal(out.sequences, want) and out.sequences.dtype == ids.dtype
    assert beam_search(ids, nano, PROMPT, 2).sequences.shape == (3, PROMPT)      # nothing to generate


def test_length_penalty_acts_on_the_final_ranking_only(nano):
    ids = _prompts(1, seed=3)
    plain = beam_search(ids, nano, 14, 4)
    eos = int(plain.beam_sequences[0, 1, PROMPT + 2])
    a = beam_search(ids, nano, 14, 4, eos_token_id=eos)
    b = beam_search(ids, nano, 14, 4, eos_token_id=eos, length_penalty=1.0)
    assert torch.equal(a.beam_sequences, b.beam_sequences) and torch.equal(a.beam_scores, b.beam_scores)
    ranked = b.beam_scores / b.beam_lengths.float()
    assert torch.equal(b.sequences[0], b.beam_sequences[0, int(ranked[0].argmax())])


def test_eos_ends_the_rows_whatever_the_polling_interval(nano):
    ids = _prompts(1, seed=11)
    greedy = beam_search(ids, nano, 20, 1).sequences
    eos = int(greedy[0, PROMPT + 3])                                   # greedy emits it: with one beam the row must end
    first = int((greedy[0, PROMPT:] == eos).nonzero()[0]) + PROMPT
    outs = [beam_search(ids, nano, 20, 1, eos_token_id=eos, pad_token_id=9, stop_check_every=n) for n in (1, 3, 1000)]
    for out in outs:
        assert out.lengths.tolist() == [first + 1] and out.sequences.shape == (1, first + 1)
        assert torch.equal(out.sequences[0], greedy[0, :first + 1])
        assert torch.equal(out.beam_scores, outs[0].beam_scores)
    # several beams: the hypotheses up to the first EOS are those of the run without one; rows end at their EOS, the pad
    # fills what is behind it, and the polling interval changes nothing
    ids = _prompts(2, seed=12)
    plain = beam_search(ids, nano, 16, 3)
    eos = int(plain.sequences[0, PROMPT + 2])
    outs = [beam_search(ids, nano, 16, 3, eos_token_id=eos, pad_token_id=9, stop_check_every=n) for n in (1, 3, 1000)]
    assert (outs[0].beam_lengths < 15).any()
    for out in outs:
        assert torch.equal(out.beam_sequences, outs[0].beam_sequences) and torch.equal(out.beam_scores, outs[0].beam_scores)
        assert torch.equal(out.beam_lengths, outs[0].beam_lengths)
        cols = out.beam_sequences.shape[2]
        for b in range(2):
            for w in range(3):
                row, n = out.beam_sequences[b, w], int(out.beam_lengths[b, w])
                assert (row[PROMPT:n - 1] != eos).all() and (row[n:] == 9).all()
                assert row[n - 1] == eos or n == cols
                want = _sum_logprobs(nano, row, n)
                assert abs(out.beam_scores[b, w].item() - want) <= 1e-4 * abs(want)


def test_refusals(nano):
    ids = _prompts(1)
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match='num_beams'):
            beam_search(ids, nano, 10, bad)
    for option in ({'temperature': 0.7}, {'top_k': 5}, {'top_p': 0.9}, {'repetition_penalty': 1.2}, {'rng_state': None}):
        with pytest.raises(ValueError, match='sampling or penalty'):
            beam_search(ids, nano, 10, 2, **option)
        with pytest.raises(ValueError, match='sampling or penalty'):
            nano.beam_search(ids, 10, 2, **option)
    from types import SimpleNamespace
    with pytest.raises(ValueError, match='vocabulary'):
        beam_search(ids % 6, SimpleNamespace(config=SimpleNamespace(vocab_size=6)), 10, 8)
    with pytest.raises(ValueError, match='stop_check_every'):
        beam_search(ids, nano, 10, 2, eos_token_id=1, stop_check_every=0)
    from src.models.intervened_models import WeightedBackpackLMHeadModel, _Intervened
    assert WeightedBackpackLMHeadModel.beam_search is _Intervened.beam_search
    with pytest.raises(NotImplementedError, match='intervened'):
        _Intervened.beam_search(object(), ids, 10, 2)
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.beam_pick(torch.zeros(2, 8), torch.zeros(2), torch.zeros(2, dtype=torch.int32), 2)
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.beam_copy_rows([torch.zeros(2, 8)], torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 0)


# ---- argument checks of the two C entries: the stated codes, before any launch ----------------------------------------------------------

def test_beam_pick_argument_validation_returns_before_any_launch():
    h = bp_hip.lib()
    p, odd, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002), None
    assert h.bp_beam_pick_ws_floats(3, 4) == 3 * 4 * 16 and h.bp_beam_pick_ws_floats(0, 4) == 0

    def call(logits=p, scores=p, finished=p, parent=p, tokens=p, sequences=p, counters=p, ws=p, ws_floats=1 << 20, groups=2,
             W=4, vocab=64, row_stride=64, tokens_stride=1, seq_stride=16, seq_cols=16, eos=3, pad=0, dtype=1):
        return h.bp_beam_pick(logits, scores, finished, parent, tokens, sequences, counters, ws, ws_floats, groups, W, vocab,
                              row_stride, tokens_stride, seq_stride, seq_cols, eos, pad, dtype, null)
    assert call(dtype=3) == -1
    for bad in (dict(groups=0), dict(W=0), dict(W=9), dict(vocab=3), dict(vocab=(1 << 23) + 1, row_stride=1 << 24),
                dict(row_stride=63), dict(tokens_stride=0), dict(seq_cols=0), dict(seq_stride=15),
                dict(logits=null), dict(scores=null), dict(parent=null), dict(tokens=null), dict(ws=null),
                dict(logits=ctypes.c_void_p(0x1001)), dict(scores=odd), dict(finished=odd), dict(parent=odd),
                dict(tokens=ctypes.c_void_p(0x1004)), dict(sequences=ctypes.c_void_p(0x1004)), dict(counters=odd),
                dict(ws=ctypes.c_void_p(0x1004)), dict(eos=64), dict(pad=-1), dict(pad=64)):
        assert call(**bad) == -3, bad
    assert call(logits=odd, dtype=2) == -3                                          # fp32 logits need 4-byte alignment
    assert call(finished=null, eos=3) == -10
    assert call(ws_floats=2 * 4 * 16 - 1) == -9
    # a NULL finished is fine without an EOS id (then the pad is not looked at): the checks pass and stop at the workspace
    assert call(finished=null, eos=-1, pad=-5, ws_floats=0) == -9


def test_beam_copy_rows_argument_validation_returns_before_any_launch():
    h = bp_hip.lib()
    p, null = ctypes.c_void_p(0x1000), None

    def call(bases=(0x1000, 0x2000), strides=(64, 4096), pos=(4, 256), n=None, parent=p, lengths=p, rows=4, first=2,
             max_positions=16):
        n = len(bases) if n is None else n
        return h.bp_beam_copy_rows((ctypes.c_void_p * len(bases))(*bases), (ctypes.c_int64 * len(strides))(*strides),
                                   (ctypes.c_int64 * len(pos))(*pos), n, parent, lengths, rows, first, max_positions, null)
    for bad in (dict(n=0), dict(bases=(0x1000,) * 33, strides=(64,) * 33, pos=(4,) * 33), dict(rows=0), dict(rows=65536),
                dict(parent=null), dict(lengths=null), dict(parent=ctypes.c_void_p(0x1002)), dict(first=-1),
                dict(max_positions=-1), dict(bases=(0x1000, 0x2008)), dict(bases=(0x1000, 0)), dict(strides=(64, 4100)),
                dict(pos=(4, 258)), dict(pos=(0, 256)), dict(strides=(48, 4096))):
        assert call(**bad) == -3, bad
    assert h.bp_beam_copy_rows(null, null, null, 1, p, p, 4, 0, 16, null) == -3
