"""CPU: generation from right-padded prompts of different lengths (prompt_lengths) on the nano fp32 model -- the contract of
what comes back, every row against itself generated alone, the per-row begins of the counted penalties and of
min_new_tokens against the numpy restatement of tests/pick_lim_ref.py, the argument checks, the intervened wrappers, and
the argument checks and kernel resources of bp_pick_token_lim_rows (no launch, no GPU)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import bp_hip
import pick_lim_ref as L
import pick_ref as R
import ragged_support as G
from decode_support import _nano_backpack as _backpack
from ragged_support import BATCH, LENGTHS, MAX_LENGTH, N, S
from src.utils.generation import PickOptions, _eager_pick, _Picker

VOCAB = 200
SEED = 1                       # of the prompts: chosen so that no greedy pick of the alone runs is a near tie (asserted)
WIDTH = S + N


def _state(seed=1234, offset=77):
    return torch.tensor([seed, offset], dtype=torch.int64)


@pytest.fixture(scope='module')
def nano():
    model = _backpack()
    ids = torch.randint(0, VOCAB, (BATCH, S), generator=torch.Generator().manual_seed(SEED))
    free = model.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, return_dict_in_generate=True)
    return model, ids, free


def _rows_end_at(out, ids, pad):
    """The layout of the contract: the prompt, N tokens, the pad."""
    for b, begin in enumerate(LENGTHS):
        assert torch.equal(out.sequences[b, :begin], ids[b, :begin])
        assert (out.sequences[b, int(out.lengths[b]):] == pad).all()


# ---- what comes back --------------------------------------------------------------------------------------------------------------

def test_layout_lengths_and_scores(nano):
    model, ids, free = nano
    assert free.sequences.shape == (BATCH, WIDTH) and free.sequences.dtype == ids.dtype
    assert free.lengths.dtype == torch.int64 and free.lengths.tolist() == [b + N for b in LENGTHS]
    _rows_end_at(free, ids, 0)
    out = model.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=torch.tensor(LENGTHS), return_dict_in_generate=True,
                         output_scores=True)
    assert torch.equal(out.sequences, free.sequences)
    with torch.no_grad():
        for b, begin in enumerate(LENGTHS):       # the prefill logits of the row's own last position
            want = model(ids[b:b + 1, :begin]).logits[0, -1]
            assert (out.scores[0][b] - want).abs().max() <= 1e-4 * want.abs().max()
    # nothing to generate: no pick lands inside a shorter row
    short = model.generate(ids, S + 1, kv_cache=True, prompt_lengths=LENGTHS, return_dict_in_generate=True)
    assert torch.equal(short.sequences, G.padded(ids, LENGTHS, 0)) and short.lengths.tolist() == list(LENGTHS)
    one = model.generate(ids, S + 2, kv_cache=True, prompt_lengths=LENGTHS, return_dict_in_generate=True)
    assert torch.equal(one.sequences, free.sequences[:, :S + 1].where(
        torch.arange(S + 1)[None, :] <= torch.tensor(LENGTHS)[:, None], torch.zeros((), dtype=ids.dtype)))


@pytest.mark.parametrize('eos', [None, 'drawn'])
def test_uniform_lengths_are_the_call_without_the_argument(nano, eos):
    model, ids, free = nano
    full = [S] * BATCH
    kw = {}
    if eos is not None:      # an id the third row generates half way: rows end at different places
        plain = model.generate(ids, MAX_LENGTH, kv_cache=True)
        kw = dict(eos_token_id=int(plain[2, S + N // 2]), pad_token_id=3)
    for call, more in ((model.generate, {}), (model.sample, dict(rng_state=_state(), top_k=20))):
        want = call(ids, MAX_LENGTH, kv_cache=True, return_dict_in_generate=True, **more, **kw)
        got = call(ids, MAX_LENGTH, kv_cache=True, return_dict_in_generate=True, prompt_lengths=full, **more, **kw)
        assert torch.equal(got.sequences, want.sequences)
        if eos is not None:
            assert torch.equal(got.lengths, want.lengths) and int(got.lengths.min()) < WIDTH
        else:
            assert got.lengths.tolist() == [WIDTH] * BATCH
    want = model.beam_search(ids[:2], MAX_LENGTH, 3, return_dict_in_generate=True, **kw)
    got = model.beam_search(ids[:2], MAX_LENGTH, 3, return_dict_in_generate=True, prompt_lengths=[S, S], **kw)
    for name in ('sequences', 'scores', 'lengths', 'beam_sequences', 'beam_scores', 'beam_lengths'):
        assert torch.equal(getattr(got, name), getattr(want, name)), name


def test_greedy_rows_equal_the_rows_generated_alone(nano):
    model, ids, free = nano
    for b, begin in enumerate(LENGTHS):
        alone = model.generate(ids[b:b + 1, :begin], begin + N + 1, kv_cache=True, device_pick=True)
        assert alone.shape == (1, begin + N)
        # a condition on the reference run: no pick of it is a near tie, so the equality below cannot hang on one
        logits, _ = G.loop_logits(model, ids[b:b + 1, :begin], [begin], alone, N)
        top2 = torch.topk(logits[:, 0], 2, dim=-1).values
        margin = float((top2[:, 0] - top2[:, 1]).min())
        print(f'row {b}: smallest top-2 margin of the alone run {margin:.3e}')
        assert margin > 1e-4, (b, margin)
        assert torch.equal(free.sequences[b, :begin + N], alone[0]), b


def test_sampled_rows_equal_their_rows_in_uniform_batches(nano):
    model, ids, _ = nano
    kw = dict(kv_cache=True, rng_state=_state(), temperature=0.9, top_k=30)
    got = model.sample(ids, MAX_LENGTH, prompt_lengths=LENGTHS, **kw)
    for begin in sorted(set(LENGTHS)):
        # every row of this length keeps its place (the Philox key holds the row index), the others are fillers of that length
        uniform = torch.stack([ids[b, :begin] if LENGTHS[b] == begin else ids[(b + 1) % BATCH, S - begin:]
                               for b in range(BATCH)])
        want = model.sample(uniform, begin + N + 1, **kw)
        for b in range(BATCH):
            if LENGTHS[b] == begin:
                assert torch.equal(got[b, :begin + N], want[b]), (begin, b)


def test_pad_columns_and_pad_id_do_not_matter(nano):
    model, ids, free = nano
    dirty = ids.clone()
    for b, begin in enumerate(LENGTHS):
        dirty[b, begin:] = torch.randint(0, VOCAB, (S - begin,), generator=torch.Generator().manual_seed(b))
    assert not torch.equal(dirty, ids)
    assert torch.equal(model.generate(dirty, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS), free.sequences)
    kw = dict(kv_cache=True, rng_state=_state(), top_p=0.9, prompt_lengths=LENGTHS)
    assert torch.equal(model.sample(dirty, MAX_LENGTH, **kw), model.sample(ids, MAX_LENGTH, **kw))
    a, b = (model.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, pad_token_id=p) for p in (3, 7))
    for r, begin in enumerate(LENGTHS):
        assert torch.equal(a[r, :begin + N], b[r, :begin + N]) and torch.equal(a[r, :begin + N], free.sequences[r, :begin + N])
        assert (a[r, begin + N:] == 3).all() and (b[r, begin + N:] == 7).all()


def test_rows_end_independently_at_their_eos(nano):
    model, ids, free = nano
    seq = free.sequences
    # an id that ends the second row early, and whichever other rows hold it behind their prompts
    eos = int(seq[1, LENGTHS[1] + 4])
    want = G.ends(seq, LENGTHS, N, eos)
    assert want[1] <= LENGTHS[1] + 5 and len(set(want)) > 1 and max(want) >= S
    for every in (None, 1, 5):
        out = model.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, eos_token_id=eos, pad_token_id=9,
                             stop_check_every=every, return_dict_in_generate=True)
        assert out.lengths.tolist() == want
        assert out.sequences.shape == (BATCH, max(want))
        for b in range(BATCH):
            assert torch.equal(out.sequences[b, :want[b]], seq[b, :want[b]])
            assert (out.sequences[b, want[b]:] == 9).all()
    # an EOS id inside a prompt, or in what the caller left behind a prompt, ends nothing
    inside = int(ids[3, 2])
    dirty = ids.clone()
    dirty[0, 1:] = inside
    out = model.generate(dirty, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, eos_token_id=inside,
                         return_dict_in_generate=True)
    assert out.lengths.tolist() == G.ends(out.sequences, LENGTHS, N, inside) and int(out.lengths[3]) > S


# ---- the per-row values of the pick ---------------------------------------------------------------------------------------------

def test_eager_pick_takes_the_begin_and_the_minimum_of_every_row():
    rng = np.random.default_rng(3)
    batch, vocab, cols = 6, 40, 12
    x = (2.0 * rng.standard_normal((batch, vocab))).astype(np.float32)
    seq = rng.integers(0, 6, size=(batch, cols)).astype(np.int64)
    counters = np.array([12, 12, 7, 3, 12, 0], dtype=np.int32)
    begins = np.array([0, 5, 7, 9, -4, 2], dtype=np.int32)          # at 0, mid-history, == Lh, > Lh, negative
    mins = np.array([13, 12, 8, 0, -1, 1], dtype=np.int32)           # c = m - 1, m, m - 1, beyond, negative, below
    for kw in (dict(), dict(do_sample=True, temperature=0.8, top_k=5), dict(do_sample=True, top_p=0.8, repetition_penalty=1.3)):
        got = _eager_pick(torch.tensor(x), rng_state=_state(), counters=torch.tensor(counters), sequences=torch.tensor(seq),
                          frequency_penalty=0.5, presence_penalty=0.25, penalty_begin=torch.tensor(begins), eos_token_id=4,
                          min_length=torch.tensor(mins), **kw).tolist()
        for b in range(batch):
            token, z, keep, u, _ = L.pick(x[b], seed=1234, offset=77, row=b, counter=int(counters[b]), seq_row=seq[b],
                                          frequency_penalty=0.5, presence_penalty=0.25, penalty_begin=max(int(begins[b]), 0),
                                          eos_token_id=4, min_length=max(int(mins[b]), 0), **kw)
            if keep is None:
                assert got[b] == token, (b, kw)
            else:
                R.assert_draw(got[b], z, keep, u, 1e-9, what=(b, kw))
    # by hand, a short row (prompt 2) next to a long one (prompt 6) with one history: id 7 occurs only in the short row's
    # prompt -- a member for the repetition penalty, not counted; id 8 was generated by the short row at column 3, inside what
    # is prompt for the long one -- counted for the short row only
    y = np.full((2, 10), 3.0, dtype=np.float32)
    hand = np.array([[7, 1, 2, 8, 2, 2, 0, 0]] * 2, dtype=np.int64)
    z = [L.values(y[b], None, hand[b], 6, 10, repetition_penalty=2.0, frequency_penalty=0.5, presence_penalty=0.25,
                  penalty_begin=begin) for b, begin in enumerate((2, 6))]
    assert z[0][7] == 1.5 and z[0][8] == 1.5 - 0.75 and z[0][2] == 1.5 - 1.75 and z[0][1] == 1.5
    assert z[1][7] == 1.5 and z[1][8] == 1.5 and z[1][2] == 1.5
    for sign, want in ((1.0, [0, 0]), (-1.0, [2, 0])):     # rewarding repetition: the short row takes its most frequent id
        got = _eager_pick(torch.tensor(y), counters=torch.tensor([6, 6], dtype=torch.int32), sequences=torch.tensor(hand),
                          repetition_penalty=2.0, frequency_penalty=sign * 0.5, presence_penalty=sign * 0.25,
                          penalty_begin=torch.tensor([2, 6], dtype=torch.int32))
        assert got.tolist() == want, sign


def _teacher_forced(model, out, begins, ends=None, min_new_tokens=None, **limits):
    """Every greedy pick of every row against the restatement called with the row's begin, on the logits of the full forward
    over the row's unpadded sequence; a pick is compared where the two best values are further apart than the rounding of a
    384-term fp32 dot product.  Returns (the number of compared picks, the (row, column)s that disagree)."""
    checked, wrong = 0, []
    for b, begin in enumerate(LENGTHS):
        row = out[b, :begin + N if ends is None else ends[b]]
        with torch.no_grad():
            logits = model(row[None]).logits[0].float().numpy()
        if min_new_tokens is not None:
            limits['min_length'] = begins[b] + min_new_tokens
        for t in range(begin, len(row)):
            v = L.values(logits[t - 1], None, row.tolist(), t, VOCAB, penalty_begin=begins[b], **limits)
            top2 = np.sort(v)[-2:]
            if top2[1] - top2[0] > 384 * 2.0 ** -23 * np.abs(logits[t - 1]).max():
                checked += 1
                if int(row[t]) != int(np.argmax(v)):
                    wrong.append((b, t))
    return checked, wrong


def test_counted_penalties_begin_at_every_rows_own_prompt(nano):
    model, ids, free = nano
    for fp, pp, theta in ((0.5, 0.25, 1.0), (2.0, 0.0, 1.3), (0.0, 1.5, 1.0)):
        kw = dict(frequency_penalty=fp, presence_penalty=pp, repetition_penalty=theta)
        out = model.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, **kw)
        assert not torch.equal(out, free.sequences), 'the penalties changed nothing: a weak test'
        checked, wrong = _teacher_forced(model, out, LENGTHS, **kw)
        assert wrong == [] and checked >= BATCH * N - 4, (kw, checked, wrong)
        # one begin for all, the padded width, is another function: it misses what a short row generated in front of column S
        _, wrong = _teacher_forced(model, out, [S] * BATCH, **kw)
        assert wrong and all(LENGTHS[b] < S for b, _ in wrong), (kw, wrong)
    # the prompt is not counted: the first token of every row is the free run's
    first = model.generate(ids, S + 2, kv_cache=True, prompt_lengths=LENGTHS, frequency_penalty=100.0, presence_penalty=100.0)
    assert torch.equal(first, free.sequences[:, :S + 1].where(
        torch.arange(S + 1)[None, :] <= torch.tensor(LENGTHS)[:, None], torch.zeros((), dtype=ids.dtype)))


def test_min_new_tokens_masks_the_eos_for_exactly_that_many_picks(nano):
    model, ids, free = nano
    # the pick itself, on logits whose maximum is always the EOS id: row b yields it from its pick number m on, not before
    eos, m = 11, 3
    x = torch.zeros((BATCH, 50))
    x[:, eos] = 5.0
    x[:, 20] = 1.0
    at = torch.tensor(LENGTHS, dtype=torch.int32)
    picker = _Picker(PickOptions(eos_token_id=eos, min_new_tokens=m, penalty_begin=S), None, x.device, at)
    for i in range(m + 2):
        picker.finished = None                                   # every pick on fresh flags
        got = picker(x, at + i).tolist()
        assert got == ([20] * BATCH if i < m else [eos] * BATCH), i
    scalar = _Picker(PickOptions(eos_token_id=eos, min_new_tokens=m, penalty_begin=S), None, x.device)
    assert scalar.keywords['min_length'] == S + m
    assert scalar(x, torch.full((BATCH,), S + m - 1, dtype=torch.int32)).tolist() == [20] * BATCH
    scalar.finished = None
    assert scalar(x, torch.full((BATCH,), S + m, dtype=torch.int32)).tolist() == [eos] * BATCH
    # in the loop: an id that every row generates among its first tokens
    seq = free.sequences
    eos = int(seq[0, LENGTHS[0]])                                # the first row's first token
    plain = model.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, eos_token_id=eos, return_dict_in_generate=True)
    assert int(plain.lengths[0]) == LENGTHS[0] + 1
    for m in (1, 4):
        out = model.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, eos_token_id=eos, min_new_tokens=m,
                             return_dict_in_generate=True)
        assert out.lengths.tolist() == G.ends(out.sequences, LENGTHS, N, eos)
        for b, begin in enumerate(LENGTHS):
            assert int(out.lengths[b]) >= begin + m + 1 and eos not in out.sequences[b, begin:begin + m].tolist()
        checked, wrong = _teacher_forced(model, out.sequences, LENGTHS, ends=out.lengths.tolist(), min_new_tokens=m, eos_token_id=eos)
        assert wrong == [] and checked >= int(out.lengths.sum()) - sum(LENGTHS) - 4, (m, checked, wrong)
    # without prompt_lengths the option is the absolute minimum S + m
    a = model.generate(ids, MAX_LENGTH, kv_cache=True, eos_token_id=eos, min_new_tokens=4, return_dict_in_generate=True)
    b = model.generate(ids, MAX_LENGTH, kv_cache=True, eos_token_id=eos, min_length=S + 4, return_dict_in_generate=True)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.lengths, b.lengths)


# ---- argument checks ----------------------------------------------------------------------------------------------------------------

def test_argument_checks(nano):
    model, ids, _ = nano
    for cg in (False, True):
        with pytest.raises(ValueError, match='kv_cache'):
            model.generate(ids, MAX_LENGTH, cg=cg, prompt_lengths=LENGTHS)
        with pytest.raises(ValueError, match='kv_cache'):
            model.sample(ids, MAX_LENGTH, cg=cg, prompt_lengths=LENGTHS)
    for bad in ([0, 5, 8, 8], [1, 5, 8, 9], [-1, 5, 8, 8], [1, 5, 8], [1, 5, 8, 8, 8], [[1, 5, 8, 8]], [1.0, 5.0, 8.0, 8.0],
                torch.tensor([1, 5, 8, S + 1])):
        with pytest.raises(ValueError, match='prompt_lengths'):
            model.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=bad)
        with pytest.raises(ValueError, match='prompt_lengths'):
            model.sample(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=bad)
        with pytest.raises(ValueError, match='prompt_lengths'):
            model.beam_search(ids, MAX_LENGTH, 2, prompt_lengths=bad)
    with pytest.raises(ValueError, match='min_new_tokens'):
        model.generate(ids, MAX_LENGTH, kv_cache=True, eos_token_id=3, min_length=10, min_new_tokens=2)
    with pytest.raises(ValueError, match='min_new_tokens'):
        model.generate(ids, MAX_LENGTH, kv_cache=True, eos_token_id=3, min_new_tokens=-1)
    with pytest.raises(ValueError, match='kv_cache'):
        model.generate(ids, MAX_LENGTH, eos_token_id=3, min_new_tokens=2)


def test_intervened_wrappers(nano):
    from src.models.intervened_models import ReplacedWordLMHeadModel, WeightedBackpackLMHeadModel
    model, ids, _ = nano
    g = torch.Generator().manual_seed(11)
    k, d = model.config.num_content_vectors, model.config.n_embd
    cw = torch.rand(VOCAB, k, generator=g) * 3
    weighted = WeightedBackpackLMHeadModel(model, cw, None, 0.1, anneal=False, upweight_nearby=True).eval()
    replaced = ReplacedWordLMHeadModel(model, {int(ids[1, 2]): torch.randn(k, d, generator=g) * 0.5,
                                               int(ids[0, 5]): torch.randn(k, d, generator=g) * 0.5}).eval()
    dirty = ids.clone()
    dirty[0, 1:] = ids[0, 5]          # a replaced word behind the first row's prompt: ignored
    for wrapper in (weighted, replaced):
        want = wrapper.generate(ids, MAX_LENGTH, kv_cache=True, device_pick=True)
        assert torch.equal(wrapper.generate(ids, MAX_LENGTH, kv_cache=True, device_pick=True, prompt_lengths=[S] * BATCH), want)
        kw = dict(kv_cache=True, rng_state=_state(), top_k=10)
        assert torch.equal(wrapper.sample(ids, MAX_LENGTH, prompt_lengths=[S] * BATCH, **kw), wrapper.sample(ids, MAX_LENGTH, **kw))
        out = wrapper.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, return_dict_in_generate=True)
        assert out.sequences.shape == (BATCH, WIDTH) and out.lengths.tolist() == [b + N for b in LENGTHS]
        assert torch.equal(out.sequences[2:], want[2:])                       # the full rows are the uniform call's
        assert torch.equal(wrapper.generate(dirty, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS), out.sequences)
    annealed = WeightedBackpackLMHeadModel(model, cw, None, 0.1, anneal=True, upweight_nearby=True).eval()
    for call in (annealed.generate, annealed.sample):
        with pytest.raises(NotImplementedError, match='prompt_lengths'):
            call(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS)
    assert annealed.generate(ids, S + 3, kv_cache=True).shape == (BATCH, S + 2)       # without the argument: as before


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def test_pick_token_lim_rows_rejects_bad_arguments_before_any_launch():
    h = bp_hip.lib()
    assert h.bp_abi_version() == 11
    p, null = ctypes.c_void_p(0x1000), None
    INF, NAN = float('inf'), float('nan')

    def call(logits=p, tokens=p, sequences=p, stats=null, rng=p, counters=null, finished=p, batch=2, vocab=100, row_stride=100,
             tokens_stride=1, seq_stride=8, seq_cols=8, do_sample=1, temperature=1.0, top_k=0, top_p=1.0, theta=1.2, eos=7,
             pad=7, min_length=0, ngram=3, fp=0.5, pp=0.25, begin=2, suppress=p, n_suppress=4, begins=p, mins=p, dtype=1):
        return h.bp_pick_token_lim_rows(logits, tokens, sequences, stats, rng, counters, finished, batch, vocab, row_stride,
                                        tokens_stride, seq_stride, seq_cols, do_sample, temperature, top_k, top_p, theta, eos,
                                        pad, min_length, ngram, fp, pp, begin, suppress, n_suppress, begins, mins, dtype, null)
    # everything bp_pick_token_lim rejects, with its codes, whether the arrays are given or not
    for arrays in (dict(), dict(begins=null, mins=null), dict(begins=null), dict(mins=null)):
        assert call(dtype=3, **arrays) == -1 and call(dtype=-1, **arrays) == -1
        for kw in (dict(batch=0), dict(vocab=0), dict(vocab=2 ** 23 + 1, row_stride=2 ** 24), dict(row_stride=99),
                   dict(tokens_stride=0), dict(logits=null), dict(tokens=null),
                   dict(sequences=p, seq_cols=0, seq_stride=8), dict(sequences=p, seq_cols=8, seq_stride=7),
                   dict(logits=ctypes.c_void_p(0x1001)), dict(tokens=ctypes.c_void_p(0x1004)), dict(stats=ctypes.c_void_p(0x1002)),
                   dict(counters=ctypes.c_void_p(0x1002)), dict(rng=ctypes.c_void_p(0x1004)),
                   dict(eos=100), dict(pad=-1), dict(pad=100), dict(finished=ctypes.c_void_p(0x1002)),
                   dict(vocab=2 ** 19 + 1, row_stride=2 ** 20), dict(ngram=-1), dict(ngram=65), dict(n_suppress=-1),
                   dict(seq_cols=8192, seq_stride=8192),
                   dict(vocab=2 ** 19, row_stride=2 ** 19, fp=0.0, pp=0.0)):
            assert call(**kw, **arrays) == -3, (kw, arrays)
        for bad in (0.0, -1.0, NAN, INF):
            assert call(temperature=bad, **arrays) == -4 and call(theta=bad, **arrays) == -10, bad
        for bad in (0.0, 1.0000001, NAN):
            assert call(top_p=bad, **arrays) == -10, bad
        for bad in (NAN, INF, -INF):
            assert call(fp=bad, **arrays) == -10 and call(pp=bad, **arrays) == -10, bad
        assert call(rng=null, **arrays) == -10 and call(finished=null, **arrays) == -10
        assert call(suppress=null, **arrays) == -10 and call(suppress=ctypes.c_void_p(0x1002), **arrays) == -10
        assert call(sequences=null, seq_stride=0, seq_cols=0, theta=1.0, ngram=0, pp=0.0, **arrays) == -10
    # its own: a misaligned array; a negative scalar only where its array is NULL
    assert call(begins=ctypes.c_void_p(0x1002)) == -3 and call(mins=ctypes.c_void_p(0x1001)) == -3
    assert call(begins=null, begin=-1) == -3 and call(begins=null, mins=null, begin=-1) == -3
    assert call(mins=null, min_length=-1) == -3 and call(begins=null, mins=null, min_length=-1) == -3
    # (with the array, the scalar is not read: the call passes every check and reaches the launch, which is not tried here)
    # the binding: a tensor selects the entry, and host tensors are refused
    at = torch.zeros(2, dtype=torch.int32)
    assert bp_hip.pick_form(penalty_begin=at) == 'rows' and bp_hip.pick_form(min_length=at) == 'rows'
    assert bp_hip.pick_form(penalty_begin=at, no_repeat_ngram_size=2, eos_token_id=3) == 'rows'
    assert bp_hip.pick_form(penalty_begin=2) == 'lim' and bp_hip.pick_form(min_length=2) == 'ctl' and bp_hip.pick_form() == 'plain'
    for kw in (dict(penalty_begin=at, frequency_penalty=0.5), dict(min_length=at, eos_token_id=1)):
        with pytest.raises(RuntimeError, match='GPU'):
            bp_hip.pick_token(torch.zeros(2, 8), sequences=torch.zeros(2, 4, dtype=torch.int64), **kw)


def test_row_limited_pick_kernels_use_no_scratch_spill_nothing_and_keep_the_static_lds():
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
    ks = KR.kernels([os.path.join(KR.BUILD, 'pick_token_rows.o')])
    assert {k['name'].replace(' ', '') for k in ks} == {'pick_token_kernel<RowLimited<BF16>>', 'pick_token_kernel<RowLimited<F16>>',
                                                        'pick_token_kernel<RowLimited<float>>'}
    for k in ks:
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
        assert k['group_segment_fixed_size'] == L.STATIC_LDS and k['max_flat_workgroup_size'] == 1024, k
        assert k['vgpr_count'] <= 128, k                      # 16 waves a workgroup: four per SIMD, 512 / 4 registers each
