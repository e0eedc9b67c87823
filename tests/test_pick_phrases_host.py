"""Host: banned phrases and stop sequences of more than one token (bp_pick_token_phrases; src/utils/generation.py:
bad_words_ids, stop_sequences) -- the restatement of tests/pick_phrase_ref.py against a brute-force string search, _eager_pick
against the restatement on the contract's edges, generation on the CPU nano model against an independent scan of the free run,
the argument checks of the C ABI on fake pointers, and the resources of the new code object."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import bp_hip
import pick_lim_ref as L
import pick_phrase_ref as P
from decode_support import PROMPT
from decode_support import _nano_backpack as _backpack
from src.utils.generation import PickOptions, _eager_pick

SEED, OFFSET = 1234, 77
VOCAB = 200
NAN, INF = float('nan'), float('inf')


def _state(seed=SEED, offset=OFFSET):
    return torch.tensor([seed, offset], dtype=torch.int64)


# ---- the restatement against a string search ------------------------------------------------------------------------------------------
#
# Over an alphabet of 4 ids a history is a string of the letters a..d and a phrase a word: str.endswith / str.find know
# nothing of offsets and slices.

def _text(ids):
    return ''.join('abcd'[i] for i in ids)


def test_the_restatement_agrees_with_a_string_search():
    rng = np.random.default_rng(0)
    bans = stops = 0
    for _ in range(400):
        n = int(rng.integers(0, 14))
        h = [int(v) for v in rng.integers(0, 4, size=n)]
        phrases = [[int(v) for v in rng.integers(0, 4, size=int(rng.integers(1, 5)))] for _ in range(int(rng.integers(1, 5)))]
        want = {w[-1] for w in phrases if _text(h).endswith(_text(w[:-1]))}
        assert P.banned_by_phrases(h, phrases, 4) == want, (h, phrases)
        assert P.banned_by_phrases(h, phrases, 2) == {t for t in want if t < 2}
        bans += bool(want)
        token, begin, minimum = int(rng.integers(0, 4)), int(rng.integers(0, n + 2)), int(rng.integers(0, n + 2))
        text, reason = _text(h + [token]), None
        for j, w in enumerate(phrases):
            if n >= minimum and text.endswith(_text(w)) and len(text) - len(w) >= begin:
                reason = 1 + j
                break
        assert P.stop_match(h, token, n, begin, minimum, phrases, None) == reason, (h, token, begin, minimum, phrases)
        assert P.stop_match(h, token, n, begin, minimum, phrases, token) == 0
        assert P.stop_match(None, token, n, begin, minimum, phrases, None) is None
        stops += reason is not None
    assert bans > 100 and stops > 40, (bans, stops)


def test_ignored_phrases_of_a_packed_pair():
    ids = list(range(10, 20))
    #          fine      empty   decreasing  beyond total  negative
    offsets = [0, 3,     3,      2,          11,           -1, 4]
    assert P.unpack(ids, offsets) == [[10, 11, 12], None, None, None, None, None]
    assert P.unpack(list(range(70)), [0, 64, 70, 70 - 65]) == [list(range(64)), list(range(64, 70)), None]
    assert P.unpack(list(range(70)), [0, 65]) == [None]
    packed = P.pack([[1, 2], [3], [4, 5, 6]])
    assert packed[0].tolist() == [1, 2, 3, 4, 5, 6] and packed[1].tolist() == [0, 2, 3, 6] and packed[0].dtype == np.int32


# ---- _eager_pick against the restatement ------------------------------------------------------------------------------------------------

def test_eager_pick_bans_by_phrase_as_the_restatement_says():
    vocab, cols = 20, 12
    rng = np.random.default_rng(3)
    seq = rng.integers(0, 6, size=(8, cols)).astype(np.int64)
    seq[1, 2], seq[2, 4] = -1, vocab + 3                                 # raw values in a prefix
    counters = np.array([0, 3, 5, 1, cols, cols + 4, 2, -2], dtype=np.int32)
    x = rng.standard_normal((8, vocab)).astype(np.float32)
    phrases = [[7]]                                                      # L = 1: always
    for b in range(8):
        h = L.clamped_history(seq[b], counters[b])
        best = int(np.argmax(x[b]))
        phrases.append(h[len(h) - 1:] + [best])                          # L = 2 (L = 1 for an empty history): bans the row's argmax
        phrases.append(h[len(h) - 3:] + [int(np.argsort(x[b])[-2])])     # up to L = 4, from column 0 for the short histories
    phrases += [[3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 1],          # longer than any history
                [int(seq[0, 0]), -1], [int(seq[0, 0]), vocab], [0], [vocab - 1], [-1, 5], [vocab + 3, 6]]
    got = _eager_pick(torch.tensor(x), counters=torch.tensor(counters), sequences=torch.tensor(seq), bad_words_ids=phrases)
    decided = 0
    for b in range(8):
        want = P.step(x[b], seq[b], int(counters[b]), False, 0, 0, phrases, [])[0]
        assert int(got[b]) == want, b
        decided += want != int(np.argmax(x[b]))
    assert decided >= 6
    every = [[t] for t in range(vocab)]                                  # a row with every id banned takes index 0
    assert _eager_pick(torch.tensor(x), sequences=torch.tensor(seq), bad_words_ids=every).tolist() == [0] * 8
    drawn = _eager_pick(torch.tensor(x), do_sample=True, rng_state=_state(), sequences=torch.tensor(seq), bad_words_ids=every)
    assert drawn.tolist() == [0] * 8


def test_eager_pick_stops_as_the_restatement_says():
    vocab, cols, eos = 20, 10, 4
    cases = []   # (history, token, begin, minimum, finished on entry, counter or None for len(history))

    def case(h, token, begin=0, minimum=0, finished=0, counter=None):
        cases.append((h, token, begin, minimum, finished, len(h) if counter is None else counter))
    stops = [[1, 2, 3], [2, 3], [9], [3], [5, 5, 5, 5], [eos, 7], [6, eos]]
    case([0, 1, 2], 3)                  # two phrases end here: the lower index
    case([0, 1, 2], 3, begin=1)         # the longer one begins exactly at the row's begin
    case([0, 1, 2], 3, begin=2)         # ... one column in front of it: the shorter one
    case([0, 1, 2], 3, begin=3)         # only [3] lies behind the begin
    case([0, 1, 2], 3, begin=4)         # nothing does
    case([0, 1, 2], 3, minimum=3)       # c == m counts
    case([0, 1, 2], 3, minimum=4)       # c == m - 1 does not
    case([], 9)                         # c = 0, L = 1
    case([], 3, begin=-5, minimum=-1)   # negative values count as 0
    case([1, 2], 3, finished=1)         # finished on entry: the pad, nothing recorded
    case([6], eos)                      # the EOS id and a phrase: reason 0
    case([eos], 7)                      # a phrase that holds the EOS id
    case([5, 5, 5], 5)                  # from column 0
    case([0, 5, 5, 5], 5, begin=1)
    case([0, 5, 5, 5], 5, begin=2)
    case([1, 2, 3, 0, 0, 0, 0, 0, 0, 0], 3, counter=cols)          # no column: no phrase
    case([1, 2, 3, 0, 0, 0, 0, 0, 0, 0], eos, counter=cols + 3)    # ... but the EOS id still ends the row
    case([0, 0, 1, 2], eos, minimum=9)  # the EOS id below the minimum is masked: another token, no end
    n = len(cases)
    seq = np.zeros((n, cols), dtype=np.int64)
    x = np.zeros((n, vocab), dtype=np.float32)
    for b, (h, token, *_rest) in enumerate(cases):
        seq[b, :len(h)] = h
        x[b, token] = 5.0
    x[-1, 11] = 4.0
    counters = torch.tensor([c[5] for c in cases], dtype=torch.int32)
    begins = torch.tensor([c[2] for c in cases], dtype=torch.int32)
    mins = torch.tensor([c[3] for c in cases], dtype=torch.int32)
    finished = torch.tensor([c[4] for c in cases], dtype=torch.int32)
    ends, reasons = torch.full((n,), -9, dtype=torch.int32), torch.full((n,), -9, dtype=torch.int32)
    got = _eager_pick(torch.tensor(x), counters=counters, sequences=torch.tensor(seq), finished=finished, eos_token_id=eos,
                      pad_token_id=2, min_length=mins, penalty_begin=begins, stop_sequences=stops, ends=ends, reasons=reasons)
    want_reasons = []
    for b, (h, token, begin, minimum, fin, c) in enumerate(cases):
        tok, why = P.step(x[b], seq[b], c, bool(fin), begin, minimum, [], stops, eos=eos, pad=2)
        assert int(got[b]) == tok, b
        assert int(finished[b]) == int(bool(fin) or why is not None), b
        assert (int(ends[b]), int(reasons[b])) == ((-9, -9) if why is None else (c + 1, why)), (b, why)
        want_reasons.append(why)
    assert want_reasons == [1, 1, 2, 4, None, 1, None, 3, 4, None, 0, 6, 5, 5, None, None, 0, None]
    assert int(got[-1]) == 11 and int(got[9]) == 2


# ---- generation on the nano model ----------------------------------------------------------------------------------------------------

NEW = 40
N = PROMPT + NEW


@pytest.fixture(scope='module')
def nano():
    model = _backpack()
    ids = torch.randint(0, VOCAB, (3, PROMPT), generator=torch.Generator().manual_seed(1))
    free = model.sample(ids, N, kv_cache=True, rng_state=_state(), top_k=6)
    return model, ids, free


def _scan(row, begin, full, stops, eos=None, minimum=0):
    """(end, reason) of an untrimmed row: the first column c in [begin, full) whose token is the EOS id or ends a stop sequence
    that lies in [begin, c], looked for once c >= minimum; (full, -1) when there is none."""
    for c in range(begin, full):
        if eos is not None and row[c] == eos:
            return c + 1, 0
        for j, w in enumerate(stops):
            if c >= minimum and c + 1 - len(w) >= begin and row[c + 1 - len(w):c + 1] == w:
                return c + 1, 1 + j
    return full, -1


def _occurrences(row, begin, stops):
    """The ends of every occurrence of a stop sequence that lies in row[begin:]."""
    return sorted({c + 1 for w in stops for c in range(begin + len(w) - 1, len(row)) if row[c + 1 - len(w):c + 1] == w})


def _check_against_scan(out, free, begins, stops, pad, eos=None, minimum=None):
    rows = free.tolist()
    full = [free.shape[1]] * len(rows) if isinstance(begins, int) else [b + free.shape[1] - max(begins) for b in begins]
    begins = [begins] * len(rows) if isinstance(begins, int) else begins
    want = [_scan(r, b, f, stops, eos, b + minimum if minimum is not None else 0) for r, b, f in zip(rows, begins, full)]
    assert out.lengths.tolist() == [w[0] for w in want] and out.stop_reasons.tolist() == [w[1] for w in want]
    assert out.lengths.dtype == torch.int64 and out.stop_reasons.dtype == torch.int64
    assert out.sequences.shape == (len(rows), max(w[0] for w in want))
    for b, (end, _) in enumerate(want):
        assert out.sequences[b, :end].tolist() == rows[b][:end], b
        assert (out.sequences[b, end:] == pad).all(), b
    return want


def test_stop_sequences_end_the_rows_where_a_scan_of_the_free_run_says(nano):
    model, ids, free = nano
    assert free.shape == (3, N - 1)
    r = free.tolist()
    stops = [r[0][PROMPT + 9:PROMPT + 12], r[1][PROMPT + 20:PROMPT + 22], [r[2][PROMPT + 30]], r[1][PROMPT + 5:PROMPT + 7],
             [VOCAB - 1] * 5]
    for cg in (False, True):     # cg is accepted on CPU tensors and changes nothing
        out = model.sample(ids, N, kv_cache=True, cg=cg, rng_state=_state(), top_k=6, stop_sequences=stops, pad_token_id=3,
                           return_dict_in_generate=True)
        want = _check_against_scan(out, free, PROMPT, stops, 3)
        assert all(end < N - 1 for end, _ in want) and len({why for _, why in want}) >= 2, want
        for b, (end, why) in enumerate(want):   # the only occurrence in generated text is the one that ended the row
            assert _occurrences(out.sequences[b, :end].tolist(), PROMPT, stops) == [end], b
    polled = model.sample(ids, N, kv_cache=True, rng_state=_state(), top_k=6, stop_sequences=stops, pad_token_id=3,
                          stop_check_every=1, return_dict_in_generate=True)
    assert torch.equal(polled.sequences, out.sequences) and torch.equal(polled.lengths, out.lengths)
    # the record is trimmed by the same lengths
    rec = model.sample(ids, N, kv_cache=True, rng_state=_state(), top_k=6, stop_sequences=stops, pad_token_id=3,
                       output_logprobs=True, return_dict_in_generate=True)
    assert torch.equal(rec.sequences, out.sequences) and rec.token_ranks.shape == out.sequences.shape
    for b, (end, _) in enumerate(want):
        assert (rec.token_ranks[b, PROMPT:end] >= 0).all() and (rec.token_ranks[b, end:] == -1).all()
    # a run that never stops: the full width, reasons -1
    never = model.sample(ids, N, kv_cache=True, rng_state=_state(), top_k=6, stop_sequences=[[VOCAB - 1] * 5],
                         return_dict_in_generate=True)
    assert torch.equal(never.sequences, free) and never.lengths.tolist() == [N - 1] * 3 and never.stop_reasons.tolist() == [-1] * 3


def test_a_prompt_that_ends_with_the_phrase_stops_nothing(nano):
    model, ids, free = nano
    r = free.tolist()
    stops = [r[0][PROMPT - 2:PROMPT], r[1][PROMPT - 1:PROMPT + 1], [r[2][PROMPT - 1]]]     # in the prompt, across its end, its last id
    out = model.sample(ids, N, kv_cache=True, rng_state=_state(), top_k=6, stop_sequences=stops, return_dict_in_generate=True)
    _check_against_scan(out, free, PROMPT, stops, 0)
    assert out.lengths[1] > PROMPT + 1


def test_eos_and_stop_sequences_together_and_eos_alone_as_before(nano):
    model, ids, free = nano
    r = free.tolist()
    eos = r[0][PROMPT + 6]
    alone = model.sample(ids, N, kv_cache=True, rng_state=_state(), top_k=6, eos_token_id=eos, return_dict_in_generate=True)
    assert alone.stop_reasons is None
    want = [_scan(row, PROMPT, N - 1, [], eos) for row in r]
    assert alone.lengths.tolist() == [w[0] for w in want] and alone.sequences.shape[1] == max(w[0] for w in want)
    for b, (end, _) in enumerate(want):
        assert alone.sequences[b, :end].tolist() == r[b][:end] and (alone.sequences[b, end:] == eos).all()
    both = model.sample(ids, N, kv_cache=True, rng_state=_state(), top_k=6, eos_token_id=eos, stop_sequences=[[VOCAB - 1] * 5],
                        return_dict_in_generate=True)
    assert torch.equal(both.sequences, alone.sequences) and torch.equal(both.lengths, alone.lengths)
    assert both.stop_reasons.tolist() == [w[1] for w in want] and 0 in both.stop_reasons.tolist()
    stops = [r[1][PROMPT + 2:PROMPT + 4], [eos]]
    mixed = model.sample(ids, N, kv_cache=True, rng_state=_state(), top_k=6, eos_token_id=eos, stop_sequences=stops,
                         return_dict_in_generate=True)
    got = _check_against_scan(mixed, free, PROMPT, stops, eos, eos=eos)
    assert got[0][1] == 0                                           # the EOS id wins over the phrase that holds it


def test_min_new_tokens_delays_a_stop_as_it_delays_the_eos(nano):
    model, ids, free = nano
    r = free.tolist()
    stops = [[r[0][PROMPT + 2]], [r[1][PROMPT + 1]], r[2][PROMPT + 3:PROMPT + 5]]
    early = model.sample(ids, N, kv_cache=True, rng_state=_state(), top_k=6, stop_sequences=stops, return_dict_in_generate=True)
    first = _check_against_scan(early, free, PROMPT, stops, 0)
    assert [e for e, _ in first] == [PROMPT + 3, PROMPT + 2, PROMPT + 5]
    for m in (2, 3, 5, 12):
        late = model.sample(ids, N, kv_cache=True, rng_state=_state(), top_k=6, stop_sequences=stops, min_new_tokens=m,
                            return_dict_in_generate=True)
        got = _check_against_scan(late, free, PROMPT, stops, 0, minimum=m)
        assert all(end > PROMPT + m for end, _ in got)
    absolute = model.sample(ids, N, kv_cache=True, rng_state=_state(), top_k=6, stop_sequences=stops, min_length=PROMPT + 5,
                            return_dict_in_generate=True)
    _check_against_scan(absolute, free, PROMPT, stops, 0, minimum=5)


def test_prompt_lengths_give_every_row_its_own_begin(nano):
    model, ids, _ = nano
    lengths = [PROMPT, PROMPT - 2, PROMPT - 1]
    free = model.generate(ids, N, kv_cache=True, prompt_lengths=lengths, return_dict_in_generate=True).sequences
    r = free.tolist()
    # row 1: a phrase across ITS prompt's end (inside the generated text of no row at that place); row 2: its first token
    stops = [r[1][lengths[1] - 1:lengths[1] + 1], [r[2][lengths[2]]], r[0][PROMPT + 10:PROMPT + 12]]
    out = model.generate(ids, N, kv_cache=True, prompt_lengths=lengths, stop_sequences=stops, pad_token_id=5,
                         return_dict_in_generate=True)
    want = _check_against_scan(out, free, lengths, stops, 5)
    assert want[1][0] > lengths[1] + 1 and want[2] == (lengths[2] + 1, 2)
    delayed = model.generate(ids, N, kv_cache=True, prompt_lengths=lengths, stop_sequences=stops, pad_token_id=5,
                             min_new_tokens=4, return_dict_in_generate=True)
    assert _check_against_scan(delayed, free, lengths, stops, 5, minimum=4)[2][0] > lengths[2] + 4


def _pairs(row, begin):
    return [(row[t - 1], row[t]) for t in range(begin, len(row))]


def test_a_banned_phrase_never_occurs_while_its_last_id_does(nano):
    model, ids, free = nano
    r = free.tolist()
    pairs = [p for row in r for p in _pairs(row, PROMPT)]
    # bigrams of the free run whose last id also follows another id somewhere in it
    banned = [list(p) for p in dict.fromkeys(pairs) if any(q[1] == p[1] and q[0] != p[0] for q in pairs)][:6]
    assert len(banned) == 6
    out = model.sample(ids, N, kv_cache=True, rng_state=_state(), top_k=6, bad_words_ids=banned, return_dict_in_generate=True)
    assert out.sequences.shape == free.shape and torch.equal(out.sequences[:, :PROMPT], ids) and out.stop_reasons is None
    got = [p for row in out.sequences.tolist() for p in _pairs(row, PROMPT)]
    assert not any(list(p) in banned for p in got)
    assert sum(t in {b[1] for b in banned} for _, t in got) >= 3, 'the last ids vanished with the phrases: a weak test'
    # up to the first banned bigram of the free run the tokens are the free run's
    for b, row in enumerate(r):
        first = next(t for t in range(PROMPT, len(row)) if [row[t - 1], row[t]] in banned) if any(
            [row[t - 1], row[t]] in banned for t in range(PROMPT, len(row))) else len(row)
        assert out.sequences[b, :first].tolist() == row[:first] and (first == len(row) or out.sequences[b, first] != row[first])
    # a phrase whose first id is the prompt's last one: the prompt counts
    across = [[r[0][PROMPT - 1], r[0][PROMPT]]]
    moved = model.sample(ids, N, kv_cache=True, rng_state=_state(), top_k=6, bad_words_ids=across)
    assert moved[0, PROMPT] != r[0][PROMPT] and torch.equal(moved[1:], free[1:])
    greedy = model.generate(ids, N, kv_cache=True)
    g = greedy.tolist()
    word = [[g[0][PROMPT + 4], g[0][PROMPT + 5]], [g[1][PROMPT + 1]]]
    held = model.generate(ids, N, kv_cache=True, bad_words_ids=word)
    assert not any(list(p) == word[0] for row in held.tolist() for p in _pairs(row, PROMPT))
    assert not (held[:, PROMPT:] == word[1][0]).any() and torch.equal(held[0, :PROMPT + 5], greedy[0, :PROMPT + 5])


def test_intervened_wrapper_takes_both_options(nano):
    from src.models.intervened_models import WeightedBackpackLMHeadModel
    model, ids, _ = nano
    cw = torch.rand(VOCAB, model.config.num_content_vectors, generator=torch.Generator().manual_seed(11)) * 3
    wrapper = WeightedBackpackLMHeadModel(model, cw, None, 0.1, anneal=False, upweight_nearby=True).eval()
    free = wrapper.generate(ids, N, kv_cache=True, device_pick=True)
    r = free.tolist()
    stops = [r[0][PROMPT + 8:PROMPT + 10], r[2][PROMPT + 15:PROMPT + 18]]
    out = wrapper.generate(ids, N, kv_cache=True, stop_sequences=stops, return_dict_in_generate=True)
    _check_against_scan(out, free, PROMPT, stops, 0)
    word = [r[1][PROMPT + 2:PROMPT + 4]]
    both = wrapper.generate(ids, N, kv_cache=True, stop_sequences=stops, bad_words_ids=word, return_dict_in_generate=True)
    assert not any(list(p) == word[0] for row in both.sequences.tolist() for p in _pairs(row, PROMPT))
    assert torch.equal(both.sequences[0], out.sequences[0]) or r[0][:out.lengths[0]].count(word[0][0]) > 0
    drawn = wrapper.sample(ids, N, kv_cache=True, stop_sequences=stops, bad_words_ids=word, rng_state=_state(), top_k=4,
                           return_dict_in_generate=True)
    assert drawn.stop_reasons.shape == (3,) and not any(list(p) == word[0] for row in drawn.sequences.tolist() for p in _pairs(row, PROMPT))


def test_the_phrases_need_the_kv_cache_and_sane_values(nano):
    model, ids, _ = nano
    for kw in (dict(bad_words_ids=[[3, 4]]), dict(stop_sequences=[[3, 4]])):
        for cg in (False, True):
            with pytest.raises(ValueError, match='kv_cache'):
                model.generate(ids, PROMPT + 2, cg=cg, **kw)
            with pytest.raises(ValueError, match='kv_cache'):
                model.sample(ids, PROMPT + 2, cg=cg, **kw)
        with pytest.raises(ValueError, match='beam_search takes no'):
            model.beam_search(ids, PROMPT + 2, 2, **kw)
    with pytest.raises(ValueError, match='bad_words_ids and stop_sequences need kv_cache'):
        model.generate(ids, PROMPT + 2, stop_sequences=[[1]])
    for bad in ([[]], [[1] * 65], [[1]] * 1025):
        for name in ('bad_words_ids', 'stop_sequences'):
            with pytest.raises(ValueError):
                model.generate(ids, PROMPT + 2, kv_cache=True, **{name: bad})
            with pytest.raises(ValueError):
                bp_hip.pack_phrases(bad, 'cpu', name)
    assert PickOptions(stop_sequences=[[1]]).controlled and not PickOptions(stop_sequences=[[1]]).limited
    assert PickOptions(bad_words_ids=[[1]]).controlled and PickOptions(bad_words_ids=[[1]]).limited
    assert not PickOptions().controlled and PickOptions().bad_words_ids is None and PickOptions().stop_sequences is None


# ---- the binding and the C ABI -------------------------------------------------------------------------------------------------------

def test_pick_form_answers_for_new_and_old_arguments():
    f = bp_hip.pick_form
    assert f() == 'plain' and f(repetition_penalty=1.2) == 'ctl' and f(eos_token_id=3) == 'ctl'
    assert f(finished=torch.zeros(2, dtype=torch.int32)) == 'ctl' and f(min_length=3) == 'ctl'
    assert f(no_repeat_ngram_size=2) == 'lim' and f(penalty_begin=4) == 'lim' and f(suppress_tokens=torch.zeros(1)) == 'lim'
    assert f(frequency_penalty=0.5) == 'lim' and f(presence_penalty=0.5) == 'lim'
    per_row = torch.zeros(2, dtype=torch.int32)
    assert f(penalty_begin=per_row) == 'rows' and f(min_length=per_row) == 'rows' and f(1.2, 3, 3, per_row) == 'rows'
    assert f(bad_words_ids=[[1, 2]]) == 'phrases' and f(stop_sequences=[[1]]) == 'phrases'
    assert f(penalty_begin=per_row, stop_sequences=[[1]]) == 'phrases' and f(no_repeat_ngram_size=2, bad_words_ids=[]) == 'phrases'
    ids, offsets = bp_hip.pack_phrases([[5, 6], [7], [8, 9, 10]], 'cpu')
    assert ids.tolist() == [5, 6, 7, 8, 9, 10] and offsets.tolist() == [0, 2, 3, 6] and ids.dtype == offsets.dtype == torch.int32
    assert bp_hip.pack_phrases((ids, offsets), 'cpu')[0] is ids
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.pick_token(torch.zeros(2, 8), stop_sequences=[[1]], sequences=torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='ends and reasons need'):
        bp_hip.pick_token(torch.zeros(2, 8), ends=torch.zeros(2, dtype=torch.int32))


def test_pick_token_phrases_rejects_bad_arguments_before_any_launch():
    h = bp_hip.lib()
    assert h.bp_abi_version() == 11
    p, null, odd = ctypes.c_void_p(0x1000), None, ctypes.c_void_p(0x1002)

    def call(logits=p, tokens=p, sequences=p, stats=null, rng=p, counters=null, finished=p, batch=2, vocab=100, row_stride=100,
             tokens_stride=1, seq_stride=8, seq_cols=8, do_sample=1, temperature=1.0, top_k=0, top_p=1.0, theta=1.2, eos=7,
             pad=7, min_length=0, ngram=3, fp=0.5, pp=0.25, begin=2, suppress=p, n_suppress=4, begins=null, mins=null,
             ban_ids=p, ban_offsets=p, n_ban=3, ban_total=7, stop_ids=p, stop_offsets=p, n_stop=2, stop_total=5, ends=p,
             reasons=p, dtype=1):
        return h.bp_pick_token_phrases(logits, tokens, sequences, stats, rng, counters, finished, batch, vocab, row_stride,
                                       tokens_stride, seq_stride, seq_cols, do_sample, temperature, top_k, top_p, theta, eos, pad,
                                       min_length, ngram, fp, pp, begin, suppress, n_suppress, begins, mins, ban_ids, ban_offsets,
                                       n_ban, ban_total, stop_ids, stop_offsets, n_stop, stop_total, ends, reasons, dtype, null)
    # everything bp_pick_token_lim_rows rejects, with its codes
    assert call(dtype=3) == -1 and call(dtype=-1) == -1
    for kw in (dict(batch=0), dict(vocab=0), dict(vocab=2 ** 23 + 1, row_stride=2 ** 24), dict(row_stride=99),
               dict(tokens_stride=0), dict(logits=null), dict(tokens=null),
               dict(sequences=p, seq_cols=0, seq_stride=8), dict(sequences=p, seq_cols=8, seq_stride=7),
               dict(logits=ctypes.c_void_p(0x1001)), dict(logits=odd, dtype=2),
               dict(tokens=ctypes.c_void_p(0x1004)), dict(stats=odd), dict(counters=odd), dict(rng=ctypes.c_void_p(0x1004)),
               dict(eos=100), dict(pad=-1), dict(pad=100), dict(min_length=-1), dict(finished=odd),
               dict(vocab=2 ** 19 + 1, row_stride=2 ** 20), dict(ngram=-1), dict(ngram=65), dict(n_suppress=-1), dict(begin=-1),
               dict(seq_cols=8192, seq_stride=8192), dict(begins=odd), dict(mins=odd),
               dict(vocab=2 ** 19, row_stride=2 ** 19, fp=0.0, pp=0.0)):
        assert call(**kw) == -3, kw
    for bad in (0.0, -1.0, NAN, INF):
        assert call(temperature=bad) == -4, bad
    for bad in (0.0, -0.5, 1.0000001, NAN):
        assert call(top_p=bad) == -10, bad
    assert call(rng=null) == -10 and call(finished=null) == -10 and call(theta=0.0) == -10 and call(fp=NAN) == -10
    assert call(suppress=null) == -10
    # its own: BP_ERR_SAMPLING
    off = dict(theta=1.0, ngram=0, fp=0.0, pp=0.0, n_suppress=0)
    no_seq = dict(sequences=null, seq_stride=0, seq_cols=0, **off)
    assert call(ban_ids=null) == -10 and call(ban_offsets=null) == -10
    assert call(stop_ids=null) == -10 and call(stop_offsets=null) == -10
    assert call(n_stop=0, **no_seq) == -10 and call(n_ban=0, **no_seq) == -10
    assert call(finished=null, eos=-1, n_ban=0, **off) == -10       # stop phrases without flags
    # BP_ERR_SHAPE
    for kw in (dict(n_ban=-1), dict(n_stop=-1), dict(ban_total=-1), dict(stop_total=-1), dict(n_ban=1025), dict(n_stop=1025),
               dict(ban_ids=odd), dict(ban_offsets=odd), dict(stop_ids=odd), dict(stop_offsets=odd), dict(ends=odd), dict(reasons=odd),
               dict(n_ban=0, ban_total=-1), dict(n_stop=0, ban_ids=null, ban_offsets=null, n_ban=-2),
               dict(vocab=2 ** 19 + 1, row_stride=2 ** 20, n_stop=0, **off),
               # LDS: at 2^19 entries one bitmap fits, the history's and the ban list's do not
               dict(vocab=2 ** 19, row_stride=2 ** 19, ngram=0, fp=0.0, pp=0.0, n_suppress=0)):
        assert call(**kw) == -3, kw
    assert L.lds_bytes(2 ** 19, 8, 1.2, 0, 0.0, 0.0, n_suppress=1) > L.MAX_LDS_BYTES      # n_ban > 0 switches the same bitmap on
    assert P.MAX_PHRASES == bp_hip.PICK_MAX_PHRASES == 1024 and P.MAX_PHRASE_LEN == bp_hip.PICK_MAX_PHRASE_LEN == L.MAX_NGRAM



# ---- the code object -----------------------------------------------------------------------------------------------------------------

def test_phrased_pick_kernels_use_no_scratch_spill_nothing_and_keep_the_static_lds():
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
    ks = KR.kernels([os.path.join(KR.BUILD, 'pick_token_phrases.o')])
    # the stop phrases are matched inside the pick: no second kernel
    assert {k['name'].replace(' ', '') for k in ks} == {'pick_token_kernel<Phrased<BF16>>', 'pick_token_kernel<Phrased<F16>>',
                                                        'pick_token_kernel<Phrased<float>>'}
    for k in ks:
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
        assert k['group_segment_fixed_size'] == L.STATIC_LDS == 68112 and k['max_flat_workgroup_size'] == 1024, k
        assert k['vgpr_count'] <= 128, k                      # 16 waves a workgroup: four per SIMD, 512 / 4 registers each
