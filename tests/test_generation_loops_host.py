"""CPU: which C ABI entry a set of pick options selects (bp_hip.pick_form, and the keywords _Picker hands to
bp_hip.pick_token), and how many model forwards the cached loops make on the nano model."""
import pytest
import torch

import bp_hip
from decode_support import _nano_backpack

PROMPT, N = 5, 20


# ---- routing -------------------------------------------------------------------------------------------------------------------------

# Written down from the two conditions of bp_hip.pick_token as they stood before pick_form existed: 'lim' unless
# no_repeat_ngram_size == 0, frequency_penalty == 0.0, presence_penalty == 0.0, penalty_begin == 0 and suppress_tokens is None;
# else 'ctl' unless repetition_penalty == 1.0, eos_token_id, pad_token_id and finished are None and min_length == 0; else 'plain'.
ROUTES = [
    (dict(), 'plain'),
    (dict(repetition_penalty=1.2), 'ctl'),
    (dict(eos_token_id=3), 'ctl'),
    (dict(pad_token_id=0), 'ctl'),
    (dict(min_length=4), 'ctl'),
    (dict(finished=torch.zeros(2, dtype=torch.int32)), 'ctl'),
    (dict(no_repeat_ngram_size=3), 'lim'),
    (dict(frequency_penalty=0.5), 'lim'),
    (dict(presence_penalty=-0.5), 'lim'),
    (dict(suppress_tokens=torch.zeros(0, dtype=torch.int32)), 'lim'),
    (dict(penalty_begin=7), 'lim'),
    (dict(repetition_penalty=1.2, eos_token_id=3, min_length=4, frequency_penalty=0.5), 'lim'),
]


@pytest.mark.parametrize('kw,form', ROUTES, ids=str)
def test_pick_form_routes_as_the_two_conditions_did(kw, form):
    assert bp_hip.pick_form(**kw) == form


@pytest.mark.parametrize('options,form', [(dict(), 'plain'), (dict(repetition_penalty=1.2), 'ctl'), (dict(eos_token_id=3), 'ctl'),
                                          (dict(eos_token_id=3, presence_penalty=0.5), 'lim')], ids=str)
def test_the_keywords_of_the_picker_select_the_entry_of_its_options(monkeypatch, options, form):
    """A prompt-length penalty_begin alone must not send a pick to bp_pick_token_lim."""
    from src.utils.generation import PickOptions, _Picker
    seen = []

    def recorder(logits, **kw):
        seen.append(kw)
        return torch.zeros((logits.shape[0],), dtype=torch.int64)

    class OnDevice:                    # what _Picker reads of the logits before it hands them on
        is_cuda, shape, device = True, (2, 8), torch.device('cpu')

    monkeypatch.setattr(bp_hip, 'pick_token', recorder)
    picker = _Picker(PickOptions(penalty_begin=PROMPT, **options), None, torch.device('cpu'))
    picker(OnDevice(), torch.full((2,), PROMPT, dtype=torch.int32))
    kw = {k: v for k, v in seen[0].items() if k in ('repetition_penalty', 'eos_token_id', 'pad_token_id', 'min_length', 'finished',
                                                   'no_repeat_ngram_size', 'frequency_penalty', 'presence_penalty',
                                                   'penalty_begin', 'suppress_tokens')}
    assert bp_hip.pick_form(**kw) == form
    assert (kw.get('finished') is not None) == ('eos_token_id' in options)


# ---- step counts ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def counted():
    model = _nano_backpack()
    calls = [0]
    model.register_forward_pre_hook(lambda *a: calls.__setitem__(0, calls[0] + 1))
    ids = torch.randint(0, 200, (1, PROMPT), generator=torch.Generator().manual_seed(3))

    def count(fn):
        calls[0] = 0
        out = fn()
        return calls[0], out
    return model, ids, count


# Recorded by running this test's calls on the commit before the cached-step driver (three separate loops): the driver must make
# the same number of model forwards, prefill included.
GENERATE_FORWARDS = 15                              # the prefill + (N - 1 - PROMPT) cached steps
GENERATE_EOS_FORWARDS = {1: 5, 3: 7}                # stop_check_every -> forwards, the EOS at column PROMPT + 4
BEAM_FORWARDS = 14                                  # the prefill + (N - 2 - PROMPT) cached steps: the first pick reads the prefill
BEAM_EOS_FORWARDS = {1: 4, 3: 6}                    # both hypotheses end by column PROMPT + 3


def test_forwards_of_the_cached_pick_loop(counted):
    model, ids, count = counted
    n, free = count(lambda: model.generate(ids, N, kv_cache=True, device_pick=True))
    assert free.shape == (1, N - 1)
    print('generate', n)
    assert n == GENERATE_FORWARDS
    eos = int(free[0, PROMPT + 4])
    assert eos not in free[0, PROMPT:PROMPT + 4].tolist()
    for every, want in GENERATE_EOS_FORWARDS.items():
        n, out = count(lambda: model.generate(ids, N, kv_cache=True, device_pick=True, eos_token_id=eos, stop_check_every=every,
                                              return_dict_in_generate=True))
        print('generate eos every', every, n)
        assert out.lengths.tolist() == [PROMPT + 5] and n == want, (every, n)


def test_forwards_of_beam_search(counted):
    model, ids, count = counted
    n, free = count(lambda: model.beam_search(ids, N, 2, return_dict_in_generate=True))
    print('beam', n)
    assert n == BEAM_FORWARDS
    eos = int(free.beam_sequences[0, 0, PROMPT + 2])
    for every, want in BEAM_EOS_FORWARDS.items():
        n, out = count(lambda: model.beam_search(ids, N, 2, eos_token_id=eos, stop_check_every=every, return_dict_in_generate=True))
        print('beam eos every', every, n, out.beam_lengths.tolist())
        assert int(out.beam_lengths.max()) < N - 1, 'both hypotheses must end early: a weak test otherwise'
        assert n == want, (every, n)
