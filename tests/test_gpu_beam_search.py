"""GPU: beam search on the decode models.  The test drives the loop itself from the public pieces (model step,
bp_hip.beam_pick, bp_hip.beam_copy_rows), holds every step's pick against tests/beam_ref.py on the same logits, and
`model.beam_search` must then return the same tensors bit for bit, eagerly and with the captured step.  The caches of the
final slots must be those of a fresh run that teacher-forces the final hypotheses.

Decided groups (beam_ref.decided) must match the reference exactly.  The cap on undecided picks, at most 5 % of them, is
held by every case of its own -- a (model, W, form) over its three prompt sets -- and is a condition on the inputs: whether
a pick is decided is a property of the logits alone.  The bf16 logits of these randomly initialised models are far flatter
than the drawn rows of test_gpu_beam_pick.py, and with W = 4 the five best candidates of a group crowd together: over
prompt seeds 0..29 `small` leaves 3 % of its W = 4 picks undecided (0 to 5 of a set's 54) and `mini_k4` 7 % (1 to 9 of 54;
none at W = 1), so the
prompt sets of PROMPT_SEEDS are ones whose logits meet the condition in every case.  A change to the model's arithmetic
moves the logits: if the cap then fails, that is the inputs no longer meeting the condition, and other seeds are chosen
by the same measure.  An undecided pick is not dropped either: beam_ref.check_near_tie holds it to everything but the
order of the candidates that are closer than the tolerances.

Every buffer the driven loop hands to the two kernels lies between canary rows (one group of rows on either side of the
scores, flags, parents and tokens, a row on either side of the sequences), which the whole loop, the EOS loop included,
must leave as they were."""
import numpy as np
import pytest
import torch

import beam_ref as R
from decode_support import DEV, VOCAB, _bp, _model, _same_bits
from src.utils.generation import InferenceParams, _beam_row_sets

pytestmark = pytest.mark.gpu

PROMPT, MAX_LENGTH, BATCH = 5, 24, 3
WIDTH = MAX_LENGTH - 1
CAPACITY = (WIDTH + 3) // 4 * 4          # what beam_search gives its caches: rows on 16-byte boundaries


PROMPT_SEEDS = {1: (1, 11, 21), 4: (27, 23, 21)}     # per W: three prompt sets whose picks meet the cap in every case (see above)
CANARY = -9


@pytest.fixture(scope='module', params=['small', 'mini_k4'])
def model(request):
    m = _model(request.param)
    mode = m.transformer.sense_table_mode
    yield m
    m.transformer.sense_table_mode = mode              # the cached model goes back as it came


def _prompts(seed=0):
    return torch.randint(0, VOCAB, (BATCH, PROMPT), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _guarded(rows, guard, fill, dtype, cols=None):
    """A device buffer of `rows` rows filled with `fill` between `guard` canary rows on either side: (view, whole)."""
    shape = (rows + 2 * guard,) if cols is None else (rows + 2 * guard, cols)
    whole = torch.full(shape, CANARY, dtype=dtype, device=DEV)
    whole[guard:-guard] = fill
    return whole[guard:-guard], whole


def _drive(model, ids, W, eos=None, pad=None):
    """The loop of beam_search from the public pieces, every pick checked against the reference.  Returns
    (sequences (B W, WIDTH), beam_scores, finished, the InferenceParams, undecided groups, picks)."""
    bp = _bp()
    rows = ids.shape[0] * W
    ip = InferenceParams(max_sequence_len=CAPACITY, max_batch_size=rows)
    ip.lengths_per_sample = torch.zeros((rows,), dtype=torch.int32, device=DEV)
    sequences, sequences_w = _guarded(rows, 1, 0, torch.int64, CAPACITY)
    sequences = sequences[:, :WIDTH]
    sequences[:, :PROMPT] = ids.repeat_interleave(W, dim=0)
    static_ids, static_w = _guarded(rows, W, 0, torch.int64, 1)
    scores, scores_w = _guarded(rows, W, float('-inf'), torch.float32)
    scores[::W] = 0.0
    finished, finished_w = _guarded(rows, W, 0, torch.int32) if eos is not None else (None, None)
    parent, parent_w = _guarded(rows, W, 0, torch.int32)
    parent.copy_(torch.arange(rows, dtype=torch.int32, device=DEV))
    undecided = picks = 0
    with torch.inference_mode():
        logits = model(ids.repeat_interleave(W, dim=0), inference_params=ip).logits[:, -1]
        ip.sequence_len_offset = PROMPT
        ip.lengths_per_sample.fill_(PROMPT)
        sets = _beam_row_sets(ip, sequences)
        for column in range(PROMPT, WIDTH):
            if column > PROMPT:
                logits = model(static_ids, inference_params=ip).logits[:, -1]
                ip.lengths_per_sample += 1
                ip.sequence_len_offset += 1
            seen, old_scores = logits.float().cpu().numpy(), scores.cpu().numpy()
            fin_before = None if finished is None else finished.cpu().numpy()
            e, p = -1 if eos is None else eos, 0 if pad is None else pad
            ref = R.beam_pick(seen, old_scores, fin_before, W, eos=e, pad=p)
            bp.beam_pick(logits, scores, parent, W, finished=finished, tokens=static_ids, sequences=sequences,
                         counters=ip.lengths_per_sample, eos_token_id=eos, pad_token_id=pad)
            got = (parent.cpu().numpy(), static_ids.view(-1).cpu().numpy(), scores.cpu().numpy(),
                   None if finished is None else finished.cpu().numpy())
            undecided += R.check(got, ref, W, logits.shape[-1], check_finished=finished is not None,
                                 inputs=(seen, old_scores, fin_before, e, p))
            picks += ids.shape[0]
            bp.beam_copy_rows(sets, parent, ip.lengths_per_sample, PROMPT)
    for whole, guard in ((sequences_w, 1), (static_w, W), (scores_w, W), (finished_w, W), (parent_w, W)):
        assert whole is None or bool((whole[:guard] == CANARY).all() and (whole[-guard:] == CANARY).all()), 'canary rows'
    assert (sequences_w[1:-1, WIDTH:] == 0).all(), 'the columns past the width are not written'
    return sequences, scores, finished, ip, undecided, picks


def _drive_three(model, W, form):
    """The driven loop on the three prompt sets of W, every pick checked, the case's cap asserted: the first set's results."""
    model.transformer.sense_table_mode = 'cached' if form == 'table' else 'batch'
    runs = [_drive(model, _prompts(seed=seed), W) for seed in PROMPT_SEEDS[W]]
    undecided, picks = sum(r[4] for r in runs), sum(r[5] for r in runs)
    print(f'{form} W={W}: {undecided} of {picks} picks undecided, held to beam_ref.check_near_tie')
    assert picks == 3 * BATCH * (WIDTH - PROMPT) and undecided <= R.UNDECIDED_CAP * picks
    return runs[0]


def _teacher_forced(model, sequences):
    """A fresh run at the same batch shape that feeds the rows of `sequences`: its InferenceParams."""
    rows = sequences.shape[0]
    ip = InferenceParams(max_sequence_len=CAPACITY, max_batch_size=rows)
    ip.lengths_per_sample = torch.zeros((rows,), dtype=torch.int32, device=DEV)
    with torch.inference_mode():
        model(sequences[:, :PROMPT].contiguous(), inference_params=ip)
        ip.sequence_len_offset = PROMPT
        ip.lengths_per_sample.fill_(PROMPT)
        for t in range(PROMPT, WIDTH - 1):
            model(sequences[:, t:t + 1].contiguous(), inference_params=ip)
            ip.lengths_per_sample += 1
            ip.sequence_len_offset += 1
    return ip


def _cache_sets(ip):
    return _beam_row_sets(ip, torch.zeros((ip.max_batch_size, CAPACITY), dtype=torch.int64, device=DEV))[:-1]


@pytest.mark.parametrize('form', ['table', 'content'])
@pytest.mark.parametrize('W', [1, 4])
def test_beam_search_is_the_driven_loop_and_its_caches_follow(model, W, form):
    ids = _prompts(seed=PROMPT_SEEDS[W][0])
    sequences, scores, _, ip, _, _ = _drive_three(model, W, form)
    caches = ip.key_value_memory_dict
    assert ('backpack_content' in caches) == (form == 'content')
    for cg in (False, True):
        out = model.beam_search(ids, MAX_LENGTH, W, return_dict_in_generate=True, cg=cg)
        assert torch.equal(out.beam_sequences.view(-1, WIDTH), sequences), cg
        assert _same_bits(out.beam_scores.view(-1), scores), cg
        best = out.beam_scores.argmax(dim=1)
        assert torch.equal(out.sequences, out.beam_sequences[torch.arange(BATCH, device=DEV), best])
    filled = WIDTH - 1                                                  # positions the last model step has appended
    if form == 'table':
        assert torch.equal(caches['backpack_rows'][:, :filled].long(), sequences[:, :filled])
    else:
        want = torch.arange(BATCH * W, device=DEV)[:, None] * CAPACITY + torch.arange(CAPACITY, device=DEV)[None, :]
        assert torch.equal(caches['backpack_rows'][:, :filled].long(), want[:, :filled])
    # the caches of the final slots against a fresh run that teacher-forces the final hypotheses
    fresh, again = _teacher_forced(model, sequences), _teacher_forced(model, sequences)
    for got, ref, ref2 in zip(_cache_sets(ip), _cache_sets(fresh), _cache_sets(again)):
        got, ref, ref2 = got[:, :filled], ref[:, :filled], ref2[:, :filled]
        assert _same_bits(ref.contiguous(), ref2.contiguous()), 'two teacher-forced runs differ: the hardware is not repeatable here'
        diff = (got.float() - ref.float()).abs().max().item()
        print(f'  cache set {tuple(got.shape)} {got.dtype}: max |beam - teacher-forced| = {diff:.3e}')
        assert _same_bits(got.contiguous(), ref.contiguous())


def test_one_beam_is_greedy_with_the_device_pick(model):
    model.transformer.sense_table_mode = 'cached'
    ids = _prompts(seed=9)
    want = model.generate(ids, MAX_LENGTH, kv_cache=True, device_pick=True)
    for cg in (False, True):
        assert torch.equal(model.beam_search(ids, MAX_LENGTH, 1, cg=cg), want)


def test_eos_stops_the_loop_and_freezes_the_finished_rows(model):
    model.transformer.sense_table_mode = 'cached'
    W, pad = 4, 7
    ids = _prompts(seed=4)
    plain = model.beam_search(ids, MAX_LENGTH, W, return_dict_in_generate=True)
    eos = int(plain.sequences[0, PROMPT + 2])
    sequences, scores, finished, _, undecided, picks = _drive(model, ids, W, eos=eos, pad=pad)
    print(f'EOS run: {undecided} of {picks} picks undecided, held to beam_ref.check_near_tie')
    assert finished.any()
    outs = [model.beam_search(ids, MAX_LENGTH, W, return_dict_in_generate=True, eos_token_id=eos, pad_token_id=pad, cg=cg,
                              stop_check_every=every) for cg, every in ((False, 1), (False, 1000), (True, 2))]
    cols = outs[0].beam_sequences.shape[2]
    for out in outs:
        assert torch.equal(out.beam_sequences, outs[0].beam_sequences) and _same_bits(out.beam_scores, outs[0].beam_scores)
        assert torch.equal(out.beam_lengths, outs[0].beam_lengths)
        assert _same_bits(out.beam_scores.view(-1), scores)
    # the driven loop ran to the end: cut at the rows' ends it is what beam_search returns
    seq, lengths = outs[0].beam_sequences.view(-1, cols), outs[0].beam_lengths.view(-1)
    for r in range(BATCH * W):
        n = int(lengths[r])
        assert torch.equal(seq[r, :n], sequences[r, :n]) and (seq[r, n:] == pad).all()
        assert bool(finished[r]) == bool(seq[r, n - 1] == eos and n > PROMPT)
        assert (sequences[r, n:] == pad).all() or not finished[r]      # a frozen row keeps stepping on the pad
