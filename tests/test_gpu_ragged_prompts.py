"""GPU: generation from right-padded prompts of different lengths (prompt_lengths) on the decode models -- uniform lengths are
the call without the argument, eager equals captured, the pad columns and the pad id do not matter, every pick against the
restatement (tests/pick_lim_ref.py, called with the row's own begin) on the logits of a teacher-forced run that makes the
loop's own calls, those logits against the uncached forward of every row's own unpadded sequence (the whole-model rule), and
beam search with groups of different lengths against tests/beam_ref.py, its caches against a teacher-forced run."""
import numpy as np
import pytest
import torch

import beam_ref as B
import pick_lim_ref as L
import pick_ref as R
import ragged_support as G
from decode_support import DEV, VOCAB, _bp, _fp32_twin, _model, _same_bits
from ragged_support import BATCH, LENGTHS, MAX_LENGTH, N, S
from src.utils.generation import InferenceParams, _beam_row_sets

pytestmark = pytest.mark.gpu

SEED, OFFSET = 1234, 77
WIDTH = S + N
LIMITS = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, frequency_penalty=0.5, presence_penalty=0.25)


def _state():
    return torch.tensor([SEED, OFFSET], dtype=torch.int64, device=DEV)


def _ids(batch=BATCH, seed=5):
    return torch.randint(0, VOCAB, (batch, S), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


@pytest.fixture(scope='module', params=['small', 'mini_k4'])
def case(request):
    model = _model(request.param, seed=2)
    ids = _ids()
    free = model.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, return_dict_in_generate=True, output_scores=True)
    return request.param, model, ids, free


def test_uniform_lengths_are_the_call_without_the_argument(case):
    _, model, ids, _ = case
    full = [S] * BATCH
    plain = model.generate(ids, MAX_LENGTH, kv_cache=True, device_pick=True)
    eos = int(plain[2, S + N // 2])
    for cg in (False, True):
        for call, more in ((model.generate, dict(device_pick=True)), (model.sample, dict(rng_state=_state(), top_k=20)),
                           (model.generate, dict(eos_token_id=eos, pad_token_id=3, **LIMITS)),
                           (model.sample, dict(rng_state=_state(), temperature=0.9, eos_token_id=eos, min_length=S + 3, **LIMITS))):
            want = call(ids, MAX_LENGTH, kv_cache=True, cg=cg, return_dict_in_generate=True, **more)
            got = call(ids, MAX_LENGTH, kv_cache=True, cg=cg, return_dict_in_generate=True, prompt_lengths=full, **more)
            assert torch.equal(got.sequences, want.sequences), (cg, more)
            if 'eos_token_id' in more:
                assert torch.equal(got.lengths, want.lengths)
            else:
                assert got.lengths.tolist() == [WIDTH] * BATCH


def test_eager_equals_captured_and_the_rows_are_laid_out_by_the_contract(case):
    _, model, ids, free = case
    seq = free.sequences
    assert seq.shape == (BATCH, WIDTH) and free.lengths.tolist() == [b + N for b in LENGTHS]
    for b, begin in enumerate(LENGTHS):
        assert torch.equal(seq[b, :begin], ids[b, :begin]) and (seq[b, begin + N:] == 0).all()
    eos = int(seq[1, LENGTHS[1] + 4])
    for call, more in ((model.generate, {}), (model.sample, dict(rng_state=_state(), top_k=20, temperature=0.9)),
                       (model.generate, LIMITS), (model.sample, dict(rng_state=_state(), top_p=0.9, **LIMITS)),
                       (model.generate, dict(eos_token_id=eos, pad_token_id=9, min_new_tokens=2, **LIMITS))):
        eager = call(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, return_dict_in_generate=True, **more)
        graph = call(ids, MAX_LENGTH, kv_cache=True, cg=True, prompt_lengths=torch.tensor(LENGTHS, device=DEV),
                     return_dict_in_generate=True, **more)
        assert torch.equal(eager.sequences, graph.sequences) and torch.equal(eager.lengths, graph.lengths), more
        if not more:
            assert torch.equal(eager.sequences, seq)
        if 'eos_token_id' in more:
            want = G.ends(eager.sequences.cpu(), LENGTHS, N, eos)
            assert eager.lengths.tolist() == want and eager.sequences.shape[1] == max(want)
            for b, begin in enumerate(LENGTHS):
                assert eos not in eager.sequences[b, begin:begin + 2].tolist() and (eager.sequences[b, want[b]:] == 9).all()


def test_pad_columns_and_pad_id_do_not_matter(case):
    _, model, ids, free = case
    dirty = ids.clone()
    for b, begin in enumerate(LENGTHS):
        dirty[b, begin:] = torch.randint(0, VOCAB, (S - begin,), generator=torch.Generator().manual_seed(b)).to(DEV)
    for cg in (False, True):
        assert torch.equal(model.generate(dirty, MAX_LENGTH, kv_cache=True, cg=cg, prompt_lengths=LENGTHS), free.sequences)
        kw = dict(kv_cache=True, cg=cg, rng_state=_state(), top_p=0.9, prompt_lengths=LENGTHS, **LIMITS)
        assert torch.equal(model.sample(dirty, MAX_LENGTH, **kw), model.sample(ids, MAX_LENGTH, **kw))
        a, b = (model.generate(ids, MAX_LENGTH, kv_cache=True, cg=cg, prompt_lengths=LENGTHS, pad_token_id=p) for p in (3, 7))
        for r, begin in enumerate(LENGTHS):
            assert torch.equal(a[r, :begin + N], b[r, :begin + N]) and torch.equal(a[r, :begin + N], free.sequences[r, :begin + N])
            assert (a[r, begin + N:] == 3).all() and (b[r, begin + N:] == 7).all()


def test_every_pick_against_the_restatement_on_teacher_forced_logits(case):
    name, model, ids, free = case
    vocab = model.lm_head.weight.shape[0]
    greedy = model.generate(ids, MAX_LENGTH, kv_cache=True, cg=True, prompt_lengths=LENGTHS, **LIMITS)
    drawn = model.sample(ids, MAX_LENGTH, kv_cache=True, cg=True, prompt_lengths=LENGTHS, rng_state=_state(), top_k=10,
                         temperature=0.9, **LIMITS)
    assert not torch.equal(greedy, free.sequences), 'the limits changed nothing: a weak test'
    # the teacher-forced run makes the calls of the loop itself (same kernels, same shapes, no atomics): its logits are the
    # loop's bit for bit -- two such runs are, and the first of them is what the loop returned as `scores`
    first, _ = G.loop_logits(model, ids, LENGTHS, free.sequences, N)
    again, _ = G.loop_logits(model, ids, LENGTHS, free.sequences, N)
    assert _same_bits(first, again), 'two teacher-forced runs differ: the hardware is not repeatable here'
    assert _same_bits(first[0], free.scores[0])
    lg, _ = G.loop_logits(model, ids, LENGTHS, greedy, N)
    ld, _ = G.loop_logits(model, ids, LENGTHS, drawn, N)
    lg, ld = lg.float().cpu().numpy(), ld.float().cpu().numpy()
    rows_g, rows_d = greedy.cpu().numpy(), drawn.cpu().numpy()
    eps = R.epsilon(vocab)
    undecided = picks = 0
    for b, begin in enumerate(LENGTHS):
        for i in range(N):
            t = begin + i
            v = L.values(lg[i, b], None, rows_g[b], t, vocab, penalty_begin=begin, **LIMITS)
            top2 = np.sort(v)[-2:]
            picks += 1
            if top2[1] > top2[0]:
                assert int(rows_g[b, t]) == int(np.argmax(v)), (name, b, t)
            else:
                undecided += 1
                assert v[int(rows_g[b, t])] == top2[1], (name, b, t)
            z = L.values(ld[i, b], 0.9, rows_d[b], t, vocab, penalty_begin=begin, **LIMITS)
            R.assert_draw(int(rows_d[b, t]), z, R.kept_set(z, 10, 1.0), R.uniform(SEED, OFFSET, b, t), eps, what=(name, b, t))
    print(f'{name}: {undecided} of {picks} greedy picks undecided')
    assert picks == BATCH * N and undecided <= 0.05 * picks, f'{undecided} of {picks} greedy picks undecided'


def _eager16_twin(model):
    """The eager op sequence (use_flash_attn=False, no fused layer) in the model's own 16-bit type with the same weights: the
    yardstick of the whole-model rule."""
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    kw = {k: v for k, v in model.config.to_dict().items() if k in ('n_embd', 'n_head', 'n_layer', 'num_content_vectors',
                                                                   'vocab_size', 'n_positions')}
    twin = BackpackLMHeadModel(BackpackConfig(scale_attn_by_inverse_layer_idx=True, use_flash_attn=False, **kw))
    twin.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    return twin.to(device=DEV, dtype=model.lm_head.weight.dtype).eval()


def test_the_loops_logits_against_the_uncached_forward_of_every_rows_own_sequence(case):
    """The project's whole-model rule (tests/test_gpu_configs.py): the error against the fp32 twin is at
    most 3 x the error of the 16-bit eager twin on the same input (+ 1e-3, as there)."""
    name, model, ids, free = case
    logits, _ = G.loop_logits(model, ids, LENGTHS, free.sequences, N)              # (N, batch, vocab), the loop's own
    twin, eager = _fp32_twin(model), _eager16_twin(model)
    with torch.inference_mode():
        for b, begin in enumerate(LENGTHS):
            row = free.sequences[b:b + 1, :begin + N - 1]                          # unpadded: the prompt and what was fed back
            ref = twin(row).logits[0, begin - 1:].float()
            base = (eager(row).logits[0, begin - 1:].float() - ref).abs().max().item()
            err = (logits[:, b].float() - ref).abs().max().item()
            print(f'{name} row {b} (prompt {begin}): loop {err:.3e} eager-16-bit {base:.3e} (|ref| max {ref.abs().max().item():.2f})')
            assert err <= 3 * base + 1e-3, (name, b, err, base)


# ---- beam search: groups of different lengths --------------------------------------------------------------------------------------------

GROUP_LENGTHS, W = (3, 8), 4
CAPACITY = (WIDTH + 3) // 4 * 4
# prompt sets whose picks meet the cap on undecided ones with room to spare (the measure of test_gpu_beam_search.py: whether a
# pick is decided is a property of the logits alone; over the seeds 0..11 small leaves 0 to 3 of its 62 picks undecided and
# mini_k4 2 to 7)
BEAM_SEEDS = {'small': 8, 'mini_k4': 5}


def _drive_beams(model, ids):
    """beam_search's loop from the public pieces for groups that begin at GROUP_LENGTHS, every pick checked against
    tests/beam_ref.py on the logits it saw: (sequences (B W, WIDTH), scores, the InferenceParams, undecided, picks)."""
    bp = _bp()
    rows = ids.shape[0] * W
    at = torch.tensor(GROUP_LENGTHS, device=DEV).repeat_interleave(W)
    ip = InferenceParams(max_sequence_len=CAPACITY, max_batch_size=rows)
    ip.lengths_per_sample = torch.zeros((rows,), dtype=torch.int32, device=DEV)
    sequences = torch.zeros((rows, CAPACITY), dtype=torch.int64, device=DEV)[:, :WIDTH]
    sequences[:, :S] = G.padded(ids.repeat_interleave(W, dim=0), at, 0)
    static_ids = torch.zeros((rows, 1), dtype=torch.int64, device=DEV)
    scores = torch.full((rows,), float('-inf'), dtype=torch.float32, device=DEV)
    scores[::W] = 0.0
    parent = torch.arange(rows, dtype=torch.int32, device=DEV)
    undecided = picks = 0
    with torch.inference_mode():
        logits = model(sequences[:, :S].contiguous(), inference_params=ip).logits[torch.arange(rows, device=DEV), at - 1]
        ip.sequence_len_offset = S
        ip.lengths_per_sample.copy_(at)
        sets = _beam_row_sets(ip, sequences)
        for i in range(N):
            if i > 0:
                logits = model(static_ids, inference_params=ip).logits[:, -1]
                ip.lengths_per_sample += 1
                ip.sequence_len_offset += 1
            seen, old_scores = logits.float().cpu().numpy(), scores.cpu().numpy()
            ref = B.beam_pick(seen, old_scores, None, W, eos=-1, pad=0)
            bp.beam_pick(logits, scores, parent, W, tokens=static_ids, sequences=sequences, counters=ip.lengths_per_sample)
            got = (parent.cpu().numpy(), static_ids.view(-1).cpu().numpy(), scores.cpu().numpy(), None)
            undecided += B.check(got, ref, W, logits.shape[-1], check_finished=False, inputs=(seen, old_scores, None, -1, 0))
            picks += ids.shape[0]
            bp.beam_copy_rows(sets, parent, ip.lengths_per_sample, min(GROUP_LENGTHS))
    return sequences, scores, ip, undecided, picks


def test_beam_search_with_groups_of_different_lengths(case):
    name, model, _, _ = case
    ids = _ids(len(GROUP_LENGTHS), seed=BEAM_SEEDS[name])
    sequences, scores, ip, undecided, picks = _drive_beams(model, ids)
    print(f'{name} W={W}: {undecided} of {picks} picks undecided, held to beam_ref.check_near_tie')
    assert picks == len(GROUP_LENGTHS) * N and undecided <= B.UNDECIDED_CAP * picks
    at = torch.tensor(GROUP_LENGTHS, device=DEV).repeat_interleave(W)
    for r in range(at.shape[0]):
        assert (sequences[r, int(at[r]) + N:] == 0).all()
    for cg in (False, True):
        out = model.beam_search(ids, MAX_LENGTH, W, return_dict_in_generate=True, cg=cg, prompt_lengths=GROUP_LENGTHS)
        assert torch.equal(out.beam_sequences.view(-1, WIDTH), sequences), cg
        assert _same_bits(out.beam_scores.view(-1), scores), cg
        assert torch.equal(out.beam_lengths.view(-1), at + N)
        best = out.beam_scores.argmax(dim=1)
        assert torch.equal(out.sequences, out.beam_sequences[torch.arange(len(GROUP_LENGTHS), device=DEV), best])
        assert out.lengths.tolist() == [g + N for g in GROUP_LENGTHS]
    # the caches of the final slots against a fresh run that teacher-forces the final hypotheses
    padded_rows = ids.repeat_interleave(W, dim=0)
    _, fresh = G.loop_logits(model, padded_rows, at.tolist(), sequences, N, capacity=CAPACITY)
    _, again = G.loop_logits(model, padded_rows, at.tolist(), sequences, N, capacity=CAPACITY)
    blank = torch.zeros((at.shape[0], CAPACITY), dtype=torch.int64, device=DEV)
    for got, ref, ref2 in zip(_beam_row_sets(ip, blank)[:-1], _beam_row_sets(fresh, blank)[:-1], _beam_row_sets(again, blank)[:-1]):
        for r in range(at.shape[0]):
            filled = int(at[r]) + N - 1                                   # positions the last model step has appended
            a, b, c = (t[r, :filled].contiguous() for t in (got, ref, ref2))
            assert _same_bits(b, c), 'two teacher-forced runs differ: the hardware is not repeatable here'
            assert _same_bits(a, b), (name, tuple(got.shape), r)
