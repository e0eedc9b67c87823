"""GPU: the packed prefill -- model(packed ids, inference_params, cu_seqlens, max_seqlen) at sequence_len_offset 0 and
generate / sample(..., prompt_lengths, kv_cache=True, packed_prefill=True) -- on the two-layer decode models: the same bits as
the packed forward, caches that hold nothing behind a row's prompt, every pick against the restatement on teacher-forced logits
made by the loop's own calls, those logits against the uncached forward of every row's own sequence (the whole-model rule: what
proves that the scattered caches are the right ones), the loop's behaviour, and the models that run the padded prefill."""
import warnings

import numpy as np
import pytest
import torch

import pick_lim_ref as L
import pick_ref as R
import ragged_support as G
from decode_support import DEV, VOCAB, _fp32_twin, _model, _same_bits
from packed_prefill_support import BATCH, LENGTHS, MAX_LENGTH, N, S, WIDTH, pack, packed_loop_logits, padded_ids
from src.utils.generation import InferenceParams

pytestmark = pytest.mark.gpu

SEED, OFFSET = 1234, 77
DRAW = dict(top_k=10, temperature=0.9, repetition_penalty=1.2, no_repeat_ngram_size=3)
# Whether a greedy pick is decided is a property of the logits alone: a randomly initialised model's bf16 logits tie exactly now
# and then.  Over the model seeds 0..7 and the ids seeds 3..5 the 36 picks of the case below left 0 to 5 undecided; model seed 5
# left none with any of the three, and with ids seed 5 its smallest top-2 margin was 0.0156, two bf16 steps at that magnitude.
MODEL_SEED, IDS_SEED = 5, 5


def _state():
    return torch.tensor([SEED, OFFSET], dtype=torch.int64, device=DEV)


@pytest.fixture(scope='module')
def case():
    model = _model('small', seed=MODEL_SEED)
    ids = padded_ids(VOCAB, DEV, seed=IDS_SEED)
    free = model.generate(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, packed_prefill=True,
                          return_dict_in_generate=True, output_scores=True)
    logits, _ = packed_loop_logits(model, ids, LENGTHS, free.sequences, N)
    return model, ids, free, logits


# ---- the model call ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', ['cached', 'batch', 'off'])
def test_same_bits_as_the_packed_forward_and_nothing_cached_behind_a_prompt(case, mode):
    """The prefill makes the launches of the packed forward on the same shapes and adds the scatters: its logits are that
    forward's bit for bit.  ('batch' below its dedup threshold runs the content network per position in both calls.)  The
    caches are a slice of a larger batch (batch_size_offset 1): nothing outside the slice, and nothing at or behind a row's
    length, is written."""
    model, ids, _, _ = case
    t = model.transformer
    packed, cu, longest = pack(ids, LENGTHS)
    keep, b0, capacity = t.sense_table_mode, 1, S + 3
    try:
        t.sense_table_mode = mode
        with torch.inference_mode():
            plain = model(packed, cu_seqlens=cu, max_seqlen=longest).logits
            ip = InferenceParams(max_sequence_len=capacity, max_batch_size=BATCH + 2, batch_size_offset=b0)
            got = model(packed, inference_params=ip, cu_seqlens=cu, max_seqlen=longest).logits
    finally:
        t.sense_table_mode = keep
    assert got.shape == (sum(LENGTHS), model.lm_head.weight.shape[0]) and _same_bits(got, plain)
    caches = ip.key_value_memory_dict
    content_form = mode != 'cached'
    assert ('backpack_content' in caches) == content_form
    layers = [caches[i] for i in range(model.config.n_layer)]
    assert all(c.shape[:3] == (BATCH + 2, capacity, 2) for c in layers)
    padded = [caches['backpack_sense_k']] + layers
    if content_form:
        padded.append(caches['backpack_content'].view(BATCH + 2, capacity, *caches['backpack_content'].shape[1:]))
        iota = torch.arange(b0, b0 + BATCH, device=DEV)[:, None] * capacity + torch.arange(capacity, device=DEV)
        assert torch.equal(caches['backpack_rows'][b0:b0 + BATCH].long(), iota)
    else:
        padded.append(caches['backpack_rows'])
        for b, n in enumerate(LENGTHS):
            assert torch.equal(caches['backpack_rows'][b0 + b, :n].long(), ids[b, :n])
    for c in padded:
        assert not c[:b0].any() and not c[b0 + BATCH:].any()
        for b, n in enumerate(LENGTHS):
            assert not c[b0 + b, n:].any(), (mode, tuple(c.shape), b)
            assert c[b0 + b, :n].any(), (mode, tuple(c.shape), b)
    # the trunk alone: hidden states of the packed forward, bit for bit, and the same K/V in its caches
    with torch.inference_mode():
        ip2 = InferenceParams(max_sequence_len=capacity, max_batch_size=BATCH + 2, batch_size_offset=b0)
        a = t.gpt2_model(packed, cu_seqlens=cu, max_seqlen=longest)
        b = t.gpt2_model(packed, inference_params=ip2, cu_seqlens=cu, max_seqlen=longest)
    assert _same_bits(a, b)
    for i, c in enumerate(layers):
        assert _same_bits(ip2.key_value_memory_dict[i], c)


def test_a_packed_call_behind_the_prompt_is_refused(case):
    model, ids, _, _ = case
    packed, cu, longest = pack(ids, LENGTHS)
    ip = InferenceParams(max_sequence_len=WIDTH, max_batch_size=BATCH)
    with torch.inference_mode():
        model(packed, inference_params=ip, cu_seqlens=cu, max_seqlen=longest)
        ip.sequence_len_offset = S
        for call in (model, model.transformer, model.transformer.gpt2_model):
            with pytest.raises(ValueError, match='sequence_len_offset'):
                call(packed, inference_params=ip, cu_seqlens=cu, max_seqlen=longest)


# ---- the picks ---------------------------------------------------------------------------------------------------------------------

def test_every_pick_against_the_restatement_on_teacher_forced_logits(case):
    """The teacher-forced run makes the calls of the loop itself (same kernels, same shapes, no atomics): its logits are the
    loop's bit for bit -- two such runs are, and the first of them is what the loop returned as `scores`.  A greedy pick is the
    argmax of those logits where the two largest differ, else it holds the largest value; a draw is held to the contract of
    the pick through tests/pick_lim_ref.py with the row's own begin.
    Seen with MODEL_SEED / IDS_SEED of this file: 0 of 36 greedy picks undecided (the cap of 5 % allows one); with the seeds
    4 / 3 of tests/test_gpu_packed_forward.py it was 2 of 36, which is why this file has its own."""
    model, ids, free, first = case
    vocab = model.lm_head.weight.shape[0]
    again, _ = packed_loop_logits(model, ids, LENGTHS, free.sequences, N)
    assert _same_bits(first, again), 'two teacher-forced runs differ: the hardware is not repeatable here'
    assert _same_bits(first[0], free.scores[0])
    assert free.sequences.shape == (BATCH, WIDTH) and free.lengths.tolist() == [n + N for n in LENGTHS]
    drawn = model.sample(ids, MAX_LENGTH, kv_cache=True, cg=True, prompt_lengths=LENGTHS, packed_prefill=True,
                         rng_state=_state(), **DRAW)
    ld, _ = packed_loop_logits(model, ids, LENGTHS, drawn, N)
    lg, ld = first.float().cpu().numpy(), ld.float().cpu().numpy()
    rows_g, rows_d = free.sequences.cpu().numpy(), drawn.cpu().numpy()
    eps = R.epsilon(vocab)
    limits = {k: v for k, v in DRAW.items() if k in ('repetition_penalty', 'no_repeat_ngram_size')}
    undecided = picks = 0
    for b, begin in enumerate(LENGTHS):
        assert (rows_g[b, :begin] == ids[b, :begin].cpu().numpy()).all() and (rows_g[b, begin + N:] == 0).all()
        for i in range(N):
            t = begin + i
            v = lg[i, b]
            top2 = np.sort(v)[-2:]
            picks += 1
            if top2[1] > top2[0]:
                assert int(rows_g[b, t]) == int(np.argmax(v)), (b, t)
            else:
                undecided += 1
                assert v[int(rows_g[b, t])] == top2[1], (b, t)
            z = L.values(ld[i, b], DRAW['temperature'], rows_d[b], t, vocab, penalty_begin=begin, **limits)
            R.assert_draw(int(rows_d[b, t]), z, R.kept_set(z, DRAW['top_k'], 1.0), R.uniform(SEED, OFFSET, b, t), eps, what=(b, t))
    print(f'{undecided} of {picks} greedy picks undecided')
    assert picks == BATCH * N and undecided <= 0.05 * picks, f'{undecided} of {picks} greedy picks undecided'


def _eager16_twin(model):
    """The eager op sequence (use_flash_attn=False, no fused layer) in the model's own 16-bit type with the same weights: the
    yardstick of the whole-model rule (as tests/test_gpu_ragged_prompts.py builds it)."""
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    kw = {k: v for k, v in model.config.to_dict().items() if k in ('n_embd', 'n_head', 'n_layer', 'num_content_vectors',
                                                                   'vocab_size', 'n_positions')}
    twin = BackpackLMHeadModel(BackpackConfig(scale_attn_by_inverse_layer_idx=True, use_flash_attn=False, **kw))
    twin.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    return twin.to(device=DEV, dtype=model.lm_head.weight.dtype).eval()


@pytest.mark.parametrize('mode', ['cached', 'off'])
def test_the_loops_logits_against_the_uncached_forward_of_every_rows_own_sequence(case, mode):
    """The project's whole-model rule (tests/test_gpu_configs.py): the error against the fp32 twin is at
    most 3 x the error of the 16-bit eager twin on the same input (+ 1e-3, as there).  From the second logits on, every
    value comes out of the caches the packed prefill filled: a key in the wrong slot or a wrong length shows here.  'off':
    the content form of the Backpack's caches."""
    model, ids, free, logits = case
    t = model.transformer
    if mode != 'cached':
        keep = t.sense_table_mode
        try:
            t.sense_table_mode = mode
            logits, ip = packed_loop_logits(model, ids, LENGTHS, free.sequences, N)
        finally:
            t.sense_table_mode = keep
        assert 'backpack_content' in ip.key_value_memory_dict
    twin, eager = _fp32_twin(model), _eager16_twin(model)
    with torch.inference_mode():
        for b, begin in enumerate(LENGTHS):
            row = free.sequences[b:b + 1, :begin + N - 1]                          # unpadded: the prompt and what was fed back
            ref = twin(row).logits[0, begin - 1:].float()
            base = (eager(row).logits[0, begin - 1:].float() - ref).abs().max().item()
            err = (logits[:, b].float() - ref).abs().max().item()
            print(f'{mode} row {b} (prompt {begin}): loop {err:.3e} eager-16-bit {base:.3e} (|ref| max {ref.abs().max().item():.2f})')
            assert err <= 3 * base + 1e-3, (mode, b, err, base)


# ---- the loop ----------------------------------------------------------------------------------------------------------------------

def test_eager_equals_captured(case):
    model, ids, free, _ = case
    for call, more in ((model.generate, {}), (model.sample, dict(rng_state=_state(), **DRAW))):
        eager = call(ids, MAX_LENGTH, kv_cache=True, prompt_lengths=LENGTHS, packed_prefill=True, return_dict_in_generate=True,
                     **more)
        graph = call(ids, MAX_LENGTH, kv_cache=True, cg=True, prompt_lengths=torch.tensor(LENGTHS, device=DEV),
                     packed_prefill=True, return_dict_in_generate=True, **more)
        assert torch.equal(eager.sequences, graph.sequences) and torch.equal(eager.lengths, graph.lengths), more
        if not more:
            assert torch.equal(eager.sequences, free.sequences)


def test_pad_columns_and_pad_id_do_not_matter(case):
    model, ids, free, _ = case
    dirty = ids.clone()
    for b, begin in enumerate(LENGTHS):
        dirty[b, begin:] = torch.randint(0, VOCAB, (S - begin,), generator=torch.Generator().manual_seed(b)).to(DEV)
    assert not torch.equal(dirty, ids)
    kw = dict(kv_cache=True, prompt_lengths=LENGTHS, packed_prefill=True)
    assert torch.equal(model.generate(dirty, MAX_LENGTH, **kw), free.sequences)
    more = dict(rng_state=_state(), **DRAW)
    assert torch.equal(model.sample(dirty, MAX_LENGTH, **kw, **more), model.sample(ids, MAX_LENGTH, **kw, **more))
    a, b = (model.generate(dirty, MAX_LENGTH, pad_token_id=p, **kw) for p in (3, 7))
    for r, begin in enumerate(LENGTHS):
        assert torch.equal(a[r, :begin + N], b[r, :begin + N]) and torch.equal(a[r, :begin + N], free.sequences[r, :begin + N])
        assert (a[r, begin + N:] == 3).all() and (b[r, begin + N:] == 7).all()


def test_rows_end_at_their_eos(case):
    model, ids, free, _ = case
    seq = free.sequences
    eos = int(seq[1, LENGTHS[1] + 2])                   # ends the second row early, and whichever rows hold it too
    want = G.ends(seq.cpu(), LENGTHS, N, eos)
    assert want[1] <= LENGTHS[1] + 3 and len(set(w - n for w, n in zip(want, LENGTHS))) > 1
    for cg in (False, True):
        out = model.generate(ids, MAX_LENGTH, kv_cache=True, cg=cg, prompt_lengths=LENGTHS, packed_prefill=True, eos_token_id=eos,
                             pad_token_id=9, stop_check_every=1, return_dict_in_generate=True)
        assert out.lengths.tolist() == want and out.sequences.shape == (BATCH, max(want))
        for b in range(BATCH):
            assert torch.equal(out.sequences[b, :want[b]], seq[b, :want[b]]) and (out.sequences[b, want[b]:] == 9).all()


def test_the_record_of_the_picks_is_aligned_with_the_sequences(case):
    """Entry [b, c] of the record describes sequences[b, c] under the logits it was picked from -- the teacher-forced ones.
    Ranks and the top ids are integer functions of those bits: exact.  A log-probability is x - lse in fp32: within twice
    the bound of tests/pick_ref.py on an fp32 mass sum of the vocabulary, plus an fp32 rounding at the logits' magnitude."""
    model, ids, free, logits = case
    out = model.generate(ids, MAX_LENGTH, kv_cache=True, cg=True, prompt_lengths=LENGTHS, packed_prefill=True,
                         return_dict_in_generate=True, output_logprobs=True, top_logprobs=3)
    assert torch.equal(out.sequences, free.sequences) and torch.equal(out.lengths, free.lengths)
    x = logits.float().cpu().numpy().astype(np.float64)                     # (N, batch, vocab)
    seq = out.sequences.cpu().numpy()
    logprobs, ranks = out.token_logprobs.cpu().numpy(), out.token_ranks.cpu().numpy()
    top_ids, top_lp = out.top_token_ids.cpu().numpy(), out.top_token_logprobs.cpu().numpy()
    assert logprobs.shape == ranks.shape == (BATCH, WIDTH) and top_ids.shape == top_lp.shape == (BATCH, WIDTH, 3)
    vocab = x.shape[-1]
    bound = 2 * R.epsilon(vocab) + 2.0 ** -23 * np.abs(x).max() * 4
    for b, begin in enumerate(LENGTHS):
        outside = np.r_[0:begin, begin + N:WIDTH]
        assert (logprobs[b, outside] == 0).all() and (ranks[b, outside] == -1).all()
        assert (top_ids[b, outside] == -1).all() and (top_lp[b, outside] == 0).all()
        for i in range(N):
            c, row = begin + i, x[i, b]
            lse = row.max() + np.log(np.exp(row - row.max()).sum())
            token = int(seq[b, c])
            assert abs(logprobs[b, c] - (row[token] - lse)) <= bound, (b, c)
            assert ranks[b, c] == int((row > row[token]).sum() + ((row == row[token]) & (np.arange(vocab) < token)).sum()), (b, c)
            order = np.lexsort((np.arange(vocab), -row))[:3]
            assert top_ids[b, c].tolist() == order.tolist(), (b, c)
            assert np.abs(top_lp[b, c] - (row[order] - lse)).max() <= bound, (b, c)


# ---- models that run the padded prefill ------------------------------------------------------------------------------------------

def test_wide_senses_run_the_padded_prefill_with_one_warning():
    model = _model('mini_k4', seed=5)
    ids = padded_ids(VOCAB, DEV, seed=6)
    kw = dict(kv_cache=True, prompt_lengths=LENGTHS, return_dict_in_generate=True, output_scores=True)
    want = model.generate(ids, MAX_LENGTH, **kw)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        got = model.generate(ids, MAX_LENGTH, packed_prefill=True, **kw)
    said = [str(w.message) for w in caught if 'packed_prefill' in str(w.message)]
    assert len(said) == 1 and '> 128' in said[0], said
    with warnings.catch_warnings(record=True) as later:
        warnings.simplefilter('always')
        again = model.generate(ids, MAX_LENGTH, packed_prefill=True, cg=True, **kw)
        drawn = model.sample(ids, MAX_LENGTH, packed_prefill=True, rng_state=_state(), **DRAW, **kw)
    assert not any('packed_prefill' in str(w.message) for w in later)     # said once per model
    for out in (got, again):
        assert torch.equal(out.sequences, want.sequences) and torch.equal(out.lengths, want.lengths)
        assert _same_bits(out.scores[0], want.scores[0])
    ref = model.sample(ids, MAX_LENGTH, rng_state=_state(), **DRAW, **kw)
    assert torch.equal(drawn.sequences, ref.sequences) and _same_bits(drawn.scores[0], ref.scores[0])
