"""CPU: scoring text (src/utils/scoring.py) -- the torch twin of bp_score_rows against the float64 restatement of
tests/score_ref.py (ranks and top1 exactly, on rows with thousands of ties, -inf entries, NaNs and targets outside the row), the
refusals of the C ABI without a device, and every function of the layer on the nano model with use_flash_attn=False: against
log_softmax of the model's own logits, against lm_loss_chunked, and on hand-built cases whose answer is known.

The twin's bound, in the units of tests/score_ref.py: an exponential carries a relative error of (|x - m| / 2 + 1) eps (the
rounded difference, a 1-ulp exp); only terms within ~20 of the maximum weigh anything, so <= 11 eps; the pairwise fp32 sum over
50 264 terms adds <= 8 eps: 19 eps relative on s and absolute on log s, under one unit = eps (|lse| + max |x|) >= 19 eps wherever
|lse| + max|x| >= 19 (vocabulary rows) and within TWIN_BOUND = 4 units on the narrow rows drawn here; the entropy adds twice
that on sum p x, which its unit's factor (1 + sum p |x|) absorbs."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

import bp_hip
import score_ref as R
from oracle import ref_cpu as O
from src.models.backpack import BackpackConfig, BackpackLMHeadModel
from src.models.intervened_models import (NegativeWeightedBackpackLMHeadModel, ScaledSenseLMHeadModel,
                                          WeightedBackpackLMHeadModel)
from src.utils import scoring as S
from src.utils.perplexity import lm_loss_chunked

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
TWIN_BOUND = 4.0


def _assert_matches(got, want, x64, tag):
    for name in ('rank', 'top1'):
        assert np.array_equal(got[name].numpy().astype(np.int64), want[name]), f'{tag}: {name}'
    assert got['rank'].dtype == torch.int32 and got['top1'].dtype == torch.int32 and got['lse'].dtype == torch.float32
    worst = R.worst_errors({n: got[n].numpy() for n in ('lse', 'logprob', 'entropy')}, want, x64)
    print(f'{tag}: twin error in units: ' + ', '.join(f'{n} {v:.3f}' for n, v in worst.items()))
    assert max(worst.values()) <= TWIN_BOUND, (tag, worst)
    outside = want['rank'] < 0
    assert (got['logprob'].numpy()[outside] == 0).all() and (got['rank'].numpy()[outside] == -1).all()


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('cols,m', [(1, 1), (7, 2), (96, 1), (2049, 8), (50264, 1), (50264, 3)])
def test_the_twin_agrees_with_the_float64_restatement(cols, m, dtype):
    rows = 5 if cols > 10000 else 19
    x = torch.from_numpy(R.drawn_rows(rows, cols, seed=cols + m, minus_inf=0.1 if cols > 7 else 0.0)).to(DTYPES[dtype])
    targets = R.drawn_targets(rows, cols, m, seed=cols * 10 + m)
    if cols > 7:
        x[1, : cols // 2] = x[1, 0]                               # a run of ties, the target among them
        targets[1, 0] = cols // 4
    x64 = x.double().numpy()
    if dtype != 'fp32' and cols == 50264:
        assert len(np.unique(x64[0])) < cols // 4                 # 16-bit rows tie constantly
    want = R.score_rows(x64, targets if m > 1 else targets[:, 0])
    got = S._eager_score_rows(x, torch.from_numpy(targets if m > 1 else targets[:, 0]))
    assert sorted(got) == sorted(R.OUTPUTS) and got['logprob'].shape == want['logprob'].shape
    _assert_matches(got, want, x64, f'{dtype} {rows}x{cols} M={m}')
    assert np.isfinite(want['entropy']).all()                     # -inf entries contribute 0, not a NaN
    some = S._eager_score_rows(x, torch.from_numpy(targets), want=('rank', 'entropy'))
    assert sorted(some) == ['entropy', 'rank'] and torch.equal(some['entropy'], got['entropy'])


def test_degenerate_rows_follow_the_written_rule():
    x = torch.from_numpy(R.drawn_rows(6, 40, seed=3))
    x[0, 7] = math.nan
    x[0, 30] = math.nan                                           # the first NaN is the greedy token
    x[1, 5] = math.inf
    x[1, 9] = math.inf
    x[2] = -math.inf
    x[3, 11] = math.nan
    x[3, 2] = math.inf                                            # NaN beats +inf
    x[4, 20] = -0.0
    x[4, 3] = 0.0
    x[4, (x[4] > 0)] = -1.0                                       # the maximum is a zero: -0 == +0, the lower index wins
    targets = torch.tensor([[7, 1], [5, 1], [0, 39], [11, 2], [20, 3], [-100, 40]])
    got = S._eager_score_rows(x, targets)
    want = R.score_rows(x.numpy(), targets.numpy())
    assert np.array_equal(got['rank'].numpy(), want['rank']) and np.array_equal(got['top1'].numpy(), want['top1'])
    assert got['top1'].tolist()[:5] == [7, 5, 0, 11, 3]
    assert got['rank'][0, 0] == 0 and got['rank'][3, 0] == 0      # the rank of a NaN target is 0
    assert got['rank'][4].tolist() == [1, 0]                      # -0 == +0, the lower id precedes
    assert got['rank'][5].tolist() == [-1, -1] and got['logprob'][5].tolist() == [0.0, 0.0]
    for name in ('lse', 'entropy', 'logprob'):
        a, b = got[name].numpy().astype(np.float64), want[name]
        assert np.array_equal(np.isnan(a), np.isnan(b)), name
        assert np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(np.sign(a[np.isinf(a)]), np.sign(b[np.isinf(b)])), name
    assert torch.isnan(got['lse'][0]) and torch.isnan(got['entropy'][0]) and torch.isnan(got['logprob'][0]).all()
    assert got['lse'][1] == math.inf and torch.isnan(got['entropy'][1])
    assert torch.isnan(got['logprob'][1, 0]) and got['logprob'][1, 1] == -math.inf
    assert got['lse'][2] == -math.inf and torch.isnan(got['entropy'][2]) and torch.isnan(got['logprob'][2]).all()


def test_spike_rows_are_exact_in_the_twin():
    cols = 2049
    x, spikes = R.spike_rows(9, cols, R.boundary_columns(cols, 3, 8))
    targets = np.stack([spikes, (spikes + 5) % cols, np.full_like(spikes, 2), np.full_like(spikes, -100)], axis=1)
    got = S._eager_score_rows(torch.from_numpy(x).bfloat16(), torch.from_numpy(targets))
    want = R.spike_expected(spikes, targets, cols)
    for name in R.OUTPUTS:
        assert np.array_equal(got[name].numpy(), want[name]), name
    ref = R.score_rows(x, targets)
    assert np.array_equal(ref['rank'], want['rank']) and np.array_equal(ref['top1'], want['top1'])


def test_c_abi_refuses_bad_arguments_before_any_launch():
    h = bp_hip.lib()
    assert h.bp_abi_version() == 11 and bp_hip.ABI_VERSION == 11
    p, null = ctypes.c_void_p(0x1000), None                       # never dereferenced: validation fails first

    def call(logits=p, targets=p, outs=(p, p, p, p, p), rows=4, cols=96, m=1, row_stride=96, t_stride=None, o_stride=None,
             dtype=1):
        return h.bp_score_rows(logits, targets, *outs, rows, cols, m, row_stride, m if t_stride is None else t_stride,
                               m if o_stride is None else o_stride, dtype, null)

    assert call(dtype=3) == -1 and call(dtype=-1) == -1
    assert call(rows=0) == -3 and call(rows=-1) == -3 and call(rows=2 ** 31) == -3
    assert call(cols=0) == -3 and call(cols=-5) == -3 and call(cols=2 ** 31 - 16, row_stride=2 ** 31) == -3
    assert call(row_stride=95) == -3
    assert call(m=0) == -3 and call(m=9) == -3 and call(m=-1) == -3
    assert call(m=4, t_stride=3) == -3 and call(m=4, o_stride=3) == -3
    assert call(logits=null) == -3 and call(targets=null) == -3
    assert call(outs=(null,) * 5) == -3
    assert call(logits=ctypes.c_void_p(0x1001)) == -3 and call(logits=ctypes.c_void_p(0x1002), dtype=2) == -3
    assert call(targets=ctypes.c_void_p(0x1004)) == -3
    assert call(outs=(null, null, ctypes.c_void_p(0x1002), null, null)) == -3
    assert bp_hip.SCORE_MAX_TARGETS == 8 and bp_hip.SCORE_OUTPUTS == R.OUTPUTS
    x = torch.zeros(4, 96)
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.score_rows(x, torch.zeros(4, dtype=torch.int64))


# ---- the layer on the nano model -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def nano():
    g = load_golden('g4_nano_model.npz')
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('sd/')}
    cfg = BackpackConfig(n_embd=64, n_head=2, n_layer=2, num_content_vectors=4, vocab_size=96, n_positions=32,
                         scale_attn_by_inverse_layer_idx=True, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
                         use_flash_attn=False, pad_vocab_size_multiple=8)
    model = BackpackLMHeadModel(cfg)
    model.load_state_dict(sd)
    model.eval()
    with torch.no_grad():
        model.transformer.contextualization_attn.Wqkv.weight.mul_(8.0)   # default init: near-uniform attention
        model.lm_head.weight.mul_(40.0)                                  # and near-uniform predictions
    ids = torch.randint(0, 96, (3, 24), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        logp = torch.log_softmax(model(ids).logits.float(), dim=-1)
    ocfg = dict(n_embd=64, n_head=2, n_layer=2, num_content_vectors=4, layer_norm_epsilon=float(g['layer_norm_epsilon']),
                scale_attn_by_inverse_layer_idx=True)
    return model, ids, logp, ocfg


def test_score_tokens_is_log_softmax_gathered(nano):
    model, ids, logp, _ = nano
    got = S.score_tokens(model, ids)
    assert all(t.shape == ids.shape for t in got)
    assert got.mask[:, :-1].all() and not got.mask[:, -1].any()
    want = logp[:, :-1].gather(2, ids[:, 1:, None]).squeeze(2)
    torch.testing.assert_close(got.logprobs[:, :-1], want, rtol=1e-5, atol=2e-6)
    assert torch.equal(got.top1[:, :-1], logp[:, :-1].argmax(-1).int())
    ref = R.score_rows(logp[:, :-1].reshape(-1, 96).numpy(), ids[:, 1:].reshape(-1).numpy())
    assert np.array_equal(got.ranks[:, :-1].reshape(-1).numpy(), ref['rank'])
    torch.testing.assert_close(got.entropy[:, :-1], -(logp.exp() * logp).sum(-1)[:, :-1], rtol=1e-4, atol=1e-5)
    assert (got.logprobs[:, -1] == 0).all() and (got.entropy[:, -1] == 0).all() and (got.lse[:, -1] == 0).all()
    assert (got.ranks[:, -1] == -1).all() and (got.top1[:, -1] == -1).all()
    assert 0 < (got.ranks == 0).sum() < got.mask.sum()            # the sharpened model is right sometimes, not always
    for chunk in (1, 7, 1000):                                    # chunking changes nothing (same rows through the same GEMV)
        again = S.score_tokens(model, ids, chunk_tokens=chunk)
        torch.testing.assert_close(again.logprobs, got.logprobs, rtol=1e-6, atol=1e-6)
        assert torch.equal(again.ranks, got.ranks) and torch.equal(again.top1, got.top1)
    labels = torch.full_like(ids, -100)
    labels[0, 3], labels[2, 23] = 5, 96                           # an explicit label; one outside the vocabulary
    few = S.score_tokens(model, ids, labels=labels)
    assert few.mask.sum() == 2 and few.logprobs[0, 3] == logp[0, 3, 5] - 0 and few.ranks[2, 23] == -1 and few.logprobs[2, 23] == 0
    part = S.score_tokens(model, ids, want=('rank',))
    assert part.logprobs is None and torch.equal(part.ranks, got.ranks)


def test_evaluate_lm_agrees_with_lm_loss_chunked(nano):
    model, ids, logp, _ = nano
    loss, count = lm_loss_chunked(model, ids)
    got = S.evaluate_lm(model, [ids])
    assert got['tokens'] == count == 3 * 23
    assert abs(got['loss'] - float(loss)) <= 1e-5 * abs(float(loss))
    assert abs(got['perplexity'] - math.exp(got['loss'])) <= 1e-12 * got['perplexity']
    scores = S.score_tokens(model, ids)
    assert got['accuracy'] == float(((scores.ranks == 0) & scores.mask).sum()) / count
    # two batches: sums, not a mean of means; a batch as a tuple with labels and as a dict
    more = torch.randint(0, 96, (1, 9), generator=torch.Generator().manual_seed(1))
    both = S.evaluate_lm(model, [(ids, None), {'input_ids': more}])
    l2, c2 = lm_loss_chunked(model, more)
    want = (float(loss) * count + float(l2) * c2) / (count + c2)
    assert both['tokens'] == count + c2 and abs(both['loss'] - want) <= 1e-5 * want
    assert math.isnan(S.evaluate_lm(model, [])['loss'])


def test_lengths_mask_and_pads_do_not_matter(nano):
    model, ids, logp, _ = nano
    lengths = torch.tensor([24, 10, 1])
    got = S.score_tokens(model, ids, lengths=lengths)
    pos = torch.arange(24)
    assert torch.equal(got.mask, pos[None, :] < (lengths[:, None] - 1))
    full = S.score_tokens(model, ids)
    assert torch.equal(got.logprobs[got.mask], full.logprobs[got.mask])
    assert (got.logprobs[~got.mask] == 0).all() and (got.ranks[~got.mask] == -1).all()
    changed = ids.clone()
    changed[1, 10:] = 7
    changed[2, 1:] = 0                                            # pads replaced: nothing moves
    again = S.score_tokens(model, changed, lengths=lengths)
    for a, b in zip(again, got):
        assert torch.equal(a, b)


def test_sequence_scores_with_a_prefix_is_the_slice_sum(nano):
    model, ids, logp, _ = nano
    lengths, prefix = torch.tensor([24, 10, 5]), torch.tensor([0, 4, 5])
    got = S.sequence_scores(model, ids, lengths=lengths, prefix_lengths=prefix)
    full = S.score_tokens(model, ids)
    for b in range(3):
        first = max(int(prefix[b]), 1)                            # token j is scored at position j - 1
        sl = slice(first - 1, int(lengths[b]) - 1)
        assert got.count[b] == int(lengths[b]) - first
        assert abs(float(got.logprob[b]) - float(full.logprobs[b, sl].double().sum())) < 1e-12
        assert bool(got.all_top1[b]) == bool((full.ranks[b, sl] == 0).all())
    assert got.logprob.dtype == torch.float64 and got.count[2] == 0 and got.logprob[2] == 0 and got.all_top1[2]


def _greedy_continuation(model, context, n):
    seq = list(context)
    for _ in range(n):
        with torch.no_grad():
            seq.append(int(model(torch.tensor([seq])).logits[0, -1].argmax()))
    return seq[len(context):]


def test_last_word_pairs_and_choices_on_known_answers(nano):
    model, ids, logp, _ = nano
    contexts = [ids[0, :6].tolist(), ids[1, :11].tolist(), ids[2, :3].tolist()]
    greedy = [_greedy_continuation(model, c, 2) for c in contexts]
    wrong = [[(g[0] + 1) % 96, g[1]] for g in greedy]
    assert S.last_word_eval(model, list(zip(contexts, greedy)))['accuracy'] == 1.0
    assert S.last_word_eval(model, list(zip(contexts, wrong)))['accuracy'] == 0.0
    mixed = S.last_word_eval(model, [(contexts[0], greedy[0]), (contexts[1], wrong[1]), (contexts[2], greedy[2])], batch_size=2)
    assert mixed['accuracy'] == pytest.approx(2 / 3) and mixed['examples'] == 3 and mixed['tokens'] == 6
    # its perplexity is exp(-mean log-prob of the target tokens), from the model's own log_softmax
    total = 0.0
    for c, t in ((contexts[0], greedy[0]), (contexts[1], wrong[1]), (contexts[2], greedy[2])):
        with torch.no_grad():
            lp = torch.log_softmax(model(torch.tensor([c + t])).logits[0].double(), dim=-1)
        total += sum(float(lp[len(c) - 1 + i, tok]) for i, tok in enumerate(t))
    assert mixed['perplexity'] == pytest.approx(math.exp(-total / 6), rel=1e-5)
    with pytest.raises(ValueError):
        S.last_word_eval(model, [([], [1])])

    # minimal pairs: the greedy continuation beats the same context with another last token
    good = [c + g for c, g in zip(contexts, greedy)]
    bad = [c + [g[0], (g[1] + 1) % 96] for c, g in zip(contexts, greedy)]
    res = S.pair_accuracy(model, good, bad)
    assert res['accuracy'] == 1.0 and (res['good'] > res['bad']).all() and res['good'].dtype == torch.float64
    assert S.pair_accuracy(model, bad, good)['accuracy'] == 0.0
    assert S.pair_accuracy(model, good[:2] + bad[2:], bad[:2] + good[2:])['accuracy'] == pytest.approx(2 / 3)

    # multiple choice: one-token choices are ordered as the next-token distribution orders them
    ctx = contexts[1]
    with torch.no_grad():
        nxt = torch.log_softmax(model(torch.tensor([ctx])).logits[0, -1].double(), dim=-1)
    choices = [[5], [17], [int(nxt.argmax())], [60]]
    order, scores = S.rank_choices(model, ctx, choices)
    assert order[0] == 2 and order.tolist() == torch.sort(nxt[[5, 17, int(nxt.argmax()), 60]], descending=True).indices.tolist()
    torch.testing.assert_close(scores, nxt[[5, 17, int(nxt.argmax()), 60]], rtol=1e-5, atol=1e-6)
    # normalisation: a long choice pays per token
    long_choice = greedy[1] + _greedy_continuation(model, ctx + greedy[1], 2)
    _, raw = S.rank_choices(model, ctx, [greedy[1][:1], long_choice])
    _, norm = S.rank_choices(model, ctx, [greedy[1][:1], long_choice], normalize=True)
    assert norm[0] == raw[0] and norm[1] == pytest.approx(float(raw[1]) / 4, rel=1e-12) and raw[1] < raw[0]


def test_candidate_probs_and_bias_ratio_are_the_softmax_formula(nano):
    model, ids, logp, _ = nano
    places = [(0, 3), (2, 23), (1, 0), (1, 0)]
    cand = torch.tensor([[4, 9, 4, 95, 0, 50, 51, 52]] * 4)
    lp, rank = S.candidate_probs(model, ids, places, cand)
    assert lp.shape == (4, 8) and lp.dtype == torch.float32 and rank.dtype == torch.int32
    want = torch.stack([logp[b, s] for b, s in places])
    torch.testing.assert_close(lp, want.gather(1, cand), rtol=1e-5, atol=2e-6)
    assert np.array_equal(rank.numpy(), R.score_rows(want.numpy(), cand.numpy())['rank'])
    shared, _ = S.candidate_probs(model, ids, places, [4, 9])
    assert torch.equal(shared, lp[:, :2])
    with pytest.raises(ValueError):
        S.candidate_probs(model, ids, places, list(range(9)))
    ratio = S.bias_ratio(model, ids, places, 4, 9)
    p = want.double().exp()
    torch.testing.assert_close(ratio, torch.maximum(p[:, 4] / p[:, 9], p[:, 9] / p[:, 4]), rtol=1e-5, atol=0)
    assert (ratio >= 1).all()


@pytest.mark.parametrize('percent', [0.0, 0.5, 1.0])
def test_scaled_sense_is_the_alpha_column_scaling_of_the_oracle(nano, percent):
    model, ids, logp, ocfg = nano
    words, sense = [int(ids[0, 2]), int(ids[1, 5]), 95], 2
    wrapped = ScaledSenseLMHeadModel(model, words, sense, percent)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    st = O.backpack_forward(sd, ocfg, ids, return_stages=True)
    alpha = st['alpha'].clone()
    hit = torch.isin(ids, torch.tensor(words))
    assert hit.sum() >= 2
    for b, j in hit.nonzero().tolist():
        alpha[b, sense, :, j] *= percent                          # compute_counterfactual, test_genderbias.py:71-78
    want = torch.sum(alpha @ st['content'], dim=1) @ sd['lm_head.weight'].t()
    with torch.no_grad():
        got = wrapped(ids).logits
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    if percent == 1.0:
        with torch.no_grad():
            torch.testing.assert_close(got, model(ids).logits, rtol=1e-6, atol=1e-6)
    else:
        assert (got - model(ids).logits).abs().max() > 1e-3
    # the scoring layer goes through the wrapper's own hidden states
    scores = S.score_tokens(wrapped, ids)
    lp = torch.log_softmax(got.float(), dim=-1)[:, :-1].gather(2, ids[:, 1:, None]).squeeze(2)
    torch.testing.assert_close(scores.logprobs[:, :-1], lp, rtol=1e-5, atol=2e-6)
    with pytest.raises(NotImplementedError):
        wrapped(ids, inference_params=object())
    with pytest.raises(ValueError):
        ScaledSenseLMHeadModel(model, words, 4, percent)


def test_wrappers_go_through_their_own_hidden_states(nano):
    model, ids, logp, _ = nano
    cw = torch.rand(96, 4, generator=torch.Generator().manual_seed(2)) * 2
    weighted = WeightedBackpackLMHeadModel(model, cw, None, 0.1, anneal=False)
    with torch.no_grad():
        lp = torch.log_softmax(weighted(ids).logits.float(), dim=-1)[:, :-1].gather(2, ids[:, 1:, None]).squeeze(2)
    torch.testing.assert_close(S.score_tokens(weighted, ids).logprobs[:, :-1], lp, rtol=1e-5, atol=2e-6)
    with pytest.raises(NotImplementedError):
        S.score_tokens(NegativeWeightedBackpackLMHeadModel(model, cw, None, 0.1, anneal=False), ids)
    with pytest.raises(TypeError):
        S.score_tokens(torch.nn.Linear(2, 2), ids)


# ---- the code object ---------------------------------------------------------------------------------------------------------------

def test_no_instantiation_of_the_kernel_touches_scratch():
    """All six instantiations (three element types, M = 1 and the general form): no spilled register, no scratch, and
    registers that leave a workgroup's four waves room for at least four more per SIMD."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_resources as KR
    if not KR.tools_available():
        pytest.skip('llvm-objcopy / clang-offload-bundler / llvm-readelf not found under /opt/rocm')
    obj = os.path.join(KR.BUILD, 'score_rows.o')
    if not os.path.exists(obj):                                   # the library was built elsewhere: compile the objects here
        import importlib.util
        spec = importlib.util.spec_from_file_location('bp_build_hip', os.path.join(ROOT, 'backpacks-flash-attn_amd', 'build_hip.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(force=True)
    found = {k['name']: k for k in KR.kernels([obj])}
    names = [f'score_rows_kernel<{et}, {m}>' for et in ('BF16', 'F16', 'float') for m in (1, 8)]
    assert sorted(found) == sorted(names)
    for name in names:
        k = found[name]
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, k
        assert k['waves_per_simd'] >= 4 and k['max_flat_workgroup_size'] == 256, k
