"""GPU: the scoring layer (src/utils/scoring.py) on Small- and Mini-shaped two-layer Backpacks in bf16, HIP path.

  parity       score_tokens' log-probabilities against the fp32 eager twin of the same model, within the project's whole-model
               rule: at most 3x the error of the eager bf16 model against that twin (+ 1e-3)
  exactness    ranks, top1 and the log-probabilities against the model's OWN logits: the model runs once for (B, S, vocab)
               logits, tests/score_ref.py scores them in float64, and what score_tokens returned -- after its gather of the
               scored rows and its chunked LM head -- has the same ranks and top1, entry for entry
  chunking     chunk_tokens 7, 64 and all rows give identical outputs
  lengths      right-padded rows: the mask, the unscored values, and pads that do not matter
  wrappers     WeightedBackpackLMHeadModel and ScaledSenseLMHeadModel go through their own hidden states; candidate_probs and
               bias_ratio read the M-target kernel
"""
import warnings

import numpy as np
import pytest
import torch

import score_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SHAPES = {'small': dict(n_embd=768, n_head=12, num_content_vectors=16), 'mini_k4': dict(n_embd=640, n_head=8, num_content_vectors=4)}
VOCAB = 300                       # padded to 304 rows
B, S = 4, 32


def _build(shape, use_flash, dtype, state=None):
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    cfg = BackpackConfig(n_layer=2, vocab_size=VOCAB, n_positions=S, scale_attn_by_inverse_layer_idx=True, resid_pdrop=0.0,
                         embd_pdrop=0.0, attn_pdrop=0.0, use_flash_attn=use_flash, pad_vocab_size_multiple=8, **SHAPES[shape])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = BackpackLMHeadModel(cfg)
        if state is not None:
            model.load_state_dict(state)
        return model.to(DEV, dtype).eval()


@pytest.fixture(scope='module', params=sorted(SHAPES))
def models(request):
    """(HIP bf16 model, eager bf16 model, eager fp32 twin, ids, the HIP model's own logits): one set of bf16-exact weights."""
    import bp_hip
    bp_hip.lib()
    torch.manual_seed(11)
    hip = _build(request.param, True, torch.bfloat16)
    with torch.no_grad():         # the default init predicts near-uniformly: sharpen attention and predictions
        hip.transformer.contextualization_attn.Wqkv.weight.mul_(8.0)
        hip.lm_head.weight.mul_(6.0)
    state = {k: v.detach().float().cpu() for k, v in hip.state_dict().items()}
    eager = _build(request.param, False, torch.bfloat16, state)
    twin = _build(request.param, False, torch.float32, state)
    ids = torch.randint(0, VOCAB, (B, S), generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        logits = hip(ids).logits
    return hip, eager, twin, ids, logits


def _equal(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def test_score_tokens_follows_the_whole_model_rule(models):
    from src.utils import scoring as SC
    hip, eager, twin, ids, _ = models
    got, base, ref = SC.score_tokens(hip, ids), SC.score_tokens(eager, ids), SC.score_tokens(twin, ids)
    assert got.mask[:, :-1].all() and not got.mask[:, -1].any()
    for name in ('logprobs', 'entropy', 'lse'):
        want = getattr(ref, name)
        err = (getattr(got, name) - want).abs().max().item()
        yard = (getattr(base, name) - want).abs().max().item()
        print(f'{name}: hip {err:.3e} eager-bf16 {yard:.3e} (|ref| max {want.abs().max().item():.2f})')
        assert torch.isfinite(getattr(got, name)).all()
        assert err <= 3 * yard + 1e-3, (name, err, yard)
    assert float(ref.entropy[got.mask].min()) < float(np.log(VOCAB)) - 0.2      # the sharpened model is not uniform
    res, want = SC.evaluate_lm(hip, [ids]), SC.evaluate_lm(twin, [ids])
    from src.utils.perplexity import lm_loss_chunked
    loss, count = lm_loss_chunked(hip, ids)
    assert res['tokens'] == count == B * (S - 1) and abs(res['loss'] - float(loss)) <= 1e-5 * abs(float(loss))
    # a mean of per-token errors is at most their maximum: the bound of the log-probabilities above holds for the loss (the
    # eager model's own error of the MEAN is no yardstick: its per-token errors may cancel)
    yard = (base.logprobs - ref.logprobs).abs().max().item()
    assert abs(res['loss'] - want['loss']) <= 3 * yard + 1e-3


def test_ranks_top1_and_logprobs_are_those_of_the_models_own_logits(models):
    from src.utils import scoring as SC
    hip, _, _, ids, logits = models
    got = SC.score_tokens(hip, ids)
    x = logits[:, :-1].reshape(-1, logits.shape[-1])
    assert x.shape[1] == 304
    want = R.score_rows(x.double().cpu().numpy(), ids[:, 1:].reshape(-1).cpu().numpy())
    assert np.array_equal(got.ranks[:, :-1].reshape(-1).cpu().numpy(), want['rank'])
    assert np.array_equal(got.top1[:, :-1].reshape(-1).cpu().numpy(), want['top1'])
    worst = R.worst_errors({'logprob': got.logprobs[:, :-1].reshape(-1).cpu().numpy(), 'lse': got.lse[:, :-1].reshape(-1).cpu().numpy(),
                            'entropy': got.entropy[:, :-1].reshape(-1).cpu().numpy()}, want, x.double().cpu().numpy())
    print('against the own logits, in units: ' + ', '.join(f'{n} {v:.3f}' for n, v in worst.items()))
    import bp_hip
    direct = bp_hip.score_rows(x, ids[:, 1:].reshape(-1))     # the kernel on the model's logits: the same bits as through the layer
    assert torch.equal(direct['logprob'], got.logprobs[:, :-1].reshape(-1))
    assert torch.equal(direct['entropy'], got.entropy[:, :-1].reshape(-1)) and torch.equal(direct['lse'], got.lse[:, :-1].reshape(-1))
    assert int(got.ranks[got.mask].min()) >= 0 and len(torch.unique(got.ranks[got.mask])) > 20     # drawn labels: ranks all over


def test_chunking_changes_no_bit(models):
    from src.utils import scoring as SC
    hip, _, _, ids, _ = models
    whole = SC.score_tokens(hip, ids, chunk_tokens=B * S)
    for chunk in (7, 64):
        assert _equal(SC.score_tokens(hip, ids, chunk_tokens=chunk), whole), chunk


def test_lengths_mask_and_pads_do_not_matter(models):
    from src.utils import scoring as SC
    hip, _, _, ids, _ = models
    lengths = torch.tensor([S, 10, 1, 17], device=DEV)
    got, full = SC.score_tokens(hip, ids, lengths=lengths), SC.score_tokens(hip, ids)
    pos = torch.arange(S, device=DEV)
    assert torch.equal(got.mask, pos[None, :] < (lengths[:, None] - 1))
    assert torch.equal(got.ranks[got.mask], full.ranks[got.mask]) and torch.equal(got.top1[got.mask], full.top1[got.mask])
    assert torch.equal(got.logprobs[got.mask], full.logprobs[got.mask])
    assert (got.logprobs[~got.mask] == 0).all() and (got.entropy[~got.mask] == 0).all() and (got.lse[~got.mask] == 0).all()
    assert (got.ranks[~got.mask] == -1).all() and (got.top1[~got.mask] == -1).all()
    changed = ids.clone()
    changed[1, 10:], changed[2, 1:], changed[3, 17:] = 7, 0, 299
    assert _equal(SC.score_tokens(hip, changed, lengths=lengths), got)
    seq = SC.sequence_scores(hip, ids, lengths=lengths, prefix_lengths=torch.tensor([0, 4, 1, 17], device=DEV))
    assert seq.count.tolist() == [S - 1, 6, 0, 0]
    assert abs(float(seq.logprob[1]) - float(full.logprobs[1, 3:9].double().sum())) < 1e-9


def test_the_wrappers_and_the_candidate_readout(models):
    from src.models.intervened_models import ScaledSenseLMHeadModel, WeightedBackpackLMHeadModel
    from src.utils import scoring as SC
    hip, eager, twin, ids, logits = models
    k = hip.transformer.num_content_vectors
    cw = (torch.rand(304, k, generator=torch.Generator().manual_seed(2)) * 2).to(DEV)
    words = [int(ids[0, 2]), int(ids[1, 5])]
    for make in (lambda m: WeightedBackpackLMHeadModel(m, cw, None, 0.1, anneal=False),
                 lambda m: ScaledSenseLMHeadModel(m, words, k - 1, 0.25)):
        wrapped, ref = make(hip), make(twin)
        with torch.no_grad():
            own = wrapped(ids).logits
        got = SC.score_tokens(wrapped, ids)
        x = own[:, :-1].reshape(-1, own.shape[-1])
        want = R.score_rows(x.double().cpu().numpy(), ids[:, 1:].reshape(-1).cpu().numpy())
        assert np.array_equal(got.ranks[:, :-1].reshape(-1).cpu().numpy(), want['rank'])
        assert np.array_equal(got.top1[:, :-1].reshape(-1).cpu().numpy(), want['top1'])
        err = (got.logprobs - SC.score_tokens(ref, ids).logprobs).abs().max().item()
        yard = (SC.score_tokens(make(eager), ids).logprobs - SC.score_tokens(ref, ids).logprobs).abs().max().item()
        print(f'{type(wrapped).__name__}: hip {err:.3e} eager-bf16 {yard:.3e}')
        assert err <= 3 * yard + 1e-3
        assert not torch.equal(got.logprobs, SC.score_tokens(hip, ids).logprobs)      # the intervention does something
    same = SC.score_tokens(ScaledSenseLMHeadModel(hip, words, k - 1, 1.0), ids)
    plain = SC.score_tokens(hip, ids)
    assert (same.logprobs - plain.logprobs).abs().max().item() < 0.05     # percent = 1: the wrapped network, through the weighted kernel

    places = [(0, 3), (3, S - 1), (1, 0), (1, 0)]
    cand = torch.tensor([[4, 9, 4, 299, 0, 50, 51, 303]] * 4)
    lp, rank = SC.candidate_probs(hip, ids, places, cand)
    rows = torch.stack([logits[b, s] for b, s in places])
    want = R.score_rows(rows.double().cpu().numpy(), cand.numpy())
    assert np.array_equal(rank.cpu().numpy(), want['rank'])
    import bp_hip
    assert torch.equal(lp, bp_hip.score_rows(rows.contiguous(), cand.to(DEV))['logprob'])
    ratio = SC.bias_ratio(hip, ids, places, 4, 9)
    p = torch.softmax(rows.double(), dim=-1)
    torch.testing.assert_close(ratio, torch.maximum(p[:, 4] / p[:, 9], p[:, 9] / p[:, 4]), rtol=1e-5, atol=0)
