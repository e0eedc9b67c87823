"""GPU: the packed forward of BackpackModel / BackpackLMHeadModel (input_ids (total,) + cu_seqlens + max_seqlen) and
score_tokens(packed=True), on the two-layer decode models of tests/decode_support.py.

Every comparison between two runs whose GEMMs see different row counts is held to the whole-model rule of DESIGN.md section 2
(tests/test_gpu_configs.py): with `base` = the error of the 16-bit eager twin against the fp32 twin on a sequence of its own,
a HIP result may be 3 x base + 1e-3 away from the fp32 twin, and two HIP results of the same sequence that far from each
other (what differs between them is how BLAS rounds a row, the rule's own allowance).  mini_k4 (d_k = 160) has no packed
sense kernels: it pads and runs, and equals the padded forward's real rows bit for bit."""
import warnings

import pytest
import torch

from decode_support import DEV, VOCAB, _fp32_twin, _model, _same_bits
from src.utils import scoring
from src.utils.packing import pack_sequences

pytestmark = pytest.mark.gpu


def _eager16_twin(model):
    """The eager op sequence (use_flash_attn=False, no fused layer) in the model's own 16-bit type with the same weights: the
    yardstick of the whole-model rule (as tests/test_gpu_ragged_prompts.py builds it)."""
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    kw = {k: v for k, v in model.config.to_dict().items() if k in ('n_embd', 'n_head', 'n_layer', 'num_content_vectors',
                                                                   'vocab_size', 'n_positions')}
    twin = BackpackLMHeadModel(BackpackConfig(scale_attn_by_inverse_layer_idx=True, use_flash_attn=False, **kw))
    twin.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    return twin.to(device=DEV, dtype=model.lm_head.weight.dtype).eval()

LENGTHS = (1, 70, 37, 130, 64, 5)          # 307 positions; 130 > 128: two flash query tiles, 64 / 70: a key tile and a bit


def _padded_ids(seed=3):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, VOCAB, (len(LENGTHS), max(LENGTHS)), generator=g)
    for b, n in enumerate(LENGTHS):
        ids[b, n:] = 0
    return ids.to(DEV)


@pytest.fixture(scope='module')
def small():
    """The model, its ids, the packed and the padded logits, and per sequence the fp32 twin's logits and the eager error."""
    model = _model('small', seed=4)
    ids = _padded_ids()
    packed, cu, longest = pack_sequences(ids, LENGTHS)
    twin, eager = _fp32_twin(model), _eager16_twin(model)
    with torch.inference_mode():
        got = model(packed, cu_seqlens=cu, max_seqlen=longest).logits
        padded = model(ids).logits
        refs, bases = [], []
        for b, n in enumerate(LENGTHS):
            refs.append(twin(ids[b:b + 1, :n]).logits[0].float())
            bases.append((eager(ids[b:b + 1, :n]).logits[0].float() - refs[-1]).abs().max().item())
    return dict(model=model, ids=ids, packed=packed, cu=cu, longest=longest, got=got, padded=padded, refs=refs, bases=bases)


def _rule(got, want, base, what):
    err = (got.float() - want.float()).abs().max().item()
    print(f'{what}: {err:.3e} against 3 x {base:.3e} + 1e-3')
    assert err <= 3 * base + 1e-3, (what, err, base)


def test_packed_logits_against_every_sequence_on_its_own_and_the_padded_rows(small):
    s = small
    assert s['got'].shape == (sum(LENGTHS), s['padded'].shape[-1]) and torch.isfinite(s['got'].float()).all()
    cu = s['cu'].tolist()
    with torch.inference_mode():
        for b, n in enumerate(LENGTHS):
            rows = s['got'][cu[b]:cu[b + 1]]
            _rule(rows, s['refs'][b], s['bases'][b], f'packed vs fp32 twin, sequence {b} ({n})')
            _rule(rows, s['padded'][b, :n], s['bases'][b], f'packed vs padded rows, sequence {b} ({n})')
            alone = s['model'](s['ids'][b:b + 1, :n]).logits[0]
            _rule(rows, alone, s['bases'][b], f'packed vs the uncached forward of sequence {b} ({n}) alone')
        out = torch.empty_like(s['got'])
        assert s['model'](s['packed'], cu_seqlens=s['cu'], max_seqlen=s['longest'], logits_out=out).logits is out
        assert _same_bits(out, s['got'])


def test_the_three_sense_table_modes_agree(small):
    s = small
    t = s['model'].transformer
    cu, results = s['cu'].tolist(), {}
    import bp_hip
    keep = (t.sense_table_mode, t.dedup_min_positions)
    entered, call = {}, bp_hip._call
    try:
        for mode in ('cached', 'batch', 'off'):
            t.sense_table_mode, t.dedup_min_positions = mode, 0
            entered[mode] = []
            bp_hip._call = lambda name, *args, names=entered[mode]: (names.append(name), call(name, *args))[1]
            with torch.inference_mode():
                results[mode] = s['model'](s['packed'], cu_seqlens=s['cu'], max_seqlen=s['longest']).logits
    finally:
        t.sense_table_mode, t.dedup_min_positions = keep
        bp_hip._call = call
    # the packed kernels ran, the padded ones did not: the table forms through the gathering mix, 'off' through the dense one
    for mode, mix in (('cached', 'bp_sense_mix_gather_varlen'), ('batch', 'bp_sense_mix_gather_varlen'), ('off', 'bp_sense_mix_varlen')):
        senses = [n for n in entered[mode] if n.startswith('bp_sense_')]
        assert senses == [mix], (mode, senses)
        assert any(n.startswith('bp_flash_fwd') for n in entered[mode])
    assert _same_bits(results[keep[0]], s['got'])
    for b, n in enumerate(LENGTHS):
        sl = slice(cu[b], cu[b + 1])
        for mode in results:
            _rule(results[mode][sl], s['refs'][b], s['bases'][b], f'{mode} vs fp32 twin, sequence {b}')
        for a, c in (('cached', 'batch'), ('cached', 'off'), ('batch', 'off')):
            _rule(results[a][sl], results[c][sl], s['bases'][b], f'{a} vs {c}, sequence {b}')


def test_wide_senses_pad_and_run_with_one_warning():
    model = _model('mini_k4', seed=5)
    ids = _padded_ids(seed=6)
    packed, cu, longest = pack_sequences(ids, LENGTHS)
    with torch.inference_mode():
        with pytest.warns(UserWarning, match='padded') as caught:
            got = model(packed, cu_seqlens=cu, max_seqlen=longest).logits
        said = [str(w.message) for w in caught if 'padded' in str(w.message)]
        assert len(said) == 1 and '> 128' in said[0], said
        with warnings.catch_warnings(record=True) as later:
            warnings.simplefilter('always')
            again = model(packed, cu_seqlens=cu, max_seqlen=longest).logits
        assert not any('padded' in str(w.message) for w in later)     # said once per model
        padded = model(ids).logits
    assert _same_bits(again, got)
    for b, n in enumerate(LENGTHS):
        assert _same_bits(got[int(cu[b]):int(cu[b + 1])], padded[b, :n].contiguous()), b


def test_score_tokens_packed_against_padded(small):
    """The bound is the whole-model rule's own, D = 3 x base + 1e-3 per sequence, the one `_rule` holds two HIP results of a
    sequence to elsewhere in this file: the log-probabilities of the two scorings lie within D of each other, and the rank and
    the greedy token are equal wherever the padded run's top-2 margin exceeds D -- a set that must not be empty.  (Both runs
    use the same kernels with the same per-sample arithmetic; what the rule allows for is how BLAS rounds a row when the row
    count changes.)  A packed scoring that read a neighbour's row would move log-probabilities by whole nats."""
    s = small
    lengths = torch.tensor(LENGTHS, device=DEV)
    a = scoring.score_tokens(s['model'], s['ids'], lengths=lengths)
    b = scoring.score_tokens(s['model'], s['ids'], lengths=lengths, packed=True)
    assert torch.equal(a.mask, b.mask) and int(a.mask.sum()) == sum(n - 1 for n in LENGTHS)
    d = (3 * torch.tensor(s['bases'], device=DEV) + 1e-3)[:, None]          # per sequence
    off = (a.logprobs - b.logprobs).abs()
    print(f'log-probs differ by {off.max().item():.3e}, bounds {d.min().item():.3e} .. {d.max().item():.3e}; '
          f'ranks equal at {int(((a.ranks == b.ranks) & a.mask).sum())}, greedy tokens at '
          f'{int(((a.top1 == b.top1) & a.mask).sum())} of {int(a.mask.sum())} scored positions')
    assert (off <= d).all()
    top2 = s['padded'].float().topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]
    decided = a.mask & (margin > d)
    print(f'{int(decided.sum())} of {int(a.mask.sum())} positions decided (largest top-2 margin {margin[a.mask].max().item():.3f})')
    assert int(decided.sum()) > 0
    assert torch.equal(a.top1[decided], b.top1[decided])
    assert torch.equal(a.ranks[decided], b.ranks[decided])
    for field in ('logprobs', 'entropy', 'lse'):
        assert (getattr(b, field)[~b.mask] == 0).all()
    assert (b.ranks[~b.mask] == -1).all() and (b.top1[~b.mask] == -1).all()
