"""CPU: the record of a generation's picks (output_logprobs / top_logprobs).  _eager_report (src/utils/generation.py), the torch
twin of bp_pick_report, against the float64 restatement tests/pick_report_ref.py; the generation loops on the fp32 nano Backpack
against that restatement applied to the logits of every step, which a recording wrapper defined here keeps; argument checks;
and the register account of the new kernels (hipcc cross-compiles: no GPU needed).

Criteria: ranks and top ids are comparisons and must be equal.  The real-valued records must lie within TWIN_BOUND = 4 units of
tests/score_ref.py:units -- eps32 (|lse| + max |x|), times (1 + sum p |x|) for the entropy -- which is the bound
tests/test_scoring_host.py derives for the fp32 evaluation of these formulas (19 eps on s: a 1-ulp exponential of a rounded
difference plus a pairwise fp32 sum); a top log-probability is one more subtraction against that lse and takes the lse's unit.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT

import pick_report_ref as P
import score_ref as R
from decode_support import PROMPT, STEPS, _anneal_scale, _assert_scores_in_band
from decode_support import _nano_backpack as _backpack
from src.utils import generation as G
from src.utils.generation import _eager_report, greedy_decode, sample

TWIN_BOUND = 4.0
VOCAB = 200


# ---- _eager_report against the restatement ---------------------------------------------------------------------------------------

def _twin(x, tokens, counters, cols, n_top, names=P.RECORDS, canary=False):
    """_eager_report into records at their initial values (or canaries) -> dict of numpy arrays."""
    rows = x.shape[0]
    fill = {'logprob': 7.5, 'rank': 77, 'entropy': 7.5, 'top_idx': 77, 'top_logprob': 7.5} if canary else P.INITIAL
    recs = {}
    for n in names:
        if n.startswith('top_') and not n_top:
            continue
        shape = (rows, cols, n_top) if n.startswith('top_') else (rows, cols)
        recs[n] = torch.full(shape, fill[n], dtype=torch.int32 if n in ('rank', 'top_idx') else torch.float32)
    _eager_report(x, torch.as_tensor(tokens), torch.as_tensor(counters, dtype=torch.int32), **recs)
    return {n: v.numpy() for n, v in recs.items()}


def _assert_records(got, want, unit, unit_ent, tag):
    """got: fp32 / int32 records; want: the restatement's; unit, unit_ent (rows, cols): score_ref's units where a record was
    written, 0 elsewhere (there the values must be equal)."""
    for n in got:
        if n in ('rank', 'top_idx'):
            assert np.array_equal(got[n], want[n]), (tag, n)
            continue
        u = unit_ent if n == 'entropy' else unit
        u = u[:, :, None] if got[n].ndim == 3 else u
        a, b = got[n].astype(np.float64), want[n]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (tag, n, 'NaNs')
        inf = np.isinf(b)
        assert np.array_equal(np.isinf(a), inf) and np.array_equal(a[inf], b[inf]), (tag, n, 'infinities')
        real = ~np.isnan(b) & ~inf
        with np.errstate(invalid='ignore'):
            err = np.abs(np.where(real, a - b, 0.0))
        assert (err <= TWIN_BOUND * np.broadcast_to(u, err.shape)).all(), (tag, n, float(err.max()))


def _units_at(x64, counters, cols):
    rows = x64.shape[0]
    unit, unit_ent = np.zeros((rows, cols)), np.zeros((rows, cols))
    finite = np.isfinite(np.where(np.isneginf(x64), 0.0, x64)).all(axis=1) & np.isfinite(x64).any(axis=1)
    with np.errstate(all='ignore'):
        u, ue = R.units(np.where(finite[:, None], x64, 0.0))
    for b, c in enumerate(counters):
        if 0 <= c < cols and finite[b]:
            unit[b, c], unit_ent[b, c] = u[b], ue[b]
    return unit, unit_ent


def _check_rows(x, tokens, counters, cols, n_top, tag):
    x64 = x.double().numpy()
    want = P.pick_report(x64, tokens, counters, P.new_records(x.shape[0], cols, n_top))
    got = _twin(x, tokens, counters, cols, n_top)
    _assert_records(got, want, *_units_at(x64, counters, cols), tag)
    return got, want


@pytest.mark.parametrize('n_top', [0, 1, 5, 16])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_twin_equals_the_restatement_on_drawn_and_tied_rows(dtype, n_top):
    rows, vocab, cols = (12, 4099, 5) if dtype == torch.float32 else (6, 50264, 5)
    x = torch.from_numpy(R.drawn_rows(rows, vocab, seed=3, minus_inf=0.02)).to(dtype)
    if dtype != torch.float32:
        assert len(np.unique(x[0].double().numpy())) < vocab // 4          # 16-bit vocabulary rows: thousands of ties
    x[1, 100:3000] = x[1, 100]                                              # one run of ties over many chunks
    tokens = R.drawn_targets(rows, vocab, 1, seed=4)[:, 0]
    tokens[1], tokens[2], tokens[3] = 1500, -1, vocab                        # inside the run; two tokens out of range
    counters = np.arange(rows) % cols
    got, want = _check_rows(x, tokens, counters, cols, n_top, f'{dtype} n={n_top}')
    assert got['rank'][2, 2] == -1 and got['logprob'][2, 2] == 0 and got['rank'][3, 3] == -1
    assert (want['rank'][np.arange(rows), counters] >= -1).all()


def test_twin_on_signed_zeros_nans_and_infinities():
    vocab, cols, n = 257, 3, 6
    x = R.drawn_rows(8, vocab, seed=5)
    x[0, x[0] > 0] = -1.0
    x[0, [3, 40, 256]] = [-0.0, 0.0, -0.0]                                   # the maximum is a zero at three columns
    x[1, [7, 200]] = np.nan
    x[2, 5] = np.inf
    x[3] = -np.inf
    x[4, 1:] = -np.inf
    x[5, [9, 10]] = [np.inf, np.nan]
    x[6, :250] = -np.inf
    tokens = np.array([40, 7, 5, 0, 0, 10, 252, 3])
    got, want = _check_rows(torch.from_numpy(x), tokens, np.array([0, 1, 2, 0, 1, 2, 0, 1]), cols, n, 'specials')
    assert got['top_idx'][0, 0].tolist()[:3] == [3, 40, 256] and got['rank'][0, 0] == 1
    assert got['top_idx'][1, 1].tolist()[:2] == [7, 200] and got['rank'][1, 1] == 0      # NaNs first; a NaN token ranks 0
    assert got['top_idx'][5, 2].tolist()[:2] == [10, 9]                                   # the NaN above +inf
    assert np.isnan(got['logprob'][1, 1]) and np.isnan(got['top_logprob'][1, 1]).all()
    assert got['top_idx'][3, 0].tolist() == list(range(n))                                # a row of -inf: column order


def test_a_counter_out_of_range_writes_nothing():
    vocab, cols, n = 64, 4, 3
    x = torch.from_numpy(R.drawn_rows(5, vocab, seed=6))
    counters = np.array([-1, cols, 2, -100, 10 ** 6])
    got = _twin(x, np.arange(5), counters, cols, n, canary=True)
    for name, v in got.items():
        untouched = np.ones(v.shape[:2], dtype=bool)
        untouched[2, 2] = False
        canary = 77 if name in ('rank', 'top_idx') else 7.5
        assert (v[untouched] == canary).all(), name
        assert (v[2, 2] != canary).all(), name


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_the_token_at_top_position_i_has_rank_i(dtype):
    rows, vocab, n = 6, 2049, 16
    x = torch.from_numpy(R.drawn_rows(rows, vocab, seed=8)).to(dtype)
    x[0, 10:2000] = x[0, 10]
    x[1, [5, 6]] = torch.tensor([0.0, -0.0], dtype=dtype)
    first = _twin(x, np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int64), 1, n)
    for i in range(n):
        again = _twin(x, first['top_idx'][:, 0, i].astype(np.int64), np.zeros(rows, dtype=np.int64), 1, 0)
        assert (again['rank'][:, 0] == i).all(), i


# ---- generation ------------------------------------------------------------------------------------------------------------------

class Recording(torch.nn.Module):
    """Keeps logits[:, -1] of every cached step (the prefill's pick takes the logits the result returns as `scores`)."""

    def __init__(self, model):
        super().__init__()
        self.model, self.steps, self.calls = model, [], 0

    def forward(self, input_ids, inference_params=None, **kw):
        out = self.model(input_ids, inference_params=inference_params, **kw)
        if self.calls:
            self.steps.append(out.logits[:, -1].detach().clone())
        self.calls += 1
        return out


def _expected(out, step_logits, begins, n_top, names):
    """The restatement on the logits of every step, column for column: step s of row b describes column begins[b] + s, kept
    in front of the row's end."""
    seq = out.sequences.numpy()
    batch, width = seq.shape
    ends = out.lengths.numpy() if out.lengths is not None else np.full(batch, width)
    recs = P.new_records(batch, width, n_top, names)
    unit, unit_ent = np.zeros((batch, width)), np.zeros((batch, width))
    for s, lg in enumerate(step_logits):
        cols = np.asarray(begins) + s
        x64 = lg.double().numpy()
        tokens = np.array([seq[b, c] if c < width else 0 for b, c in enumerate(cols)])
        rep = P.row_report(x64, tokens, n_top)
        u, ue = R.units(x64)
        for b, c in enumerate(cols):
            if c < min(ends[b], width):
                for n in recs:
                    recs[n][b, c] = rep[n][b]
                unit[b, c], unit_ent[b, c] = u[b], ue[b]
    return recs, unit, unit_ent


def _fields(out):
    got = {'logprob': out.token_logprobs, 'rank': out.token_ranks, 'entropy': out.token_entropies, 'top_idx': out.top_token_ids,
           'top_logprob': out.top_token_logprobs}
    return {n: v.numpy() for n, v in got.items() if v is not None}


def _run_and_check(decode, model, ids, n, n_top, tag, begins=None, output_logprobs=True, **kw):
    rec = Recording(model)
    out = decode(ids, rec, n, kv_cache=True, output_logprobs=output_logprobs, top_logprobs=n_top, **kw)
    plain = decode(ids, model, n, kv_cache=True, device_pick=True, **kw)
    assert torch.equal(out.sequences, plain.sequences), tag
    assert (out.lengths is None) == (plain.lengths is None) and (out.lengths is None or torch.equal(out.lengths, plain.lengths))
    got = _fields(out)
    names = tuple(n_ for n_ in P.RECORDS if n_ in got)
    assert names == tuple(n_ for n_ in P.RECORDS if (output_logprobs and not n_.startswith('top_')) or (n_top and n_.startswith('top_')))
    for v in got.values():
        assert v.shape[:2] == tuple(out.sequences.shape), tag
    begins = [ids.shape[1]] * ids.shape[0] if begins is None else list(begins)
    want, unit, unit_ent = _expected(out, [out.scores[0]] + rec.steps, begins, n_top, names)
    _assert_records(got, want, unit, unit_ent, tag)
    for b, begin in enumerate(begins):                                   # prompt columns hold the initial values
        for n_, v in got.items():
            assert (v[b, :begin] == P.INITIAL[n_]).all(), (tag, n_)
    return out, got


def _state():
    return torch.tensor([1234, 77], dtype=torch.int64)


@pytest.fixture(scope='module')
def nano():
    model = _backpack(seed=3)
    ids = torch.randint(0, VOCAB, (3, PROMPT), generator=torch.Generator().manual_seed(4))
    free = greedy_decode(ids, model, PROMPT + STEPS, kv_cache=True, device_pick=True).sequences
    return model, ids, free


def test_greedy_and_sampled_records_equal_the_restatement(nano):
    model, ids, free = nano
    n = PROMPT + STEPS
    out, got = _run_and_check(greedy_decode, model, ids, n, 5, 'greedy')
    assert (got['rank'][:, PROMPT:] == 0).all() and np.array_equal(got['top_idx'][:, PROMPT:, 0], out.sequences[:, PROMPT:].numpy())
    assert (got['logprob'][:, PROMPT:] < 0).all() and (got['entropy'][:, PROMPT:] > 0).all()
    _run_and_check(greedy_decode, model, ids, n, 0, 'greedy, scalars only')
    _, only_top = _run_and_check(greedy_decode, model, ids, n, 16, 'greedy, top only', output_logprobs=False)
    assert sorted(only_top) == ['top_idx', 'top_logprob']
    out, got = _run_and_check(sample, model, ids, n, 3, 'sample', rng_state=_state())
    assert (got['rank'][:, PROMPT:] > 0).any(), 'every draw was the greedy token: a weak test'
    _run_and_check(sample, model, ids, n, 2, 'sample top-k top-p', rng_state=_state(), top_k=20, top_p=0.9, temperature=1.3)


def test_records_stop_at_the_eos_and_follow_prompt_lengths(nano):
    model, ids, free = nano
    n = PROMPT + STEPS
    eos = int(free[0, PROMPT + 3])                                       # provably occurs: row 0 ends there at the latest
    out, got = _run_and_check(greedy_decode, model, ids, n, 4, 'greedy eos', eos_token_id=eos, pad_token_id=0)
    end = int(out.lengths[0])
    assert end <= PROMPT + 4 and int(out.sequences[0, end - 1]) == eos
    assert got['rank'][0, end - 1] == 0 and got['logprob'][0, end - 1] != 0          # the EOS itself keeps its record
    if end < out.sequences.shape[1]:
        assert (got['rank'][0, end:] == -1).all() and (got['logprob'][0, end:] == 0).all() and (got['top_idx'][0, end:] == -1).all()
    _run_and_check(sample, model, ids, n, 2, 'sample eos', rng_state=_state(), eos_token_id=eos, repetition_penalty=1.2)
    lengths = [PROMPT, 3, 5]
    out, got = _run_and_check(greedy_decode, model, ids, n, 3, 'ragged', begins=lengths, prompt_lengths=lengths)
    assert out.lengths.tolist() == [L + STEPS - 1 for L in lengths]
    assert (got['rank'][1, 3 + STEPS - 1:] == -1).all() and (got['rank'][1, 3:3 + STEPS - 1] >= 0).all()
    _run_and_check(sample, model, ids, n, 1, 'ragged sample eos', begins=lengths, prompt_lengths=lengths, rng_state=_state(),
                   eos_token_id=eos, top_k=30)


def test_the_record_of_an_annealed_wrapper_is_of_the_distribution_it_drew_from(nano):
    from src.models.intervened_models import WeightedBackpackLMHeadModel
    from src.utils.scoring import generation_logprob
    model, ids, free = nano
    n = PROMPT + STEPS
    cw = torch.rand(VOCAB, 16, generator=torch.Generator().manual_seed(11)) * 3
    scale = _anneal_scale(model, free, range(PROMPT, n))
    wrapper = WeightedBackpackLMHeadModel(model, cw, None, scale, anneal=True, upweight_nearby=True).eval()
    out, got = _run_and_check(greedy_decode, wrapper, ids, n, 4, 'annealed')
    _assert_scores_in_band(model, out.sequences, scale, range(PROMPT, n))
    # a second pass over the finished text sums the similarities over the WHOLE sequence: not the distribution of the step
    with torch.inference_mode():
        post = torch.log_softmax(wrapper(out.sequences).logits.float(), dim=-1)
    post = post[:, PROMPT - 1:-1].gather(2, out.sequences[:, PROMPT:, None])[:, :, 0].numpy()
    assert np.abs(post - got['logprob'][:, PROMPT:]).max() > 1e-3
    total = generation_logprob(out)
    assert total.count.tolist() == [STEPS - 1] * 3
    want = got['logprob'].astype(np.float64).sum(axis=1)
    assert np.allclose(total.logprob.numpy(), want, rtol=0, atol=1e-12)
    assert np.allclose(total.perplexity.numpy(), np.exp(-want / (STEPS - 1)), rtol=1e-12)
    with pytest.raises(ValueError):
        generation_logprob(greedy_decode(ids, model, n, kv_cache=True))


def test_the_record_does_not_depend_on_the_polling_interval(nano):
    model, ids, free = nano
    eos = int(free[0, PROMPT + 3])
    outs = [sample(ids, model, PROMPT + STEPS, kv_cache=True, rng_state=_state(), eos_token_id=eos, stop_check_every=every,
                   output_logprobs=True, top_logprobs=3) for every in (1, 3, 1000)]
    for out in outs[1:]:
        assert torch.equal(out.sequences, outs[0].sequences) and torch.equal(out.lengths, outs[0].lengths)
        for a, b in zip(_fields(out).values(), _fields(outs[0]).values()):
            assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_generation_logprob_counts_behind_the_prompt_and_in_front_of_the_end(nano):
    from src.utils.scoring import generation_logprob
    model, ids, free = nano
    eos = int(free[0, PROMPT + 3])
    lengths = [PROMPT, 3, 5]
    out = greedy_decode(ids, model, PROMPT + STEPS, kv_cache=True, prompt_lengths=lengths, eos_token_id=eos, output_logprobs=True)
    total = generation_logprob(out, prompt_lengths=lengths)
    assert total.count.tolist() == [int(e) - b for e, b in zip(out.lengths, lengths)]
    assert torch.equal(total.logprob, generation_logprob(out).logprob)
    assert torch.allclose(total.logprob, out.token_logprobs.double().sum(dim=1))


def test_argument_checks(nano):
    model, ids, _ = nano
    n = PROMPT + 4
    for decode in (greedy_decode, sample):
        with pytest.raises(ValueError, match='kv_cache'):
            decode(ids, model, n, output_logprobs=True)
        with pytest.raises(ValueError, match='kv_cache'):
            decode(ids, model, n, top_logprobs=2)
        with pytest.raises(ValueError, match='top_logprobs'):
            decode(ids, model, n, kv_cache=True, top_logprobs=G.PICK_REPORT_MAX_TOP + 1)
        with pytest.raises(ValueError, match='top_logprobs'):
            decode(ids, model, n, kv_cache=True, top_logprobs=-1)
    with pytest.raises(ValueError, match='kv_cache'):
        model.generate(ids, n, top_logprobs=2)
    out = model.generate(ids, n, kv_cache=True, top_logprobs=2, return_dict_in_generate=True)
    assert out.top_token_ids.shape == (3, n - 1, 2) and out.token_logprobs is None
    out = model.sample(ids, n, kv_cache=True, output_logprobs=True, return_dict_in_generate=True)
    assert out.token_logprobs.shape == (3, n - 1) and out.top_token_ids is None
    plain = model.generate(ids, n, kv_cache=True, return_dict_in_generate=True)
    assert plain.token_logprobs is None and plain.token_ranks is None and plain.top_token_logprobs is None
    tiny = _backpack(seed=1)
    tiny_logits = torch.zeros(2, 8)
    with pytest.raises(RuntimeError):
        _eager_report(tiny_logits, torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32),
                      top_idx=torch.zeros((2, 1, 9), dtype=torch.int32))

    class Narrow(torch.nn.Module):                                       # a vocabulary of 8 under top_logprobs = 9
        def forward(self, input_ids, inference_params=None):
            return SimpleNamespace(logits=tiny(input_ids, inference_params=inference_params).logits[..., :8])
    with pytest.raises(ValueError, match='vocabulary'):
        greedy_decode(ids % 8, Narrow(), n, kv_cache=True, top_logprobs=9)


def test_binding_names_its_limits_and_refuses_host_tensors():
    import bp_hip
    assert bp_hip.PICK_REPORT_MAX_TOP == G.PICK_REPORT_MAX_TOP == 16
    assert 'bp_pick_report' in bp_hip.SIGNATURES
    x = torch.zeros(2, 8)
    assert not bp_hip.pick_report_supported(x)
    with pytest.raises(RuntimeError):
        bp_hip.pick_report(x, torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32),
                           logprob=torch.zeros(2, 3))


# ---- the code objects ------------------------------------------------------------------------------------------------------------

def test_report_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_resources as KR
    if not KR.tools_available():
        pytest.skip('llvm-objcopy / clang-offload-bundler / llvm-readelf not found under /opt/rocm')
    import importlib.util
    spec = importlib.util.spec_from_file_location('bp_build_hip', os.path.join(ROOT, 'backpacks-flash-attn_amd', 'build_hip.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()   # no-op when the objects are current
    ks = KR.kernels([os.path.join(KR.BUILD, 'pick_report.o')])
    assert sorted(k['name'] for k in ks) == ['pick_report_kernel<BF16>', 'pick_report_kernel<F16>', 'pick_report_kernel<float>']
    for k in ks:
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
        assert k['waves_per_simd'] >= 4, k                                # a 1024-thread workgroup is four waves per SIMD
