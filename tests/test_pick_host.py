"""CPU: the token pick's torch restatement (_eager_pick) against the float64 numpy restatement of tests/pick_ref.py, the new
generation options on the nano model, and the argument checks of bp_pick_token (no launch, no GPU)."""
import ctypes

import numpy as np
import pytest
import torch

import bp_hip
import philox_ref as P
import pick_ref as R
from decode_support import PROMPT, STEPS
from decode_support import _nano_backpack as _backpack
from src.utils.generation import _eager_pick, _pick_uniforms

INF, NAN = float('inf'), float('nan')
SEED, OFFSET = 1234, 77


def _state(seed=SEED, offset=OFFSET):
    return torch.tensor([seed, offset], dtype=torch.int64)


def _eager(rows, counters=None, **kw):
    x = torch.tensor(np.asarray(rows, dtype=np.float32))
    c = None if counters is None else torch.tensor(counters, dtype=torch.int32)
    return _eager_pick(x, rng_state=_state(), counters=c, **kw).tolist()


# ---- the uniform -------------------------------------------------------------------------------------------------------------------

def test_uniform_of_known_seed_offset_row_counter():
    cases = [(1234, 77, 0, 0), (1234, 77, 3, 5), (1234, 77, 63, 511), (-5, 2 ** 40 + 3, 7, 2 ** 31 - 1), (2 ** 62 + 1, -9, 0, 12)]
    for seed, offset, row, counter in cases:
        counters = torch.zeros(row + 1, dtype=torch.int32)
        counters[row] = counter
        got = _pick_uniforms(_state(seed, offset), counters)[row].item()
        assert got == R.uniform(seed, offset, row, counter), (seed, offset, row, counter)
        assert 0.0 < got < 1.0
    # the restatement itself, spelled out once: stream of row 3, counter 5
    key, salt = P.stream(1234, 77, 3)
    r0, _ = P.philox2x32(5, salt, key)
    assert R.uniform(1234, 77, 3, 5) == ((int(r0) >> 8) + 0.5) / 2 ** 24
    # rows and counters draw different numbers
    us = {R.uniform(1234, 77, r, c) for r in range(4) for c in range(4)}
    assert len(us) == 16


# ---- greedy ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('row', [
    [1.0, 3.0, 3.0, 2.0],                 # tie: the lowest index
    [5.0, 1.0, 5.0],                      # tie with the first column
    [0.0, -0.0, 0.0],                     # signed zeros are equal
    [-INF, -INF, -INF],                   # nothing finite: index 0
    [1.0, INF, 2.0, INF],
    [1.0, NAN, INF, NAN],                 # the first NaN wins, even over +inf
    [-INF, -3.0, -INF],
    [7.0],
])
def test_greedy_is_numpy_argmax(row):
    assert _eager([row]) == [R.greedy(row)]
    assert _eager([row]) == [int(torch.argmax(torch.tensor(row)))]


# ---- the kept set and the draw -----------------------------------------------------------------------------------------------------

def _check_rows(x, counters, **kw):
    got = _eager(x, counters, do_sample=True, **kw)
    exact = 0
    for b, row in enumerate(x):
        token, z, keep, u = R.pick(row, True, kw.get('temperature', 1.0), kw.get('top_k', 0), kw.get('top_p', 1.0),
                                   SEED, OFFSET, b, counters[b])
        if keep is None:
            assert got[b] == token, ('degenerate rows take the greedy answer', b)
        else:
            R.assert_draw(got[b], z, keep, u, 1e-9, what=(b, kw))     # float64 both: only the order of the sums differs
        exact += got[b] == token
    assert exact >= len(x) - 1          # a draw within 1e-9 of a boundary may fall either way; not two of them
    return got


@pytest.mark.parametrize('kw', [
    dict(), dict(temperature=0.7), dict(top_k=1), dict(top_k=5), dict(top_k=0), dict(top_k=40), dict(top_k=41),
    dict(top_k=1000), dict(top_p=0.9), dict(top_p=0.05), dict(top_p=1.0), dict(temperature=1.3, top_k=10, top_p=0.8),
    dict(temperature=0.7, top_k=10),
])
def test_eager_pick_matches_the_numpy_restatement(kw):
    rng = np.random.default_rng(5)
    x = (2.0 * rng.standard_normal((48, 40))).astype(np.float32)
    x[3, 7] = x[3, 9] = x[3].max() + 1.0           # ties at the top
    x[4, :] = np.round(x[4])                       # many ties everywhere
    x[5, 10:] = -INF
    x[6, :] = -INF                                 # degenerate
    x[7, 2] = NAN                                  # degenerate
    x[8, 30] = INF                                 # degenerate
    x[9, :] = 1.5                                  # all equal
    counters = [(3 * b + 1) % 17 for b in range(48)]
    got = _check_rows(x, counters, **kw)
    assert got[6] == 0 and got[7] == 2 and got[8] == 30


def test_top_k_edges_and_ties_kept():
    z = np.array([3.0, 1.0, 2.0, 2.0, 0.0, 2.0], dtype=np.float32)
    assert R.kept_set(z, top_k=1).tolist() == [True, False, False, False, False, False]
    assert R.kept_set(z, top_k=2).tolist() == [True, False, True, True, False, True]      # the tie at the threshold stays
    assert R.kept_set(z, top_k=4).tolist() == [True, False, True, True, False, True]
    assert R.kept_set(z, top_k=5).tolist() == [True, True, True, True, False, True]
    for k in (0, -1, 6, 7):                                                                 # off
        assert R.kept_set(z, top_k=k).all()
    # _eager_pick never returns a dropped token, whatever the counter
    for k, allowed in ((1, {0}), (2, {0, 2, 3, 5}), (5, {0, 1, 2, 3, 5}), (0, set(range(6))), (6, set(range(6)))):
        seen = set(_eager([z] * 64, list(range(64)), do_sample=True, top_k=k, temperature=2.0))
        assert seen <= allowed, (k, seen)
        if k in (2, 5):
            assert len(seen) > 1


def test_top_p_rule_is_closed_under_ties():
    # probabilities 0.4, 0.2, 0.2, 0.1, 0.1
    probs = np.array([0.4, 0.2, 0.2, 0.1, 0.1])
    z = np.log(probs).astype(np.float32)
    assert R.kept_set(z, top_p=0.3).tolist() == [True, False, False, False, False]
    assert R.kept_set(z, top_p=0.41).tolist() == [True, True, True, False, False]     # mass above the pair: 0.4 < 0.41, both stay
    assert R.kept_set(z, top_p=0.7).tolist() == [True, True, True, False, False]
    assert R.kept_set(z, top_p=0.81).tolist() == [True, True, True, True, True]
    # top-p renormalises over what top-k kept: with k = 3 the masses are 0.5, 0.25, 0.25
    assert R.kept_set(z, top_k=3, top_p=0.45).tolist() == [True, False, False, False, False]
    assert R.kept_set(z, top_k=3, top_p=0.55).tolist() == [True, True, True, False, False]
    for p, allowed in ((0.3, {0}), (0.41, {0, 1, 2}), (0.81, {0, 1, 2, 3, 4})):
        seen = set(_eager([z] * 64, list(range(64)), do_sample=True, top_p=p))
        assert seen <= allowed and (len(allowed) == 1 or len(seen) > 1), (p, seen)
    seen = set(_eager([z] * 64, list(range(64)), do_sample=True, top_k=3, top_p=0.45))
    assert seen == {0}


def test_draw_is_in_vocabulary_order_not_sorted_order():
    # two tokens, the SMALLER probability first: u < 0.25 must give token 0
    z = np.log(np.array([0.25, 0.75])).astype(np.float32)
    counters = list(range(200))
    got = _eager([z] * 200, counters, do_sample=True)
    for b, c in enumerate(counters):
        u = R.uniform(SEED, OFFSET, b, c)
        if abs(u - 0.25) > 1e-6:
            assert got[b] == (0 if u < 0.25 else 1), (b, u)
    assert 20 < got.count(0) < 80


def test_the_contract_itself_stays_far_inside_the_chi_square_bound():
    """The three cases of test_gpu_pick.py::test_distribution_chi_square, drawn by the restatement: what the bound leaves to
    the kernel.  (1 - 1e-9 quantile of chi-square at the case's degrees of freedom.)"""
    from scipy.stats import chi2
    for vocab, bf16, temperature, top_k, top_p in ((1000, False, 0.8, 50, 0.9), (1000, False, 1.0, 0, 1.0),
                                                    (50257, True, 0.7, 40, 0.95)):
        x = (2.0 * np.random.default_rng(0).standard_normal(vocab)).astype(np.float32)
        if bf16:
            x = torch.from_numpy(x).bfloat16().float().numpy()
        z = R.scaled(x, temperature)
        keep = R.kept_set(z, top_k, top_p)
        probs = R.masses(z) * keep
        probs /= probs.sum()
        counts = R.simulate(z, keep, SEED, OFFSET, 4096, 64)
        assert counts.sum() == 4096 * 64 and counts[~keep].sum() == 0
        stat, df = R.chi_square(counts, probs, 4096 * 64)
        bound = chi2.ppf(1 - 1e-9, df)
        print(f'contract chi-square {stat:.1f} at df {df} (bound {bound:.1f})')
        assert stat < bound


# ---- generation on the nano model --------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def nano():
    model = _backpack()
    ids = torch.randint(0, 200, (2, PROMPT), generator=torch.Generator().manual_seed(3))
    return model, ids


def test_calls_without_the_new_arguments_are_unchanged(nano):
    model, ids = nano
    n = PROMPT + STEPS
    want = model.generate(ids, n)
    assert torch.equal(model.generate(ids, n, temperature=1.0, top_k=0, top_p=1.0, rng_state=None, device_pick=False), want)
    torch.manual_seed(11)
    a = model.sample(ids, n)
    torch.manual_seed(11)
    b = model.sample(ids, n, device_pick=False)
    torch.manual_seed(11)
    # today's sampler, statement for statement
    from src.utils.generation import _decode
    c = _decode(ids, model, n, lambda logits: torch.distributions.Categorical(
        logits=torch.log_softmax(logits.float(), dim=-1)).sample()).sequences
    assert torch.equal(a, b) and torch.equal(a, c)


def test_device_pick_greedy_equals_generate(nano):
    model, ids = nano
    n = PROMPT + STEPS
    want = model.generate(ids, n)
    assert torch.equal(model.generate(ids, n, device_pick=True), want)
    assert torch.equal(model.generate(ids, n, device_pick=True, kv_cache=True), model.generate(ids, n, kv_cache=True))
    out = model.generate(ids, n, device_pick=True, kv_cache=True, return_dict_in_generate=True, output_scores=True)
    assert out.sequences.shape == (2, n - 1) and out.sequences.dtype == ids.dtype and len(out.scores) == 1
    assert torch.equal(model.generate(ids, 3, device_pick=True, kv_cache=True), model.generate(ids, 3))
    assert torch.equal(model.generate(ids, PROMPT, device_pick=True, kv_cache=True), ids)     # nothing to generate


@pytest.mark.parametrize('kw', [dict(top_k=10, temperature=0.7), dict(top_p=0.9), dict(device_pick=True)])
def test_sampling_kv_cache_equals_the_growing_prefix(nano, kw):
    model, ids = nano
    n = PROMPT + STEPS
    grown = model.sample(ids, n, rng_state=_state(), **kw)
    cached = model.sample(ids, n, rng_state=_state(), kv_cache=True, **kw)
    assert grown.shape == (2, n - 1) and torch.equal(grown[:, :PROMPT], ids)
    assert ((grown >= 0) & (grown < 200)).all()
    # the two loops compute their logits differently (fp32 rounding); a token differs only where u sits on a boundary
    assert torch.equal(grown, cached)
    assert torch.equal(model.sample(ids, n, rng_state=_state(), **kw), grown)                  # same state, same tokens
    other = model.sample(ids, n, rng_state=_state(offset=OFFSET + 1), **kw)
    assert not torch.equal(other[:, PROMPT:], grown[:, PROMPT:])                               # another offset, other tokens


def test_sampling_follows_torch_manual_seed(nano):
    model, ids = nano
    n = PROMPT + 8
    torch.manual_seed(5)
    a = model.sample(ids, n, top_k=10)
    torch.manual_seed(5)
    b = model.sample(ids, n, top_k=10)
    c = model.sample(ids, n, top_k=10)
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_sampled_tokens_respect_top_k_of_the_teacher_forced_logits(nano):
    model, ids = nano
    n = PROMPT + STEPS
    seq = model.sample(ids, n, rng_state=_state(), top_k=3, temperature=0.9, kv_cache=True)
    with torch.no_grad():
        logits = model(seq).logits.float().numpy()
    for b in range(2):
        for t in range(PROMPT, n - 1):
            z = R.scaled(logits[b, t - 1], 0.9)
            keep = R.kept_set(z, top_k=3)
            u = R.uniform(SEED, OFFSET, b, t)
            R.assert_draw(int(seq[b, t]), z, keep, u, R.epsilon(200), what=(b, t))


def test_generation_rejects_bad_options(nano):
    model, ids = nano
    for kw in (dict(temperature=0.0), dict(temperature=float('nan')), dict(top_p=0.0), dict(top_p=1.5)):
        with pytest.raises(ValueError):
            model.sample(ids, PROMPT + 2, **kw)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_pick_token_rejects_bad_arguments_before_any_launch():
    h = bp_hip.lib()
    assert h.bp_abi_version() == 11
    p, null = ctypes.c_void_p(0x1000), None

    def call(logits=p, tokens=p, sequences=null, stats=null, rng=p, counters=null, batch=2, vocab=100, row_stride=100,
             tokens_stride=1, seq_stride=0, seq_cols=0, do_sample=1, temperature=1.0, top_k=0, top_p=1.0, dtype=1):
        return h.bp_pick_token(logits, tokens, sequences, stats, rng, counters, batch, vocab, row_stride, tokens_stride,
                               seq_stride, seq_cols, do_sample, temperature, top_k, top_p, dtype, null)
    assert call(dtype=3) == -1 and call(dtype=-1) == -1
    for kw in (dict(batch=0), dict(vocab=0), dict(vocab=2 ** 23 + 1, row_stride=2 ** 24), dict(row_stride=99),
               dict(tokens_stride=0), dict(logits=null), dict(tokens=null),
               dict(sequences=p, seq_cols=0, seq_stride=8), dict(sequences=p, seq_cols=8, seq_stride=7),
               dict(logits=ctypes.c_void_p(0x1001)), dict(logits=ctypes.c_void_p(0x1002), dtype=2),
               dict(tokens=ctypes.c_void_p(0x1004)), dict(stats=ctypes.c_void_p(0x1002)),
               dict(counters=ctypes.c_void_p(0x1002)), dict(rng=ctypes.c_void_p(0x1004))):
        assert call(**kw) == -3, kw
    for bad in (0.0, -1.0, float('nan'), float('inf'), 1e-45):
        assert call(temperature=bad) == -4, bad
        assert call(temperature=bad, do_sample=0) == -4, bad
    for bad in (0.0, -0.5, 1.0000001, float('nan')):
        assert call(top_p=bad) == -10, bad
    assert call(rng=null) == -10
    assert 'top_p' in h.bp_strerror(-10).decode()
    # the binding refuses host tensors
    with pytest.raises(RuntimeError, match='GPU'):
        bp_hip.pick_token(torch.zeros(2, 8))


def test_pick_kernels_use_no_scratch():
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_resources as KR
    if not KR.tools_available():
        pytest.skip('LLVM tools not found under /opt/rocm')
    import importlib.util
    spec = importlib.util.spec_from_file_location('bp_build_hip', os.path.join(ROOT, 'backpacks-flash-attn_amd', 'build_hip.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()   # no-op when the objects are current
    ks = KR.kernels([os.path.join(KR.BUILD, 'pick_token.o')])
    assert {k['name'] for k in ks} == {'pick_token_kernel<BF16>', 'pick_token_kernel<F16>', 'pick_token_kernel<float>'}
    for k in ks:
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, k
        assert k['group_segment_fixed_size'] <= 160 * 1024 and k['max_flat_workgroup_size'] == 1024, k
