"""Host restatement of the token pick (include/bp_hip.h: bp_pick_token) in float64 numpy -- test infrastructure shared by
test_pick_host.py and test_gpu_pick.py.  Independent of src/utils/generation.py::_eager_pick (torch) and of the kernel: the
uniform comes from philox_ref, the kept set from a walk over the distinct logit values, the token from a plain cumsum."""
import numpy as np

import philox_ref as P


def epsilon(vocab):
    """Bound on the error of a normalised fp32 mass sum against the float64 one, for ANY summation order of `vocab`
    non-negative terms (vocab 2^-24, first order) plus a few ulp per exponential (the 64)."""
    return (vocab + 64) * 2.0 ** -24


def uniform(seed, offset, row, counter):
    """u = ((r0 >> 8) + 0.5) 2^-24 in float64 (exact), r0 of philox2x32(counter, salt, key) on the stream of `row`."""
    key, salt = P.stream(seed, offset, row)
    r0, _ = P.philox2x32(np.uint32(counter & 0xFFFFFFFF), salt, key)
    return (float(int(r0) >> 8) + 0.5) * 2.0 ** -24


def greedy(x):
    """Lowest index of the maximum, the first NaN if there is one: numpy.argmax."""
    return int(np.argmax(np.asarray(x, dtype=np.float32)))


def scaled(x, temperature):
    """z = float32(x) * float32(1 / T), both roundings as the kernel makes them."""
    return (np.asarray(x, dtype=np.float32) * (np.float32(1.0) / np.float32(temperature))).astype(np.float32)


def degenerate(z):
    return bool(np.isnan(z).any() or np.isposinf(z).any() or not np.isfinite(z).any())


def masses(z):
    with np.errstate(invalid='ignore'):
        return np.exp(z.astype(np.float64) - np.float64(z.max()))


def kept_set(z, top_k=0, top_p=1.0):
    """bool mask of the tokens that stay, for a non-degenerate row of scaled logits."""
    vocab = z.shape[0]
    keep = np.ones(vocab, dtype=bool)
    if 0 < top_k < vocab:
        tau = np.sort(z)[vocab - top_k]            # k-th largest, with multiplicity
        keep = z >= tau
    if top_p < 1.0:
        w = masses(z) * keep
        total = w.sum()
        values = np.unique(z[keep])[::-1]          # distinct kept logits, largest first
        above, ok = 0.0, set()
        for v in values:
            if above < top_p * total:
                ok.add(float(v))
            above += w[(z == v) & keep].sum()
        keep = keep & np.isin(z, np.array(sorted(ok), dtype=z.dtype))
    return keep


def cdf(z, keep):
    """Normalised vocabulary-order cumulative distribution over the kept tokens, float64."""
    w = masses(z) * keep
    c = np.cumsum(w)
    return c / c[-1]


def pick(x, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0, offset=0, row=0, counter=0):
    """(token, z, keep, u) of one row; keep is None for greedy / degenerate rows."""
    if not do_sample:
        return greedy(x), None, None, None
    z = scaled(x, temperature)
    u = uniform(seed, offset, row, counter)
    if degenerate(z):
        return greedy(x), z, None, u
    keep = kept_set(z, top_k, top_p)
    c = cdf(z, keep)
    hit = np.nonzero(c > u)[0]
    token = int(hit[0]) if hit.size else int(np.nonzero(keep)[0][-1])
    return token, z, keep, u


def assert_draw(token, z, keep, u, eps, what=''):
    """The token must be kept and satisfy cdf(t - 1) - eps <= u < cdf(t) + eps."""
    assert 0 <= token < z.shape[0], (what, token)
    assert keep[token], (what, 'token outside the kept set', token)
    c = cdf(z, keep)
    below = c[token - 1] if token > 0 else 0.0
    assert below - eps <= u < c[token] + eps, (what, token, below, u, c[token], eps)


def chi_square(counts, probs, draws):
    """Pearson chi-square over the tokens with an expected count >= 10, the rest pooled; (statistic, degrees of freedom)."""
    expected = probs * draws
    big = expected >= 10
    obs, exp = list(counts[big]), list(expected[big])
    if expected[~big].sum() > 0:
        obs.append(counts[~big].sum())
        exp.append(expected[~big].sum())
    obs, exp = np.array(obs, dtype=np.float64), np.array(exp, dtype=np.float64)
    return float(((obs - exp) ** 2 / exp).sum()), len(obs) - 1


def simulate(z, keep, seed, offset, rows, ncounters):
    """Token counts of the contract itself over rows x counters draws from one row of scaled logits."""
    c = cdf(z, keep)
    key, salt = P.stream(seed, offset, np.arange(rows, dtype=np.uint32))
    counts = np.zeros(z.shape[0], dtype=np.int64)
    for counter in range(ncounters):
        r0, _ = P.philox2x32(np.uint32(counter), salt, key)
        u = ((r0 >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
        counts += np.bincount(np.searchsorted(c, u, side='right'), minlength=z.shape[0])
    return counts
