"""float64 numpy restatement of the sense-similarity measures, shared by test_sense_similarity_host.py and
test_gpu_sense_similarity.py.  Written from the reference's training/src/run_simlex.py, not from the code under test:

  flat       `flat_cosine` :194-200        both words reshaped to one vector: dot / (norm * norm)
  cosines    `_get_all_cosines` :202-208   vec1 @ vec2.t() / outer(norms1, norms2), a (k, k) matrix, rows = senses of word 1
  min_pair   :210-212  min of its diagonal       max_pair   :214-216  max of its diagonal
  min_all    :218-220  min of all of it          max_all    :222-224  max of all of it
  per_sense  `one_matched_cosine` :226-229, CosSense_l: the flat cosine of sense l of either word = the diagonal

Every function takes a (N, k, d) and b (M, k, d) and answers for ALL N x M pairs; a zero vector gives 0 / 0 = NaN and numpy's
min / max carry a NaN as torch's do.  `bounds` is the first-order fp32 error bound of every measure, from the inputs alone."""
import numpy as np

U = 2.0 ** -24


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _pair_products(a, b):
    """(N, M, k, k): [n, m, l', l] = a[n, l'] . b[m, l]."""
    n, k, d = a.shape
    m = b.shape[0]
    return (a.reshape(n * k, d) @ b.reshape(m * k, d).T).reshape(n, k, m, k).transpose(0, 2, 1, 3)


def cosines(a, b):
    """(N, M, k, k): cos[n, m, l', l] of sense l' of a[n] and sense l of b[m] (run_simlex.py:202-208)."""
    a, b = _f64(a), _f64(b)
    dot = _pair_products(a, b)
    na, nb = np.sqrt((a * a).sum(-1)), np.sqrt((b * b).sum(-1))
    with np.errstate(invalid='ignore', divide='ignore'):
        return dot / (na[:, None, :, None] * nb[None, :, None, :])


def measures(a, b):
    """dict: the five (N, M) measures and per_sense (N, k, M)."""
    a, b = _f64(a), _f64(b)
    n, k, d = a.shape
    cos = cosines(a, b)
    diag = np.diagonal(cos, axis1=2, axis2=3)                       # (N, M, k)
    fa, fb = a.reshape(n, -1), b.reshape(b.shape[0], -1)
    with np.errstate(invalid='ignore', divide='ignore'):
        flat = (fa @ fb.T) / (np.sqrt((fa * fa).sum(-1))[:, None] * np.sqrt((fb * fb).sum(-1))[None, :])
    return {'flat': flat, 'min_pair': diag.min(-1), 'max_pair': diag.max(-1),
            'min_all': cos.reshape(cos.shape[0], cos.shape[1], -1).min(-1),
            'max_all': cos.reshape(cos.shape[0], cos.shape[1], -1).max(-1),
            'per_sense': np.ascontiguousarray(diag.transpose(0, 2, 1))}


def bounds(a, b):
    """dict of the same shapes: the first-order bound on |fp32 result - exact| with u = 2^-24.  A cosine of two d-vectors
    computed as dot / (sqrt(A) * sqrt(B)) with fp32 sums in any order is within
        (d - 1) u S / (sqrt(A) sqrt(B)) + |cos| ((d - 1) u + 5 u),     S = sum_e |a_e b_e|
    (the dot's summation error; the two squared norms' summation errors, each halved by its square root: (d - 1) u together;
    five roundings: the two square roots, their product, the quotient, and one to spare).  The flat measure is a cosine of
    two k d-vectors; a min / max measure takes the largest bound among its members."""
    a, b = _f64(a), _f64(b)
    n, k, d = a.shape
    s = _pair_products(np.abs(a), np.abs(b))
    na, nb = np.sqrt((a * a).sum(-1)), np.sqrt((b * b).sum(-1))
    with np.errstate(invalid='ignore', divide='ignore'):
        cos = cosines(a, b)
        bc = (d - 1) * U * s / (na[:, None, :, None] * nb[None, :, None, :]) + np.abs(cos) * ((d - 1) * U + 5 * U)
        fa, fb = a.reshape(n, -1), b.reshape(b.shape[0], -1)
        fn = np.sqrt((fa * fa).sum(-1))[:, None] * np.sqrt((fb * fb).sum(-1))[None, :]
        flat = (fa @ fb.T) / fn
        bf = (k * d - 1) * U * (np.abs(fa) @ np.abs(fb).T) / fn + np.abs(flat) * ((k * d - 1) * U + 5 * U)
    diag = np.diagonal(bc, axis1=2, axis2=3)
    every = bc.reshape(bc.shape[0], bc.shape[1], -1).max(-1)
    return {'flat': bf, 'min_pair': diag.max(-1), 'max_pair': diag.max(-1), 'min_all': every, 'max_all': every,
            'per_sense': np.ascontiguousarray(diag.transpose(0, 2, 1))}


def worst_ratio(got, want, bound, factor=1.0):
    """max over the finite entries of |got - want| / (factor * bound); NaNs must sit in the same places."""
    got, want, bound = _f64(got), _f64(want), _f64(bound)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert (np.isnan(got) == np.isnan(want)).all(), 'NaNs in different places'
    live = ~np.isnan(want)
    if not live.any():
        return 0.0
    err, allowed = np.abs(got - want)[live], factor * bound[live]
    return float(np.max(np.where(err == 0, 0.0, err / np.where(allowed > 0, allowed, np.finfo(np.float64).tiny))))


def bits_of(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def spearman(x, y):
    """Spearman's rho with average ranks, float64 (what scipy.stats.spearmanr computes: Pearson on the ranks)."""
    def ranks(v):
        v = _f64(v)
        order = np.argsort(v, kind='stable')
        r = np.empty(len(v))
        sv = v[order]
        i = 0
        while i < len(v):
            j = i
            while j + 1 < len(v) and sv[j + 1] == sv[i]:
                j += 1
            r[order[i:j + 1]] = (i + j) / 2.0 + 1.0
            i = j + 1
        return r
    rx, ry = ranks(x), ranks(y)
    rx, ry = rx - rx.mean(), ry - ry.mean()
    return float((rx * ry).sum() / np.sqrt((rx * rx).sum() * (ry * ry).sum()))
