"""Float64 numpy restatement of bp_score_rows (contract: include/bp_hip.h), the error units of its three real-valued outputs,
and the inputs shared by tests/test_scoring_host.py, tests/test_gpu_score_rows.py and tests/test_gpu_scoring.py.

Per row, with x the logits as float64 (the conversion of a 16-bit or fp32 element is exact):
  lse      = m + log(sum exp(x - m)), m = max x
  logprob  = x_t - lse;  0 for a target outside [0, cols)
  rank     = #{x_j > x_t} + #{j < t: x_j == x_t};  -1 for a target outside [0, cols);  0 for a NaN target
  top1     = the lowest index of the maximum, a NaN counting as larger than every number
  entropy  = lse - sum p_j x_j, p_j = exp(x_j - lse), a -inf entry contributing 0
Degenerate rows, by the arithmetic of the definitions in the extended reals: a NaN anywhere makes lse, entropy and every
logprob NaN; a +inf entry gives lse = +inf and entropy NaN (exp(inf - inf)); a row of -inf gives lse = -inf and entropy NaN;
logprob = x_t - lse in each case (inf - inf = NaN).  Ranks and top1 are comparisons and hold on every row.

Error units (the rule of the row-wise kernels: a bound is 4x the worst error of the fp32 twin against this file, in these units):
  lse, logprob   2^-23 (|lse| + max |x_j|)                          the scale the exponentials' arguments are rounded at
  entropy        the same times (1 + sum_j p_j |x_j|)               first order: d(sum p x) <= sum |dp| |x|, plus d lse
"""
import numpy as np

OUTPUTS = ('logprob', 'rank', 'lse', 'top1', 'entropy')
EPS32 = 2.0 ** -23


def score_rows(x, targets):
    """x (rows, cols) any float array, targets (rows,) or (rows, M) ints -> dict of the five outputs (float64 / int64)."""
    x = np.asarray(x, dtype=np.float64)
    targets = np.asarray(targets, dtype=np.int64)
    rows, cols = x.shape
    tg = targets.reshape(rows, -1)
    nan = np.isnan(x)
    has_nan = nan.any(axis=1)
    with np.errstate(all='ignore'):
        m = np.where(nan, -np.inf, x).max(axis=1)
        inf_row = np.isinf(m)
        shifted = x - np.where(inf_row, 0.0, m)[:, None]
        e = np.exp(shifted)
        s = e.sum(axis=1)
        lse = np.where(inf_row, m, m + np.log(s))
        lse = np.where(has_nan, np.nan, lse)
        t = np.where(e > 0, e * x, 0.0).sum(axis=1)
        entropy = np.where(has_nan | inf_row, np.nan, lse - t / s)
        inside = (tg >= 0) & (tg < cols)
        at = np.clip(tg, 0, cols - 1)
        xt = np.take_along_axis(x, at, axis=1)
        logprob = np.where(inside, xt - lse[:, None], 0.0)
        col = np.arange(cols)
        rank = np.empty(tg.shape, dtype=np.int64)
        for i in range(tg.shape[1]):
            above = (x > xt[:, i:i + 1]).sum(axis=1)
            tied_lower = ((x == xt[:, i:i + 1]) & (col[None, :] < at[:, i:i + 1])).sum(axis=1)
            rank[:, i] = np.where(inside[:, i], above + tied_lower, -1)
    first_max = np.where(x == m[:, None], col[None, :], cols).min(axis=1)
    first_nan = np.where(nan, col[None, :], cols).min(axis=1)
    top1 = np.where(has_nan, first_nan, first_max)
    return {'logprob': logprob.reshape(targets.shape), 'rank': rank.reshape(targets.shape), 'lse': lse, 'top1': top1,
            'entropy': entropy}


def units(x):
    """(unit of lse and logprob (rows,), unit of entropy (rows,)) for finite rows x."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=1)
    with np.errstate(all='ignore'):
        e = np.exp(x - m[:, None])
        s = e.sum(axis=1)
        lse = m + np.log(s)
        weight = np.where(e > 0, e * np.abs(x), 0.0).sum(axis=1) / s
    unit = EPS32 * (np.abs(lse) + np.abs(x).max(axis=1, initial=0.0, where=np.isfinite(x)))
    return unit, unit * (1.0 + weight)


def worst_errors(got, want, x, scored=None):
    """Largest error of `got` (dict of arrays) against `want` = score_rows(x, targets), in the units above:
    {'lse', 'logprob', 'entropy'} -> float.  Entries of logprob whose expected value is not finite are left out, and
    those outside `scored` (bool in the shape of the targets) when it is given."""
    unit, unit_ent = units(x)
    res = {}
    if 'lse' in got:
        res['lse'] = float(np.max(np.abs(np.asarray(got['lse'], dtype=np.float64) - want['lse']) / unit))
    if 'entropy' in got:
        res['entropy'] = float(np.max(np.abs(np.asarray(got['entropy'], dtype=np.float64) - want['entropy']) / unit_ent))
    if 'logprob' in got:
        lp, ref = np.asarray(got['logprob'], dtype=np.float64), want['logprob']
        rows = lp.shape[0]
        with np.errstate(invalid='ignore'):
            err = np.abs(lp - ref).reshape(rows, -1) / unit[:, None]
        keep = np.isfinite(ref).reshape(rows, -1)
        if scored is not None:
            keep = keep & np.asarray(scored).reshape(rows, -1)
        res['logprob'] = float(np.max(np.where(keep, err, 0.0)))
    return res


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def spike_rows(rows, cols, spike_cols, low=-128.0):
    """(rows, cols) float32: `low` everywhere, 0 at column spike_cols[r % len] of row r.  Then lse = entropy = 0 exactly
    (exp(low) underflows to 0 in fp32), logprob = 0 at the spike and `low` elsewhere, top1 = the spike, and the rank of a
    column t that is not the spike is 1 + t - [spike < t]."""
    x = np.full((rows, cols), low, dtype=np.float32)
    spikes = np.array([spike_cols[r % len(spike_cols)] for r in range(rows)], dtype=np.int64)
    x[np.arange(rows), spikes] = 0.0
    return x, spikes


def spike_expected(spikes, targets, cols, low=-128.0):
    """Closed form of the five outputs on spike_rows for targets (rows, M) (out-of-range ones included)."""
    targets = np.asarray(targets, dtype=np.int64)
    c = spikes[:, None]
    inside = (targets >= 0) & (targets < cols)
    hit = targets == c
    logprob = np.where(inside, np.where(hit, 0.0, low), 0.0).astype(np.float32)
    rank = np.where(inside, np.where(hit, 0, 1 + targets - (c < targets)), -1).astype(np.int32)
    rows = len(spikes)
    return {'logprob': logprob, 'rank': rank, 'lse': np.zeros(rows, np.float32), 'top1': spikes.astype(np.int32),
            'entropy': np.zeros(rows, np.float32)}


def boundary_columns(cols, head, per16):
    """Columns worth a spike for a row of `cols` elements whose first `head` elements precede the first 16-byte boundary
    (per16 elements a chunk): the ends, the head / body and body / tail seams, and the lane 0 / 63 / wave / workgroup seams of
    the body (a thread takes chunk tid + 256 n)."""
    nhead = min(head, cols)
    nvec = (cols - nhead) // per16
    tail0 = nhead + nvec * per16
    picks = {0, cols - 1, nhead - 1, nhead, tail0 - 1, tail0, cols // 2}
    for chunk in (1, 62, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512, nvec - 1):
        for inner in (0, per16 - 1):
            picks.add(nhead + chunk * per16 + inner)
    return sorted(p for p in picks if 0 <= p < cols)


def drawn_rows(rows, cols, seed, scale=3.0, minus_inf=0.0):
    """float32 rows ~ scale * N(0, 1), a fraction `minus_inf` of the entries -inf (never a whole row)."""
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal((rows, cols))).astype(np.float32)
    if minus_inf > 0:
        drop = rng.random((rows, cols)) < minus_inf
        drop[:, rng.integers(0, cols)] = False
        x[drop] = -np.inf
    return x


def drawn_targets(rows, cols, m, seed):
    """(rows, m) int64 targets: mostly inside [0, cols), with repeats, -100 and cols (outside) sprinkled in."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, cols, size=(rows, m), dtype=np.int64)
    if m > 1:
        t[:, m - 1] = t[:, 0]                                       # a repeated target
    special = rng.random((rows, m)) < 0.15
    t[special] = rng.choice(np.array([-100, -1, cols, cols + 5], dtype=np.int64), size=int(special.sum()))
    return t
