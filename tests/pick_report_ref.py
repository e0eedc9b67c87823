"""Float64 numpy restatement of bp_pick_report (contract: include/bp_hip.h), shared by tests/test_pick_report_host.py and
tests/test_gpu_pick_report.py.

Per row b with c = counters[b], t = tokens[b] and x the logits as float64 (the conversion of an element is exact):
  c outside [0, cols)   the row writes nothing
  logprob, rank, entropy, lse   tests/score_ref.py:score_rows with the one target t
  top_idx[b, c, i]      the column of position i in the order (x descending with -0 == +0, a NaN above every number, column
                        ascending); top_logprob[b, c, i] = x - lse of that element
The record arrays are updated in place, like the kernel's buffers: what a row does not write keeps its value.
"""
import numpy as np

import score_ref

RECORDS = ('logprob', 'rank', 'entropy', 'top_idx', 'top_logprob')
INITIAL = {'logprob': 0.0, 'rank': -1, 'entropy': 0.0, 'top_idx': -1, 'top_logprob': 0.0}
DTYPES = {'logprob': np.float64, 'rank': np.int64, 'entropy': np.float64, 'top_idx': np.int64, 'top_logprob': np.float64}


def top_order(x, n):
    """(rows, n) columns of the n first elements of every row in the order of the contract."""
    x = np.asarray(x, dtype=np.float64)
    nan = np.isnan(x)
    # classes: NaN 2, numbers by value (+0.0 folds -0), so a lexicographic sort on (class, value) descending, column ascending
    value = np.where(nan, 0.0, x) + 0.0
    cols = np.arange(x.shape[1])
    out = np.empty((x.shape[0], n), dtype=np.int64)
    for r in range(x.shape[0]):
        order = np.lexsort((cols, -value[r], ~nan[r]))             # last key first: NaNs, then value descending, then column
        out[r] = order[:n]
    return out


def row_report(x, tokens, n_top=0):
    """Every row's record as if its column existed: dict of logprob, rank, entropy, lse (rows,), top_idx, top_logprob (rows, n_top)."""
    x = np.asarray(x, dtype=np.float64)
    got = score_ref.score_rows(x, np.asarray(tokens, dtype=np.int64).reshape(-1))
    res = {n: got[n] for n in ('logprob', 'rank', 'entropy', 'lse')}
    idx = top_order(x, n_top)
    with np.errstate(invalid='ignore'):
        res['top_idx'], res['top_logprob'] = idx, np.take_along_axis(x, idx, axis=1) - got['lse'][:, None]
    return res


def new_records(rows, cols, n_top=0, names=RECORDS):
    """Record arrays at their initial values: floats 0, ranks and ids -1."""
    return {n: np.full((rows, cols, n_top) if n.startswith('top_') else (rows, cols), INITIAL[n], dtype=DTYPES[n])
            for n in names if n_top or not n.startswith('top_')}


def pick_report(x, tokens, counters, records):
    """Update `records` (dict of arrays of new_records' shapes, any subset) in place with the picks of one step."""
    counters = np.asarray(counters, dtype=np.int64)
    tops = [v for n, v in records.items() if n.startswith('top_')]
    n_top = tops[0].shape[2] if tops else 0
    cols = next(iter(records.values())).shape[1]
    rep = row_report(x, tokens, n_top)
    for b, c in enumerate(counters):
        if 0 <= c < cols:
            for n, v in records.items():
                v[b, c] = rep[n][b]
    return records


def same_floats(a, b):
    """Equal as extended reals: NaN where NaN, the same infinities, equal numbers (a test of exact equality)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b)))
