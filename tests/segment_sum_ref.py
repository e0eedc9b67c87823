"""numpy float64 restatement of bp_segment_sum_rows (include/bp_hip.h): acc[u] (= or +=) the sum of rows[order[i]] over
i in [seg_begin[u], seg_begin[u + 1]), with the entry point's clamps -- seg_begin to [0, n_rows], a decreasing pair an empty
segment, order unsigned to n_rows - 1 -- and its two modes: accumulate=False overwrites (an empty segment writes zeros),
accumulate=True adds (an empty segment leaves its row alone).  Shared by the host test and the GPU tests."""
import numpy as np


def segment_sum_rows(rows, order, seg_begin, acc, accumulate=False):
    """rows (n_rows, cols) of any float dtype, order (n_rows,) ints, seg_begin (n_segments + 1,) ints, acc (n_segments, cols):
    returns (sums float64 like acc, abs_sums float64: the same sums over |rows|, for error bounds, WITHOUT acc)."""
    rows = np.asarray(rows, dtype=np.float64)
    order = np.asarray(order).astype(np.int64)
    seg_begin = np.asarray(seg_begin).astype(np.int64)
    n_rows = rows.shape[0]
    out = np.array(acc, dtype=np.float64, copy=True)
    abs_sums = np.zeros_like(out)
    clamped = np.minimum(order.astype(np.uint32).astype(np.int64), max(n_rows - 1, 0))
    for u in range(seg_begin.shape[0] - 1):
        begin = min(max(int(seg_begin[u]), 0), n_rows)
        end = min(max(int(seg_begin[u + 1]), begin), n_rows)
        if begin == end:
            if not accumulate:
                out[u] = 0.0
            continue
        picked = rows[clamped[begin:end]]
        total = picked.sum(axis=0)
        out[u] = out[u] + total if accumulate else total
        abs_sums[u] = np.abs(picked).sum(axis=0)
    return out, abs_sums


def segments_from_lengths(lengths, rng=None):
    """(order, seg_begin) for segments of the given lengths over n_rows = sum(lengths) rows: the rows are dealt to the
    segments at random (`rng`, a numpy Generator) or in turn, and listed ascending inside every segment."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n_rows = int(lengths.sum())
    owner = np.repeat(np.arange(lengths.shape[0]), lengths)
    if rng is not None:
        owner = rng.permutation(owner)
    order = np.argsort(owner, kind='stable').astype(np.int32)
    seg_begin = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    assert seg_begin[-1] == n_rows
    return order, seg_begin
