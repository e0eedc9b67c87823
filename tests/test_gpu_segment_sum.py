"""GPU: bp_segment_sum_rows (csrc/segment_sum_rows.hip) against its float64 restatement (tests/segment_sum_ref.py).
Exact where the arithmetic allows it: rows of small integers make every fp32 partial sum exact whatever the association, so
the result must be the reference bit for bit -- over the column counts, row counts and segment-length patterns at which the
kernel changes route (kSegLongRows = 32: row after row below, 16 row lanes from there; 8 rows loaded ahead on either route,
i.e. 128 per step of the 16 lanes), both `accumulate` modes, strided views, guard rows.  Random rows against the standard
bound of an fp32 sum in any order, and bit-equal reruns, also with the segments presented in another order."""
import numpy as np
import pytest
import torch

import segment_sum_ref as REF
from decode_support import DEV, _bp

pytestmark = pytest.mark.gpu

COLS = (8, 416, 12288)
N_ROWS = (1, 130, 2048)


def _lengths(pattern, n, rng):
    """Segment lengths that sum to n."""
    bp = _bp()
    if pattern == 'ones':
        return [1] * n
    if pattern == 'one':
        return [n]
    if pattern == 'empties':
        a = n // 3
        return [0, 0, a, 0, n - a, 0, 0]
    if pattern == 'skew':       # 90 % of the rows in one segment, the rest drawn over 20 more
        big = (9 * n + 9) // 10
        rest = np.bincount(rng.integers(0, 20, n - big), minlength=20).tolist()
        return rest[:7] + [big] + rest[7:]
    assert pattern == 'side'    # 63 / 64 / 65 / 257 side by side, and every size at which the kernel changes its step, +- 1
    long_rows, lanes, ahead = bp.SEGMENT_LONG_ROWS, bp.SEGMENT_ROW_LANES, bp.SEGMENT_UNROLL
    assert (long_rows, lanes, ahead) == (32, 16, 8)
    sizes = [63, 64, 65, 257]
    for part in (long_rows, lanes, ahead, lanes * ahead, long_rows + lanes * ahead):
        sizes += [part - 1, part, part + 1]
    out = []
    for size in sizes:
        if sum(out) + size > n:
            break
        out.append(size)
    return out + ([n - sum(out)] if sum(out) < n else [])


PATTERNS = ('ones', 'one', 'side', 'empties', 'skew')


def _launch(bp, rows, order, seg_begin, acc, accumulate):
    bp.segment_sum_rows(rows, torch.from_numpy(order).to(DEV), torch.from_numpy(seg_begin).to(DEV), acc, accumulate)
    return acc


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('cols', COLS)
def test_exact_on_small_integers(cols, dtype):
    bp = _bp()
    rng = np.random.default_rng(cols)
    for n in N_ROWS:
        values = rng.integers(-8, 9, (n, cols)).astype(np.float32)
        rows = torch.from_numpy(values).to(dtype).to(DEV)
        for pattern in PATTERNS:
            lengths = _lengths(pattern, n, rng)
            assert sum(lengths) == n
            order, seg_begin = REF.segments_from_lengths(lengths, rng)
            empty = torch.tensor([length == 0 for length in lengths])
            for accumulate in (False, True):
                # sentinel: small integers (exact under +=); the rows of empty segments a pattern no sum produces
                preset = torch.from_numpy(rng.integers(-5, 6, (len(lengths), cols)).astype(np.float32))
                preset[empty] = torch.tensor([-0.0, float('nan'), 3.0e38, 1.0e-40]).repeat(cols // 4)
                want, _ = REF.segment_sum_rows(values, order, seg_begin, preset.numpy(), accumulate)
                got = _launch(bp, rows, order, seg_begin, preset.to(DEV), accumulate).cpu()
                what = (n, pattern, accumulate)
                if accumulate:      # empty segments keep their row bit for bit
                    assert torch.equal(got[empty].view(torch.int32), preset[empty].view(torch.int32)), what
                else:
                    assert torch.equal(got[empty].view(torch.int32), torch.zeros_like(got[empty]).view(torch.int32)), what
                assert torch.equal(got[~empty], torch.from_numpy(want).float()[~empty]), what


@pytest.mark.parametrize('accumulate', [False, True])
def test_strided_views_and_guard_rows(accumulate):
    """rows and acc as column slices of wider buffers, acc also as a row slice: the padding columns and the guard rows in
    front of and behind acc keep their pattern."""
    bp = _bp()
    rng = np.random.default_rng(7)
    n, cols = 700, 416
    lengths = _lengths('side', n, rng) + [0]
    order, seg_begin = REF.segments_from_lengths(lengths, rng)
    values = rng.integers(-8, 9, (n, cols)).astype(np.float32)
    wide = torch.full((n, cols + 16), 99.0, dtype=torch.bfloat16, device=DEV)
    rows = wide[:, 8:8 + cols]
    rows.copy_(torch.from_numpy(values))
    guard, nseg = 2, len(lengths)
    pattern = torch.from_numpy(rng.integers(-5, 6, (nseg + 2 * guard, cols + 8)).astype(np.float32))
    whole = pattern.to(DEV)
    acc = whole[guard:guard + nseg, 4:4 + cols]
    assert rows.stride(0) == cols + 16 and acc.stride(0) == cols + 8 and acc.data_ptr() % 16 == 0
    want = pattern.clone()
    inner, _ = REF.segment_sum_rows(values, order, seg_begin, pattern[guard:guard + nseg, 4:4 + cols].numpy(), accumulate)
    want[guard:guard + nseg, 4:4 + cols] = torch.from_numpy(inner).float()
    _launch(bp, rows, order, seg_begin, acc, accumulate)
    assert torch.equal(whole.cpu(), want)


def test_order_is_clamped_and_seg_begin_is_not_trusted():
    bp = _bp()
    n, cols = 40, 136
    values = np.random.default_rng(1).integers(-8, 9, (n, cols)).astype(np.float32)
    rows = torch.from_numpy(values).bfloat16().to(DEV)
    order = np.arange(n, dtype=np.int32)
    order[[3, 17]] = (-1, 2 ** 31 - 1)
    seg_begin = np.array([-7, 5, 3, 38, 2 ** 31 - 1], dtype=np.int32)     # a decreasing pair, ends outside [0, n]
    preset = np.ones((4, cols), dtype=np.float32)
    want, _ = REF.segment_sum_rows(values, order, seg_begin, preset, False)
    got = _launch(bp, rows, order, seg_begin, torch.from_numpy(preset).to(DEV), False)
    assert torch.equal(got.cpu(), torch.from_numpy(want).float())


@pytest.fixture(scope='module')
def random_case():
    rng = np.random.default_rng(11)
    n, cols = 2048, 12288
    lengths = _lengths('skew', n - 300, rng) + [0] + _lengths('side', 300, rng)
    assert sum(lengths) == n and min(lengths) >= 0
    order, seg_begin = REF.segments_from_lengths(lengths, rng)
    rows = torch.randn(n, cols, generator=torch.Generator().manual_seed(4)).bfloat16()
    exact, magnitude = REF.segment_sum_rows(rows.float().numpy(), order, seg_begin, np.zeros((len(lengths), cols)), False)
    return dict(lengths=lengths, order=order, seg_begin=seg_begin, rows=rows.to(DEV), exact=exact, magnitude=magnitude)


def test_random_rows_within_the_bound_of_an_fp32_sum(random_case):
    """|got - exact| <= n 2^-24 sum|x_i| per element, n the segment's length: the bound of an fp32 sum in any order."""
    bp, c = _bp(), random_case
    acc = torch.full(c['exact'].shape, 5.0, device=DEV)
    got = _launch(bp, c['rows'], c['order'], c['seg_begin'], acc, False).cpu().double().numpy()
    n = np.asarray(c['lengths'], dtype=np.float64)[:, None]
    err, bound = np.abs(got - c['exact']), n * 2.0 ** -24 * c['magnitude']
    print('segment sum: max err %.3e, max err / bound %.3e' % (err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    # accumulate: one more fp32 add, of the preset and the rounded sum
    base = torch.randn(c['exact'].shape, generator=torch.Generator().manual_seed(5))
    added = _launch(bp, c['rows'], c['order'], c['seg_begin'], base.to(DEV), True).cpu()
    assert torch.equal(added, base + torch.from_numpy(got).float())


def test_reruns_and_reordered_segments_give_the_same_bits(random_case):
    bp, c = _bp(), random_case
    nseg = len(c['lengths'])
    first = _launch(bp, c['rows'], c['order'], c['seg_begin'], torch.empty(c['exact'].shape, device=DEV), False).clone()
    again = _launch(bp, c['rows'], c['order'], c['seg_begin'], torch.empty(c['exact'].shape, device=DEV), False)
    assert torch.equal(first, again)
    # the same segments in another order: order / seg_begin permuted consistently
    perm = np.random.default_rng(2).permutation(nseg)
    pieces = [c['order'][c['seg_begin'][u]:c['seg_begin'][u + 1]] for u in perm]
    order = np.concatenate(pieces).astype(np.int32)
    seg_begin = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.int32)
    moved = _launch(bp, c['rows'], order, seg_begin, torch.empty(c['exact'].shape, device=DEV), False)
    assert torch.equal(moved, first[torch.from_numpy(perm).to(DEV)])


def test_binding_checks():
    bp = _bp()
    rows = torch.zeros(6, 16, dtype=torch.bfloat16, device=DEV)
    order = torch.arange(6, dtype=torch.int32, device=DEV)
    seg_begin = torch.tensor([0, 2, 6], dtype=torch.int32, device=DEV)
    acc = torch.zeros(2, 16, device=DEV)
    assert bp.segment_sum_rows(rows, order, seg_begin, acc) is acc
    for bad in (dict(rows=rows.float()), dict(rows=rows[:, :12]), dict(rows=rows[:, 4:12]), dict(order=order.long()),
                dict(order=order[:5]), dict(seg_begin=seg_begin.long()), dict(acc=acc.bfloat16()), dict(acc=acc[:1]),
                dict(acc=torch.zeros(2, 32, device=DEV)[:, 2:18]), dict(acc=acc.cpu())):
        args = dict(rows=rows, order=order, seg_begin=seg_begin, acc=acc)
        args.update(bad)
        with pytest.raises(RuntimeError):
            bp.segment_sum_rows(**args)
