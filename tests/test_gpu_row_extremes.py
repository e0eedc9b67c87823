"""GPU: bp_row_extremes (csrc/row_extremes.hip) against the numpy restatement of tests/sense_vocab_ref.py, bit for bit: the
columns equal, the values equal as bits.  The contract is a total order on integers, so nothing is left to a tolerance.

Sizes: the 16-byte chunk edges (7, 8, 9), the edges of one full 1024-thread step for both element widths (4095 .. 4097 for
fp32, 8191 .. 8193 for the 16-bit types) and Small's vocabulary.  Every output lies between canaries."""
import ctypes

import numpy as np
import pytest
import torch

import sense_vocab_ref as R
from decode_support import DEV, _bp
from test_gpu_beam_pick import _assert_every_boundary_kind, _edge_classes

pytestmark = pytest.mark.gpu

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
COLS = [1, 7, 8, 9, 4095, 4096, 4097, 8191, 8192, 8193, 50264]
NS = [1, 2, 20, 64]
GUARD = 8
WAVES = 16


def _ns(cols):
    return [n for n in NS if n <= cols]


def _place(x, dtype, layout):
    """(rows, cols) host fp32 -> a device view of `dtype`.  'dense'; 'phases': an odd row stride and a base one element
    behind a 16-byte boundary, so consecutive rows start at every 16-byte phase; ('head', h): every row h elements behind
    a 16-byte boundary."""
    rows, cols = x.shape
    if layout == 'dense':
        pad, mis = 0, 0
    elif layout == 'phases':
        pad, mis = 1 + (cols % 2), 1
    else:
        n = 16 // torch.empty(0, dtype=dtype).element_size()
        pad, mis = (-cols) % n + n, layout[1]
    flat = torch.zeros(rows * (cols + pad) + 32, dtype=dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = flat[mis:mis + rows * (cols + pad)].view(rows, cols + pad)[:, :cols]
    view.copy_(x.to(dtype))
    if layout == 'phases' and rows >= 8:
        per16 = 16 // view.element_size()
        assert len({(view.data_ptr() // view.element_size() + r * view.stride(0)) % per16 for r in range(rows)}) == per16
    return view


def _outputs(rows, n):
    """Four (rows, n) outputs, each between two runs of GUARD canaries: (views, whole buffers)."""
    views, wholes = [], []
    for dt, canary in ((torch.float32, -777.0), (torch.int32, -9), (torch.float32, -777.0), (torch.int32, -9)):
        whole = torch.full((rows * n + 2 * GUARD,), canary, dtype=dt, device=DEV)
        wholes.append((whole, canary))
        views.append(whole[GUARD:GUARD + rows * n].view(rows, n))
    return views, wholes


def _run(logits, n, largest=True, smallest=True):
    """bp_hip.row_extremes into guarded outputs: numpy (top_val, top_idx, bot_val, bot_idx), None for a skipped end."""
    bp = _bp()
    rows = logits.shape[0]
    views, wholes = _outputs(rows, n)
    before = logits.clone()
    out = bp.row_extremes(logits, n, largest=largest, smallest=smallest, out=views)
    torch.cuda.synchronize()
    assert torch.equal(logits.view(torch.int16 if logits.element_size() == 2 else torch.int32),
                       before.view(torch.int16 if logits.element_size() == 2 else torch.int32)), 'logits are only read'
    for (whole, canary), view, wanted in zip(wholes, views, (largest, largest, smallest, smallest)):
        assert (whole[:GUARD] == canary).all() and (whole[GUARD + rows * n:] == canary).all(), 'canaries around the outputs'
        if not wanted:
            assert (view == canary).all(), 'a skipped end is not written'
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def _assert_same(got, want, what, rows=None, n=None):
    for g, w, name in zip(got, want, ('top_val', 'top_idx', 'bot_val', 'bot_idx')):
        w = w[:rows, :n]
        if 'val' in name:
            same = R.bits_of(g) == R.bits_of(w)
        else:
            same = g == w
        assert same.all(), (what, name, np.argwhere(~same)[:4].tolist())


_DRAWN = {}


def _drawn(cols, dtype):
    """37 drawn rows of `cols` columns placed at every 16-byte phase, and their reference at n = min(cols, 64): computed
    once and shared.  A smaller n is a prefix of a larger one (the order is total), fewer rows are the first rows."""
    if (cols, dtype) not in _DRAWN:
        g = torch.Generator().manual_seed(cols)
        x = torch.randn(37, cols, generator=g) * 3
        if cols >= 4095:
            x[5, 100:100 + 2000] = x[5].max() + 1      # a plateau at the top: more ties than n, across lanes and steps
            x[6, cols - 3000:] = x[6].min() - 1        # and one at the bottom that ends with the row
        logits = _place(x, DTYPES[dtype], 'phases')
        _DRAWN[(cols, dtype)] = (logits, R.row_extremes(logits, min(cols, 64)))
    return _DRAWN[(cols, dtype)]


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('cols', COLS)
def test_drawn_rows_match_the_restatement_bit_for_bit(cols, dtype):
    logits, want = _drawn(cols, dtype)
    if dtype != 'fp32' and cols == 50264:
        keys = R.ordered_key(*R.raw_bits(logits))
        assert min(len(np.unique(row)) for row in keys) < cols - 1000, '16-bit drawn rows hold thousands of exact ties'
    for rows in (1, 3, 37):
        for n in _ns(cols):
            _assert_same(_run(logits[:rows], n), want, (cols, dtype, rows, n), rows, n)
    n = _ns(cols)[-1]
    first, again = _run(logits, n), _run(logits, n)
    for a, b in zip(first, again):
        assert (a.view(np.int32) == b.view(np.int32)).all(), 'two calls give the same bits'


@pytest.mark.parametrize('dtype', sorted(DTYPES))
def test_many_rows_of_a_thousand_columns(dtype):
    g = torch.Generator().manual_seed(8192)
    logits = _place(torch.randn(8192, 1000, generator=g) * 2, DTYPES[dtype], 'phases')
    want = R.row_extremes(logits, 20)
    for n in (1, 20):
        _assert_same(_run(logits, n), want, (dtype, n), 8192, n)


@pytest.mark.parametrize('dtype', sorted(DTYPES))
def test_constant_rows_return_the_first_columns_at_both_ends(dtype):
    for cols in COLS:
        logits = _place(torch.full((3, cols), -1.625), DTYPES[dtype], 'phases')
        for n in _ns(cols):
            tv, ti, bv, bi = _run(logits, n)
            want = np.tile(np.arange(n, dtype=np.int32), (3, 1))
            assert (ti == want).all() and (bi == want).all(), (cols, n)
            assert (tv == -1.625).all() and (bv == -1.625).all()


@pytest.mark.parametrize('dtype', sorted(DTYPES))
def test_signed_zeros_infinities_and_two_valued_rows(dtype):
    g = torch.Generator().manual_seed(5)
    pool = torch.tensor([0.0, -0.0, float('inf'), -float('inf'), 1.0, -1.0])
    for cols in (9, 4097, 8193):
        x = torch.cat([pool[torch.randint(0, len(pool), (4, cols), generator=g)],
                       torch.where(torch.rand(4, cols, generator=g) < 0.5, 0.75, -2.5)])
        logits = _place(x, DTYPES[dtype], 'phases')
        for n in _ns(cols):
            _assert_same(_run(logits, n), R.row_extremes(logits, n), (cols, dtype, n))


def _needle_columns(cols, dtype, head):
    """Columns to plant at: the first and the last, and both sides of chunk edges -- every edge of a small row, else the
    edges that stand for every kind of boundary between two (wave, step, lane) owners (test_gpu_beam_pick._edge_classes)."""
    n = 4 if dtype == 'fp32' else 8
    nch = (cols + head + n - 1) // n
    cpw = (nch + WAVES - 1) // WAVES
    edges = set(range(1, nch))
    if nch > 40:
        edges = _edge_classes(nch, cpw) | {1, nch - 1}
        _assert_every_boundary_kind(edges, nch, cpw)
    columns = {0, cols - 1}
    for c in edges:
        columns |= {c * n - head - 1, c * n - head}
    return sorted(v for v in columns if 0 <= v < cols)


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('cols', COLS)
def test_a_needle_is_found_wherever_it_lies(cols, dtype):
    head = {'bf16': 3, 'fp16': 5, 'fp32': 1}[dtype]
    columns = _needle_columns(cols, dtype, head)
    rows = len(columns)
    g = torch.Generator().manual_seed(cols + 1)
    x = torch.rand(rows, cols, generator=g) * 2 - 1
    high = np.array(columns)
    low = np.roll(high, rows // 2)                                      # the small needle elsewhere in the same row
    x[torch.arange(rows), torch.from_numpy(high)] = 100.0
    if cols > 1:
        x[torch.arange(rows), torch.from_numpy(low)] = -100.0
    logits = _place(x, DTYPES[dtype], ('head', head))
    assert logits.stride(0) * logits.element_size() % 16 == 0 and logits.data_ptr() % 16 == head * logits.element_size()
    some = slice(0, rows, max(1, rows // 12))                          # the whole answer of a few rows against the restatement
    for n in _ns(cols)[:3]:
        tv, ti, bv, bi = _run(logits, n)
        assert (ti[:, 0] == high).all() and (tv[:, 0] == 100.0).all(), (cols, dtype, n)
        if cols > 1:
            assert (bi[:, 0] == low).all() and (bv[:, 0] == -100.0).all(), (cols, dtype, n)
        _assert_same((tv[some], ti[some], bv[some], bi[some]), R.row_extremes(logits[some], n), (cols, dtype, n))


def test_null_outputs_skip_an_end():
    bp = _bp()
    logits, want = _drawn(8193, 'bf16')
    for n in (1, 20):
        tv, ti, bv, bi = _run(logits, n, smallest=False)
        assert bv is None and bi is None
        _assert_same((tv, ti), want[:2], ('largest only', n), 37, n)
        tv, ti, bv, bi = _run(logits, n, largest=False)
        assert tv is None and ti is None
        _assert_same((bv, bi), want[2:], ('smallest only', n), 37, n)
        # the C ABI takes any of the four as NULL: only the columns of the top end
        idx = torch.full((37, n), -9, dtype=torch.int32, device=DEV)
        code = bp.lib().bp_row_extremes(logits.data_ptr(), None, idx.data_ptr(), None, None, 37, 8193, logits.stride(0), n, 1,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert code == 0 and (idx.cpu().numpy() == want[1][:, :n]).all()
    assert bp.row_extremes_supported(logits, 20) and not bp.row_extremes_supported(logits, 65)
    assert not bp.row_extremes_supported(logits.double(), 2) and not bp.row_extremes_supported(logits[0], 2)
    with pytest.raises(RuntimeError, match='BP_ERR_SHAPE|shape|-3'):
        bp.row_extremes(logits, 65)


def test_a_captured_call_replays_on_new_rows():
    bp = _bp()
    g = torch.Generator().manual_seed(77)
    logits = _place(torch.randn(5, 4097, generator=g), torch.float16, 'phases')
    views, _ = _outputs(5, 20)
    bp.row_extremes(logits, 20, out=views)                             # loads the code object outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bp.row_extremes(logits, 20, out=views)
    logits.copy_((torch.randn(5, 4097, generator=g) * 4).half())
    graph.replay()
    torch.cuda.synchronize()
    _assert_same(tuple(v.cpu().numpy() for v in views), R.row_extremes(logits, 20), 'replay')
