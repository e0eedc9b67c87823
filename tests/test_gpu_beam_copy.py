"""GPU: bp_beam_copy_rows (csrc/beam_copy.hip), bitwise against index_select: rows whose parent is another row take that
row's positions [first_position, length), everything else keeps its bytes."""
import pytest
import torch

import beam_ref as R
from decode_support import DEV, _bp

pytestmark = pytest.mark.gpu

POSITIONS, FIRST = 12, 5


def _parents(W, kind):
    """Parent slots of one group with parent[parent[r]] == parent[r]."""
    if kind == 'identity' or W == 1:
        return list(range(W))
    if kind == 'fan-out':                       # everything continues the last slot
        return [W - 1] * W
    half = max(W // 2, 1)                       # two disjoint fan-outs: slots below `half` from slot 0, the rest from `half`
    return [0 if t < half else half for t in range(W)]


def _sets(rows, gen):
    """Three row sets of 4, 8 and 3072 bytes a position, each inside a larger buffer: a guard row on either side, and
    for the first two a row stride wider than the positions."""
    a = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows + 2, POSITIONS + 4), generator=gen, dtype=torch.int64).to(torch.int32).to(DEV)
    b = torch.randint(-2 ** 62, 2 ** 62, (rows + 2, POSITIONS + 2), generator=gen, dtype=torch.int64).to(DEV)
    c = torch.randn((rows + 2, POSITIONS, 2, 12, 64), generator=gen).to(torch.bfloat16).to(DEV)
    wholes = [a, b, c]
    views = [a[1:-1, :POSITIONS], b[1:-1, :POSITIONS], c[1:-1]]
    assert [v[0, 0].numel() * v.element_size() for v in views] == [4, 8, 3072]
    return wholes, views


@pytest.mark.parametrize('kind', ['identity', 'fan-out', 'two fan-outs'])
@pytest.mark.parametrize('W', [1, 2, 3, 8])
def test_copy_rows_is_index_select_on_the_copied_range(W, kind):
    bp = _bp()
    groups = 4
    rows = groups * W
    gen = torch.Generator().manual_seed(17 * W + len(kind))
    parent = torch.tensor([g * W + p for g in range(groups) for p in _parents(W, kind)], dtype=torch.int32, device=DEV)
    assert torch.equal(parent[parent.long()], parent)
    pool = [0, 1, FIRST, POSITIONS, FIRST + 1, 7, POSITIONS + 3, -2]          # beyond either end: clamped
    lengths = torch.tensor([pool[(r + r // W) % len(pool)] for r in range(rows)], dtype=torch.int32, device=DEV)
    wholes, views = _sets(rows, gen)
    # the reference is tests/beam_ref.py's numpy restatement on host copies (bf16 as its bits), independent of both of the
    # project's paths; the clamp of the lengths is restated there and once more, by index_select, below
    want = [w.cpu().view(torch.int16 if w.dtype == torch.bfloat16 else w.dtype).numpy().copy() for w in wholes]
    inner = [want[0][1:-1, :POSITIONS], want[1][1:-1, :POSITIONS], want[2][1:-1]]
    for view, new in zip(inner, R.copy_rows(inner, parent.cpu().numpy(), lengths.cpu().numpy(), FIRST)):
        view[...] = new
    want = [torch.from_numpy(w).to(DEV).view(whole.dtype) for w, whole in zip(want, wholes)]
    for ref, old in zip([want[0][1:-1, :POSITIONS], want[1][1:-1, :POSITIONS], want[2][1:-1]], views):
        for r in range(rows):
            n = min(max(int(lengths[r]), 0), POSITIONS)
            as_int = torch.int16 if old.dtype == torch.bfloat16 else old.dtype
            assert torch.equal(ref[r, FIRST:n].view(as_int), old.index_select(0, parent.long())[r, FIRST:n].view(as_int))
    before = [w.clone() for w in wholes]
    bp.beam_copy_rows(views, parent, lengths, FIRST)
    torch.cuda.synchronize()
    moved = False
    for got, ref, old in zip(wholes, want, before):
        as_int = torch.int16 if got.dtype == torch.bfloat16 else got.dtype
        assert torch.equal(got.view(as_int), ref.view(as_int))
        moved = moved or not torch.equal(ref.view(as_int), old.view(as_int))
        keep = (parent == torch.arange(rows, device=DEV)).nonzero().flatten() + 1
        assert torch.equal(got[keep].view(as_int), old[keep].view(as_int))       # rows that name themselves: untouched
        assert torch.equal(got[:, :FIRST].view(as_int), old[:, :FIRST].view(as_int))
    ar = torch.arange(rows, device=DEV)
    assert moved == bool(((parent != ar) & (lengths.clamp(0, POSITIONS) > FIRST)).any())
    assert moved or kind == 'identity' or W < 3


def test_copy_rows_refuses_more_than_32_sets_and_bad_layouts():
    bp = _bp()
    parent = torch.zeros(2, dtype=torch.int32, device=DEV)
    t = torch.zeros(2, 8, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match='32'):
        bp.beam_copy_rows([t] * 33, parent, parent, 0)
    with pytest.raises(RuntimeError, match='shape'):
        bp.beam_copy_rows([torch.zeros(2, 8, dtype=torch.int16, device=DEV)], parent, parent, 0)   # 2 bytes a position
    with pytest.raises(RuntimeError, match='shape'):
        bp.beam_copy_rows([torch.zeros(2, 9, dtype=torch.int32, device=DEV)], parent, parent, 0)   # 36-byte rows
    bp.beam_copy_rows([t] * 32, parent, parent, 0)
    torch.cuda.synchronize()
