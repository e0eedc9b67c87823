"""GPU: bp_scatter_packed_rows (csrc/scatter_rows.hip), exact.  The checker restates the contract of include/bp_hip.h byte by
byte in torch on the CPU, on uint8 views of the WHOLE buffers a destination is a slice of: every byte the call must not touch
-- the guard samples around the slice, positions at or behind a sequence's end, the padding between rows -- is compared too."""
import pytest
import torch

from decode_support import DEV, _bp

pytestmark = pytest.mark.gpu

CHUNK = 32              # positions a workgroup owns (bp_hip.SCATTER_POSITIONS, asserted): lengths straddle it
LENGTHS = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 3, 3 * CHUNK + 1)
POSITIONS = 3 * CHUNK + 4
GUARD = 2               # samples of the whole cache in front of the slice (one more behind it)

# (row bytes, source row stride, offset of the source in its buffer, padding behind a destination row), bytes.  Row stride
# 1.5 x the row wherever that is a multiple of 4 (qkv[:, 1:] of (total, 3, H, D)), else 2 x.  The 16-byte path needs all
# of a set's numbers to be multiples of 16: 16 and 48 come both ways.
SPECS = [(4, 8, 4, 0), (8, 12, 4, 0), (12, 24, 12, 0), (16, 24, 8, 0), (16, 32, 16, 0), (48, 72, 24, 16), (48, 96, 48, 16),
         (3072, 4608, 1536, 0)]


def _bytes(n, gen):
    return torch.randint(1, 256, (n,), generator=gen, dtype=torch.uint8).to(DEV)      # no zero byte: a skipped write shows


class _Case:
    """Sources of `total` rows and destinations of `batch` samples inside larger buffers, by SPECS-like tuples."""

    def __init__(self, specs, batch, total, positions, seed):
        gen = torch.Generator().manual_seed(seed)
        self.batch, self.total, self.positions = batch, total, positions
        self.src_bufs, self.dst_bufs, self.pairs, self.layout = [], [], [], []
        for rb, stride, offset, pad in specs:
            sbuf = _bytes(total * stride, gen)
            dbuf = _bytes((batch + GUARD + 1) * positions * (rb + pad), gen)
            whole = sbuf.view(torch.int32).view(total, stride // 4)
            src = whole[:, offset // 4:(offset + rb) // 4]
            dst = dbuf.view(torch.int32).view(batch + GUARD + 1, positions, (rb + pad) // 4)[GUARD:GUARD + batch, :, :rb // 4]
            if rb == 3072:      # the trunk's shapes: (total, 3, H, D)[:, 1:] into (batch, positions, 2, H, D)
                src = sbuf.view(torch.int32).view(total, 3, 12, 32)[:, 1:]
                dst = dst.view(batch, positions, 2, 12, 32)
            assert src.stride(0) * 4 == stride and src[0].numel() * 4 == rb and dst.stride(1) * 4 == rb + pad
            self.src_bufs.append(sbuf)
            self.dst_bufs.append(dbuf)
            self.pairs.append((src, dst))
            self.layout.append((rb, stride, src.data_ptr() - sbuf.data_ptr(), dst.data_ptr() - dbuf.data_ptr(),
                                dst.stride(0) * 4, dst.stride(1) * 4))
        self.pattern = [d.clone() for d in self.dst_bufs]

    def reset(self):
        for d, p in zip(self.dst_bufs, self.pattern):
            d.copy_(p)

    def want(self, cu, max_seqlen, max_positions=None):
        """The destinations' whole buffers by the contract, as uint8 on the CPU."""
        max_positions = self.positions if max_positions is None else max_positions
        out = []
        for sbuf, pattern, (rb, ss, soff, doff, bs, ps) in zip(self.src_bufs, self.pattern, self.layout):
            src, dst = sbuf.cpu(), pattern.cpu().clone()
            for b in range(self.batch):
                n = min(max(cu[b + 1] - cu[b], 0), max_seqlen, max_positions)
                for j in range(n):
                    t = cu[b] + j
                    if 0 <= t < self.total:
                        dst[doff + b * bs + j * ps:doff + b * bs + j * ps + rb] = src[soff + t * ss:soff + t * ss + rb]
            out.append(dst)
        return out

    def check(self, want, changed=True):
        torch.cuda.synchronize()
        for i, (got, ref, old) in enumerate(zip(self.dst_bufs, want, self.pattern)):
            assert torch.equal(got.cpu(), ref), f'set {i} {self.layout[i]}'
            assert torch.equal(ref, old.cpu()) != changed, f'set {i}: a weak case'


def _cu(lengths):
    out = [0]
    for n in lengths:
        out.append(out[-1] + n)
    return out


def _dev(cu):
    return torch.tensor(cu, dtype=torch.int32, device=DEV)


@pytest.fixture(scope='module')
def case():
    assert _bp().SCATTER_POSITIONS == CHUNK
    return _Case(SPECS, len(LENGTHS), sum(LENGTHS), POSITIONS, seed=5)


def test_rows_land_at_their_samples_positions_and_nothing_else_is_written(case):
    bp = _bp()
    cu = _cu(LENGTHS)
    case.reset()
    bp.scatter_packed_rows(case.pairs, _dev(cu), max(LENGTHS))
    case.check(case.want(cu, max(LENGTHS)))
    # the restatement against torch's own indexing, once: sample 4 of the 3072-byte set
    src, dst = case.pairs[-1]
    b = 4
    assert torch.equal(dst[b, :LENGTHS[b]], src[cu[b]:cu[b + 1]]) and LENGTHS[b] == CHUNK + 1
    # a longer max_seqlen than any sequence changes nothing; twice is once
    bp.scatter_packed_rows(case.pairs, _dev(cu), POSITIONS)
    case.check(case.want(cu, max(LENGTHS)))


def test_a_length_is_clamped_to_max_positions_and_to_max_seqlen(case):
    bp = _bp()
    cu = _cu(LENGTHS)
    # destinations of fewer positions than the longest sequence: the same buffers, cut
    short = CHUNK + 8
    case.reset()
    bp.scatter_packed_rows([(s, d[:, :short]) for s, d in case.pairs], _dev(cu), max(LENGTHS))
    want = case.want(cu, max(LENGTHS), max_positions=short)
    case.check(want)
    assert not all(torch.equal(a, b) for a, b in zip(want, case.want(cu, max(LENGTHS))))
    # one destination decides for all
    case.reset()
    bp.scatter_packed_rows([(s, d[:, :short] if i == 2 else d) for i, (s, d) in enumerate(case.pairs)], _dev(cu), max(LENGTHS))
    case.check(want)
    for max_seqlen in (CHUNK - 5, 1):
        case.reset()
        bp.scatter_packed_rows(case.pairs, _dev(cu), max_seqlen)
        case.check(case.want(cu, max_seqlen))
    case.reset()
    bp.scatter_packed_rows(case.pairs, _dev(cu), 0)
    case.check(case.want(cu, 0), changed=False)


def test_cu_seqlens_is_not_trusted(case):
    """Negative lengths count as 0, rows outside the source are skipped, lengths beyond the destination are clamped: the
    kernel checks every row index against [0, total_rows) and every position against the clamped length."""
    bp = _bp()
    total = case.total
    for cu in ([0, 40, 10, 10, 30, 25, total, total],                  # decreasing entries: negative lengths
               [0, 5, 5, 5, total - 3, total + 500, total + 501, total + 600],      # rows behind the source's end
               [-7, 2, 2, 2, 2, 2, 2, 2]):                             # rows in front of its begin
        case.reset()
        bp.scatter_packed_rows(case.pairs, _dev(cu), POSITIONS + 50)
        case.check(case.want(cu, POSITIONS + 50))


def test_32_sets_in_one_call_and_the_refusals():
    bp = _bp()
    lengths = (3, 0, 5)
    cu = _cu(lengths)
    many = _Case([(4 * (1 + i % 5), 8 * (1 + i % 5), 0, 4 * (i % 2)) for i in range(32)], len(lengths), sum(lengths), 6, seed=9)
    bp.scatter_packed_rows(many.pairs, _dev(cu), 5)
    many.check(many.want(cu, 5))
    src, dst = many.pairs[1]                                           # 8-byte rows
    with pytest.raises(RuntimeError, match='32'):
        bp.scatter_packed_rows(many.pairs + [many.pairs[0]], _dev(cu), 5)
    with pytest.raises(RuntimeError, match='32'):
        bp.scatter_packed_rows([], _dev(cu), 5)
    halves = torch.zeros(8, 1, dtype=torch.int16, device=DEV)
    with pytest.raises(RuntimeError, match='shape'):                   # 2-byte rows
        bp.scatter_packed_rows([(halves, torch.zeros(3, 6, 1, dtype=torch.int16, device=DEV))], _dev(cu), 5)
    six = torch.zeros(8, 3, dtype=torch.int16, device=DEV)
    with pytest.raises(RuntimeError, match='shape'):                   # 4-byte rows at a 6-byte stride
        bp.scatter_packed_rows([(six[:, 1:], torch.zeros(3, 6, 2, dtype=torch.int16, device=DEV))], _dev(cu), 5)
    with pytest.raises(RuntimeError, match='shape'):                   # rows that overlap: a stride below the row
        bp.scatter_packed_rows([(src[:1].expand(8, -1), dst)], _dev(cu), 5)
    with pytest.raises(RuntimeError, match='shape'):                   # negative max_seqlen
        bp.scatter_packed_rows([(src, dst)], _dev(cu), -1)
    with pytest.raises(RuntimeError, match='shape'):                   # 65536 samples
        bp.scatter_packed_rows([(src, torch.zeros(65536, 1, src.shape[1], dtype=torch.int32, device=DEV))],
                               torch.zeros(65537, dtype=torch.int32, device=DEV), 1)
    gaps = torch.zeros(8, 2 * src.shape[1], dtype=torch.int32, device=DEV)[:, ::2]      # a row that is not contiguous
    for bad in ([(src, dst.to(torch.float32))], [(src, dst[:, :, :0])], [(src[:, None], dst)], [(src, dst[:2])],
                [(src[:5], dst), (src, dst)], [(gaps, dst)], [(src, dst.cpu().to(DEV).transpose(0, 1))]):
        with pytest.raises(RuntimeError, match='scatter_packed_rows'):
            bp.scatter_packed_rows(bad, _dev(cu), 5)
    with pytest.raises(RuntimeError, match='cu_seqlens'):
        bp.scatter_packed_rows([(src, dst)], _dev(cu).long(), 5)
    many.check(many.want(cu, 5))                                       # no refused call wrote anything


def test_a_captured_call_reads_the_lengths_of_the_replay(case):
    bp = _bp()
    first = _cu(LENGTHS)
    other = _cu((CHUNK + 1, 2, 0, CHUNK, 7, 2 * CHUNK, 5))
    assert other[-1] <= case.total and max(other[i + 1] - other[i] for i in range(len(LENGTHS))) <= max(LENGTHS)
    cu = _dev(first)
    case.reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bp.scatter_packed_rows(case.pairs, cu, max(LENGTHS))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bp.scatter_packed_rows(case.pairs, cu, max(LENGTHS))
    case.reset()
    cu.copy_(_dev(other))
    graph.replay()
    want = case.want(other, max(LENGTHS))
    case.check(want)
    assert not all(torch.equal(a, b) for a, b in zip(want, case.want(first, max(LENGTHS))))
