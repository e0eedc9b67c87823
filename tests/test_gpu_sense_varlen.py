"""GPU: the sense kernels on packed batches (bp_sense_lse_varlen, bp_sense_mix_varlen, bp_sense_mix_gather_varlen).

A sample of a packed batch must come out with the BITS of the fixed-length entry points on that sample alone: the packed job
runs the same key tiles in the same order at seqlen = its own length (csrc/sense_mix_dma_kernel.h).  That equality is the main
assertion; the 2x rule against the fp32 oracle anchors it independently.  Ownership: operands and output sit inside
NaN-filled buffers with guard rows in front and behind (the last sample ends at the last row before the guard), guards keep
their bits, and a sample that is ALL NaN leaves every other sample's bits alone.  Lengths are chosen around what the kernel
tiles by: 32-row waves, 64-key tiles, 256-query jobs; max_seqlen both the longest length and 1024 (many empty tickets)."""
import ctypes

import pytest
import torch

import prefill_needles as P
from decode_support import DEV, _bp, _same_bits
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu


def rel_check(got, ref32, eager16, name, factor=2.0, atol=1e-5):
    """The project's 2x rule, as tests/test_gpu_kernels.py states it."""
    err = (got.float().cpu() - ref32.float().cpu()).abs().max().item()
    base = (eager16.float().cpu() - ref32.float().cpu()).abs().max().item()
    print(f'{name}: kernel err {err:.3e}  eager-same-dtype err {base:.3e}')
    assert err <= factor * base + atol, f'{name}: {err} > {factor} * {base}'
    assert torch.isfinite(got.float()).all()


DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ['bf16', 'fp16']
SHAPES = [(4, 16, 64), (16, 48, 288), (2, 128, 256)]     # (k, d_k, d_out); 288 columns: two chunks, one of them partial
SHAPE_IDS = ['k4_dk16_d64', 'k16_dk48_d288', 'k2_dk128_d256']
NINE = [1, 257, 64, 513, 33, 0, 256, 641, 2]
LENGTH_SETS = {                                           # name -> (lengths, max_seqlen)
    'nine': (NINE, 641),
    'nine_max1024': (NINE, 1024),
    'six': ([255, 65, 320, 31, 63, 321], 321),
    'equal': ([300, 300], 300),
    'single': ([130], 130),
    'single_max1024': ([130], 1024),
}
GUARD = 8
NAN = float('nan')


def _cu(lengths):
    return torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32, device=DEV)


def _guarded(x, fill=NAN):
    """x (total, ...) as rows GUARD .. GUARD + total of a `fill`-filled buffer: (buffer, view)."""
    buf = torch.full((x.shape[0] + 2 * GUARD,) + tuple(x.shape[1:]), fill, dtype=x.dtype, device=DEV)
    view = buf[GUARD:GUARD + x.shape[0]]
    view.copy_(x)
    return buf, view


_cases = {}


def _case(shape, dtype, name):
    """The packed operands of one (shape, dtype, length set), their outputs and the fixed-length results per sample; built
    once and left unchanged."""
    key = (shape, dtype, name)
    if key in _cases:
        return _cases[key]
    bp = _bp()
    (k, dk, dout), (lengths, max_seqlen) = shape, LENGTH_SETS[name]
    total = sum(lengths)
    g = torch.Generator().manual_seed(total + dk)
    qk_buf, qk = _guarded((torch.randn(total, 2, k, dk, generator=g) * 1.2).to(dtype).to(DEV))
    c_buf, content = _guarded(torch.randn(total, k, dout, generator=g).to(dtype).to(DEV))
    out_buf, out = _guarded(torch.zeros(total, dout, dtype=dtype, device=DEV))
    before = [t.clone() for t in (qk_buf, c_buf, out_buf)]
    cu = _cu(lengths)
    lse = bp.sense_lse_varlen(qk, cu, max_seqlen)
    bp.sense_mix_varlen(qk, content, cu, max_seqlen, out=out)
    torch.cuda.synchronize()
    fixed = []
    for b, n in enumerate(lengths):
        lo = int(cu[b])
        fixed.append(None if n == 0 else (bp.sense_lse(qk[lo:lo + n][None]), bp.sense_mix(qk[lo:lo + n][None], content[lo:lo + n][None])))
    _cases[key] = dict(qk=qk, content=content, out=out, lse=lse, cu=cu, lengths=lengths, max_seqlen=max_seqlen, fixed=fixed,
                       bufs=(qk_buf, c_buf, out_buf), before=before)
    return _cases[key]


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('name', list(LENGTH_SETS))
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_every_sample_has_the_bits_of_the_fixed_length_call(shape, name, dtype):
    c = _case(shape, dtype, name)
    assert c['lse'].shape == (len(c['lengths']), shape[0], -(-c['max_seqlen'] // 16) * 16)
    for b, n in enumerate(c['lengths']):
        if n == 0:
            continue
        lo = int(c['cu'][b])
        want_lse, want = c['fixed'][b]
        assert _same_bits(c['lse'][b, :, :n].contiguous(), want_lse[0, :, :n].contiguous()), f'lse of sample {b} (length {n})'
        assert _same_bits(c['out'][lo:lo + n], want[0]), f'sample {b} (length {n})'
    # guards and operands keep their bits; only the output rows were written
    qk_buf, c_buf, out_buf = c['bufs']
    assert _same_bits(qk_buf, c['before'][0]) and _same_bits(c_buf, c['before'][1])
    assert _same_bits(out_buf[:GUARD], c['before'][2][:GUARD]) and _same_bits(out_buf[-GUARD:], c['before'][2][-GUARD:])
    assert torch.isfinite(c['out'].float()).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('name', ['nine', 'six'])
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_every_sample_is_within_twice_the_eager_error_of_the_oracle(shape, name, dtype):
    c = _case(shape, dtype, name)
    qk, content, out = c['qk'].cpu(), c['content'].cpu(), c['out'].cpu()
    for b, n in enumerate(c['lengths']):
        if n == 0:
            continue
        lo = int(c['cu'][b])
        q, ct = qk[lo:lo + n][None], content[lo:lo + n][None].transpose(1, 2)
        rel_check(out[lo:lo + n][None], R.sense_mix_from_qk_fp32(q, ct), R.sense_mix(R.sense_alpha_from_qk(q), ct),
                  f'varlen {shape} {name} {dtype} sample {b}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('name', ['nine', 'nine_max1024', 'six', 'single'])
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_gather_form_equals_the_dense_form_on_the_gathered_rows(shape, name, dtype):
    bp = _bp()
    c = _case(shape, dtype, name)
    k, dk, dout = shape
    total, rows = c['qk'].shape[0], 500
    g = torch.Generator().manual_seed(rows + total)
    table = torch.randn(rows, k, dout, generator=g).to(dtype).to(DEV)
    index = torch.randint(0, rows, (total,), generator=g, dtype=torch.int32)
    index[::7] = -1                      # outside the table: the last row, by the contract of bp_sense_mix_gather
    index[3::11] = rows + 1000000
    idx_buf, idx = _guarded(index.to(DEV), fill=0x7fffffff)
    clamped = torch.where((idx < 0) | (idx >= rows), rows - 1, idx).long()
    want = bp.sense_mix_varlen(c['qk'], table[clamped], c['cu'], c['max_seqlen'], lse=c['lse'])
    out_buf, out = _guarded(torch.zeros(total, dout, dtype=dtype, device=DEV))
    bp.sense_mix_gather_varlen(c['qk'], table, idx, c['cu'], c['max_seqlen'], out=out, lse=c['lse'])
    assert _same_bits(out, want)
    assert torch.isnan(out_buf[:GUARD]).all() and torch.isnan(out_buf[-GUARD:]).all()
    own_lse = bp.sense_mix_gather_varlen(c['qk'], table, idx, c['cu'], c['max_seqlen'])
    assert _same_bits(own_lse, want)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('name', ['nine', 'six'])
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_a_sample_of_nans_leaves_every_other_sample_alone(shape, name, dtype):
    """Rows behind a sample's end belong to the next sample: a store or a clamped read that crosses the border shows as a
    changed bit or a NaN in a neighbour.  Also the neighbours of the zero-length sample."""
    bp = _bp()
    c = _case(shape, dtype, name)
    cu, lengths = c['cu'].tolist(), c['lengths']
    rows = 300
    table = torch.randn(rows, shape[0], shape[2], generator=torch.Generator().manual_seed(5)).to(dtype).to(DEV)
    index = torch.randint(0, rows - 1, (c['qk'].shape[0],), generator=torch.Generator().manual_seed(6), dtype=torch.int32).to(DEV)
    base_gather = bp.sense_mix_gather_varlen(c['qk'], table, index, c['cu'], c['max_seqlen'])
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        qk, content = c['qk'].clone(), c['content'].clone()
        qk[cu[b]:cu[b + 1]] = NAN
        content[cu[b]:cu[b + 1]] = NAN
        poisoned = table.clone()
        poisoned[rows - 1] = NAN                         # the row that only sample b names
        idx = index.clone()
        idx[cu[b]:cu[b + 1]] = rows - 1
        got = bp.sense_mix_varlen(qk, content, c['cu'], c['max_seqlen'])
        got_gather = bp.sense_mix_gather_varlen(qk, poisoned, idx, c['cu'], c['max_seqlen'])
        for o in range(len(lengths)):
            if o == b or lengths[o] == 0:
                continue
            sl = slice(cu[o], cu[o + 1])
            assert _same_bits(got[sl], c['out'][sl]), f'NaN sample {b} changed sample {o}'
            assert _same_bits(got_gather[sl], base_gather[sl]), f'NaN sample {b} changed sample {o} (gather)'
            assert torch.isfinite(got[sl].float()).all() and torch.isfinite(got_gather[sl].float()).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_a_captured_call_replays_with_another_split_of_the_rows(dtype):
    """cu_seqlens is read by the kernel alone: overwritten in place with another split of the same total (same max_seqlen),
    a replay equals the eager call with that split.  queue_ws == NULL on a capturing stream is refused."""
    bp = _bp()
    k, dk, dout = 16, 48, 288
    first, second, max_seqlen = [300, 20, 0, 257, 64], [1, 320, 63, 1, 256], 320
    total = sum(first)
    assert sum(second) == total
    g = torch.Generator().manual_seed(7)
    qk = (torch.randn(total, 2, k, dk, generator=g) * 1.2).to(dtype).to(DEV)
    content = torch.randn(total, k, dout, generator=g).to(dtype).to(DEV)
    want = [bp.sense_mix_varlen(qk, content, _cu(split), max_seqlen).clone() for split in (first, second)]
    assert not _same_bits(want[0], want[1])
    cu = _cu(first)
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        bp.sense_mix_varlen(qk, content, cu, max_seqlen)
    torch.cuda.current_stream().wait_stream(warm)
    torch.cuda.synchronize()
    lse = torch.empty(len(first), k, 320, dtype=torch.float32, device=DEV)
    out = torch.zeros(total, dout, dtype=dtype, device=DEV)

    def raw(queue):
        return bp.lib().bp_sense_mix_varlen(qk.data_ptr(), content.data_ptr(), out.data_ptr(), lse.data_ptr(), 0, cu.data_ptr(),
                                            len(first), max_seqlen, k, dk, dout, qk.stride(0), qk.stride(1), qk.stride(2),
                                            content.stride(0), content.stride(1), out.stride(0), dk ** -0.5,
                                            0 if dtype == torch.float16 else 1, queue,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        refused = raw(None)
        out_g = bp.sense_mix_varlen(qk, content, cu, max_seqlen)
    assert refused == -8                                  # BP_ERR_QUEUE_WS: nothing was captured for it
    for split, expect in ((first, want[0]), (second, want[1]), (first, want[0])):
        cu.copy_(_cu(split))
        out_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out_g, expect), split
    assert (out == 0).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('form', ['dense', 'gather'])
def test_packed_needle_problems_return_their_value_rows(form, dtype):
    """Per-sample needle problems of tests/prefill_needles.py, packed: every output row is the sum of its needles' value rows,
    bit for bit -- a key of another sample, or a key behind the needle's tile, would add to it."""
    bp = _bp()
    k, dk, dout = 16, 48, 256
    lengths = [257, 1, 64, 641, 0, 33, 320]
    probs = [P.sense_problem(n, k, dk, dout, b=1, device=DEV, form=form) for n in lengths if n > 0]
    qk = torch.cat([p['qk'][0] for p in probs]).to(dtype)
    want = torch.cat([p['want'][0] for p in probs])
    cu = _cu(lengths)
    lse = bp.sense_lse_varlen(qk, cu, max(lengths), probs[0]['scale'])
    for b, n in enumerate(lengths):
        torch.testing.assert_close(lse[b, :, :n], torch.full_like(lse[b, :, :n], probs[0]['lse']), **P.LSE_TOL)
    out_buf, out = _guarded(torch.zeros(sum(lengths), dout, dtype=dtype, device=DEV))
    if form == 'gather':
        table = probs[0]['table'].to(dtype)
        table[1::2] = -8.0                                # rows no sample names
        rows = torch.cat([p['rows'][0] for p in probs])
        bp.sense_mix_gather_varlen(qk, table, rows, cu, max(lengths), probs[0]['scale'], out=out, lse=lse)
    else:
        content = torch.cat([p['content'][0] for p in probs]).to(dtype)
        bp.sense_mix_varlen(qk, content, cu, max(lengths), probs[0]['scale'], out=out, lse=lse)
    assert torch.equal(want.to(dtype).double(), want.double()), 'expected result not representable'
    wrong = (out.float() != want).any(dim=-1)
    assert not wrong.any(), f'{int(wrong.sum())} rows differ from their needles\' value rows, first at {wrong.nonzero()[0].tolist()}'
    assert torch.isnan(out_buf[:GUARD]).all() and torch.isnan(out_buf[-GUARD:]).all()
