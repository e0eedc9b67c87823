"""GPU: the decode kernels (csrc/decode_core.h behind bp_flash_decode / bp_sense_decode) where the fixed-shape parity
tests of tests/test_gpu_decode.py cannot see:

A  needles: inputs whose fp32 answer is exact (tests/decode_needles.py), so WHICH keys a row saw is checked bit for
   bit at long lengths, on tile and split borders, in every G bucket of launch_decode, with everything the step must
   not read poisoned (NaN cache rows and table rows, out-of-range row indices);
-  the 2x-rule parity check of tests/test_gpu_decode.py at the head dims and sense widths it never launches ("buckets");
B  bit-exact properties at the model's decode shapes: rows behind L are not read, permuting the samples permutes the
   result, two calls (and a NaN workspace) give the same bits, only row L of the backing buffers changes;
C  200 consecutive steps from an empty cache, the kernels' own appends as input;
D  seeded drawn shapes (BP_FUZZ_SEEDS as tests/test_gpu_fuzz.py), strided views of packed projections included;
E  the contracts of include/bp_hip.h through the C ABI: length and row clamps, the workspace bound, lse_batch_stride,
   offsets beyond 2^31 elements / 2^32 bytes.

Mutation run (single-line mutants of csrc/decode_core.h, arithmetic or in-bounds indices only, each built as a variant
library and run once against tests/test_gpu_decode.py and this file; "old" = killed by test_gpu_decode.py as it stood
before this file, number = failing cases here of 251):

   #  mutant                                                            old   killed here by
   1  a split skips its first key when split > 0                        yes   128: needles, buckets, drawn, 200 steps
   2  a full tile drops key 63                                          yes   160: needles, properties, buckets, drawn, > 4 GiB
   3  key L is read from cache row L, not k_new (append still right)    yes   240: every layer (row L holds NaN / louder rows)
   4  the combine ignores the last active split                         yes   133: needles, buckets, drawn, 200 steps, clamps
   5  acc is not rescaled by alpha on a new running maximum             yes   120: needles, buckets, drawn, > 2^31
   6  sense 0's table slice for every sense when d_out == 8             no    11: needles (d_out = 8), buckets, drawn
   7  fp16 unpack of bf16 sense keys at G = 64, NQ = 1 (d_k 264...512)  no    9: buckets (6), drawn (3); NOT the needles
   8  senses: a split skips its first key when chunk >= 256             no*   14: needles (4), buckets (9), drawn (1)
   9  trunk, G <= 4 (d <= 32): a full tile drops key 63                 no    16: needles (8), buckets (8)
  10  a length >= max_seqlen is clamped to max_seqlen - 2               no    2: test_lengths_outside_the_cache_are_clamped
  11  a row index outside the table reads row 0, not the last row       no    2: test_sense_decode_clamps_rows_outside_the_table
  12  the LSE is stored with stride nheads, not lse_batch_stride        no    1: test_softmax_lse_with_a_wider_batch_stride
  13  row_index is read with stride max_seqlen, not idx_batch_stride    no    14: drawn senses
  14  the combine reads the workspace of inactive splits (times 0)      no    28 properties (NaN workspace) [+ 21 needles]
  15  the combine ignores a last active split of ONE key, chunk >= 32   no    32: needles only (L = 4032 at nsplit = 64)

tests/test_gpu_decode.py kills the plain wrong-key-set mutants (1-5) through its LSE tolerance and its short lengths
(chunk = 1 ... 5 keys, where a split border is every other key).  It passes the forms that need a long split or a
bucket it never launches (8, 9, 15; * 8 passes that file's bf16 sense test and fails the fp16 twin added with this file),
and every contract of section E (10-14).  Mutant 14's needle failures come from NaN that earlier poisoned buffers left
in the allocator's blocks: chance; the property cases hand it a NaN workspace on purpose.  Mutant 7 shows the needles'
blind spot: a monotone rescale of the scores keeps the needle on top, so values are the business of the 2x-rule layers
(buckets, drawn), visibility that of the needles.
"""
import os
import random

import pytest
import torch

import decode_needles as N
from decode_support import (FLASH_LENGTHS, _ar, _attend, _bp, _flash_decode_matches_fp32, _same_bits,
                            _sense_decode_matches_fp32, _sense_ref, _within_2x)
from decode_support import _close_drawn as _close

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ['bf16', 'fp16']
SEEDS = range(int(os.environ.get('BP_FUZZ_SEEDS', '24')))
NAN = float('nan')
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -(2 ** 31)


def _flash_nsplit(bp, b, h, d, max_s):
    return bp.lib().bp_flash_decode_ws_floats(b, h, d, max_s) // (b * h * (d + 2))


def _sense_nsplit(bp, b, k, dout, max_s):
    return bp.lib().bp_sense_decode_ws_floats(b, k, dout, max_s) // (b * k * (dout + 2))


def _flash_abi(bp, q, k_new, v_new, cache, seqlens, scale, out, lse=None, ws=None):
    """bp_flash_decode through the binding's C signature: caller-owned out / lse / ws, any strides."""
    b, h, d = q.shape
    max_s = cache.shape[1]
    if ws is None:
        ws = torch.empty(max(bp.lib().bp_flash_decode_ws_floats(b, h, d, max_s), 4), dtype=torch.float32, device=DEV)
    bp._call('bp_flash_decode', q.device, q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(), cache.data_ptr(),
             seqlens.data_ptr(), out.data_ptr(), lse.data_ptr() if lse is not None else None, ws.data_ptr(), ws.numel(),
             b, h, d, max_s, q.stride(0), q.stride(1), k_new.stride(0), k_new.stride(1), v_new.stride(0), v_new.stride(1),
             cache.stride(0), cache.stride(1), cache.stride(2), cache.stride(3), out.stride(0), out.stride(1),
             lse.stride(0) if lse is not None else h, float(scale), bp._dtype_code(q))
    return out


def _sense_abi(bp, q, k_new, k_cache, table, rows, new_row, seqlens, scale, out, ws=None):
    b, k, dk = q.shape
    max_s, dout = k_cache.shape[1], table.shape[2]
    if ws is None:
        ws = torch.empty(max(bp.lib().bp_sense_decode_ws_floats(b, k, dout, max_s), 4), dtype=torch.float32, device=DEV)
    bp._call('bp_sense_decode', q.device, q.data_ptr(), k_new.data_ptr(), k_cache.data_ptr(), table.data_ptr(),
             rows.data_ptr(), new_row.data_ptr(), seqlens.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
             b, k, dk, dout, max_s, table.shape[0], q.stride(0), q.stride(1), k_new.stride(0), k_new.stride(1),
             k_cache.stride(0), k_cache.stride(1), k_cache.stride(2), table.stride(0), table.stride(1), rows.stride(0),
             out.stride(0), float(scale), bp._dtype_code(q))
    return out


# ---- A. needles ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case', N.TRUNK_CASES, ids=[f"d{c['d']}_{c['regime']}" for c in N.TRUNK_CASES])
def test_flash_decode_sees_exactly_keys_0_to_L(case, dtype):
    """out[b, h] == V[j*] bit for bit for a needle j* per (sample, head), at every length of decode_needles.lengths and
    every position of decode_needles.needle_positions; cache rows >= L hold NaN before the call (row L must come from
    k_new / v_new); afterwards only row L of the backing buffer differs, guard samples included."""
    bp = _bp()
    d, b, h, max_s = case['d'], case['batch'], case['heads'], case['max_seqlen']
    nsplit = _flash_nsplit(bp, b, h, d, max_s)
    assert nsplit == {'split64': 64, 'split8': 8, 'split1': 1}[case['regime']]
    pos, bi, hi = _ar(max_s), _ar(b)[:, None], _ar(h)[None, :]
    keys = N.code(pos, d)                                                          # (max_s, d)
    vals = N.values(N.trunk_value_ids(case, bi[:, :, None], hi[:, None, :], pos[None, :, None]), d)   # (b, max_s, h, d)
    clean = torch.empty(b, max_s, 2, h, d, device=DEV, dtype=dtype)
    clean[:, :, 0] = keys[None, :, None, :].to(dtype)
    clean[:, :, 1] = vals.to(dtype)
    full = torch.full((b + 2, max_s, 2, h, d), NAN, device=DEV, dtype=dtype)        # guard samples on both sides
    cache = full[1:b + 1]
    scale = N.scale(d)
    for L in N.lengths(nsplit, d, max_s):
        cache.copy_(clean)
        cache[:, L:] = NAN
        k_new = keys[L].to(dtype).expand(b, h, d).contiguous()
        v_new = vals[:, L].to(dtype).contiguous()
        want_full = full.clone()
        want_full[1:b + 1, L, 0], want_full[1:b + 1, L, 1] = k_new, v_new
        seqlens = torch.full((b,), L, dtype=torch.int32, device=DEV)
        for call in N.assign(N.needle_positions(L, nsplit), b * h):
            jstar = torch.tensor(call, device=DEV).view(b, h)
            q = N.code(jstar, d).to(dtype)
            cache[:, L] = NAN
            out, lse = bp.flash_decode(q, k_new, v_new, cache, seqlens, scale, return_lse=True)
            want = vals[bi, jstar, hi]                                              # (b, h, d)
            bad = (out.float() != want).any(dim=-1)
            assert not bad.any(), (f'd={d} {dtype} nsplit={nsplit} L={L}: wrong rows for needles '
                                   f'{sorted(set(jstar[bad].tolist()))}')
            torch.testing.assert_close(lse, torch.full_like(lse, N.needle_score(d)), rtol=1e-5, atol=1e-4)
            assert _same_bits(full, want_full), f'd={d} L={L}: only row L of each sample may change'


SENSE_IDS = [f"dk{c['dk']}of{c['dkp']}_k{c['k']}_dout{c['dout']}" for c in N.SENSE_CASES]


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('form', ['table', 'cache'])
@pytest.mark.parametrize('case', N.SENSE_CASES, ids=SENSE_IDS)
def test_sense_decode_sees_exactly_keys_0_to_L(case, form, dtype):
    """out[b] == sum_l table[row(b, j*_{b,l}), l] bit for bit, a different needle per (sample, sense).  Before the call
    key-cache rows >= L hold NaN, row_index[b, j >= L] holds indices outside the table, and every table row that no
    visible index names holds NaN."""
    bp = _bp()
    dkp, dk, k, dout, b, max_s = (case[x] for x in ('dkp', 'dk', 'k', 'dout', 'batch', 'max_seqlen'))
    nsplit = _sense_nsplit(bp, b, k, dout, max_s)
    pos, bi, li = _ar(max_s), _ar(b)[:, None], _ar(k)[None, :]
    keys = N.code(pos, dk, dkp).to(dtype)                                           # (max_s, dkp)
    table_rows = N.VOCAB if form == 'table' else b * max_s
    table_clean = N.sense_value(_ar(table_rows)[:, None], li, dout).to(dtype)       # (rows, k, dout)
    rows_clean = N.sense_row(case, form, bi, pos[None, :])                          # (b, max_s)
    poison = torch.tensor([-1, table_rows, INT32_MAX, INT32_MIN, table_rows + 7, -table_rows], dtype=torch.int32,
                          device=DEV)[(pos[None, :] + bi) % 6]                      # (b, max_s)
    k_cache = torch.empty(b, max_s, k, dkp, device=DEV, dtype=dtype)
    scale = N.scale(dk)
    for L in N.lengths(nsplit, dk, max_s):
        k_cache.copy_(keys[None, :, None, :].expand_as(k_cache))
        k_cache[:, L:] = NAN
        k_new = keys[L].expand(b, k, dkp).contiguous()
        new_row = rows_clean[:, L].contiguous()
        want_kc = k_cache.clone()
        want_kc[:, L] = k_new
        rows = torch.where(pos[None, :] >= L, poison, rows_clean).contiguous()
        want_rows = rows.clone()
        want_rows[:, L] = new_row
        named = torch.zeros(table_rows, dtype=torch.bool, device=DEV)
        named[rows_clean[:, :L + 1].long().flatten()] = True
        table = table_clean.clone()
        table[~named] = NAN
        seqlens = torch.full((b,), L, dtype=torch.int32, device=DEV)
        for call in N.assign(N.needle_positions(L, nsplit), b * k):
            jstar = torch.tensor(call, device=DEV).view(b, k)
            q = N.code(jstar, dk, dkp).to(dtype)
            k_cache[:, L] = NAN
            rows[:, L] = poison[:, L]
            out = bp.sense_decode(q, k_new, k_cache, table, rows, new_row, seqlens, scale)
            r = N.sense_row(case, form, bi, jstar).long()                           # (b, k)
            want = table_clean[r, li].float().sum(dim=1).to(dtype)                  # exact in fp32, rounded once
            bad = (out != want).any(dim=-1)
            assert not bad.any(), (f'{case} {form} {dtype} nsplit={nsplit} L={L}: wrong samples {bad.nonzero().flatten().tolist()}'
                                   f' of needles {jstar[bad].tolist()}')
            assert _same_bits(k_cache, want_kc) and torch.equal(rows, want_rows), f'{case} L={L}: appends'


# ---- every instantiation launch_decode can pick, on random inputs -------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('d', [8, 16, 24, 32, 40, 56, 96, 120])
def test_flash_decode_matches_fp32_at_every_head_dim_bucket(d, dtype):
    """The check of tests/test_gpu_decode.py (2x rule, LSE, appends, repeatability) at the head dims it does not run:
    d / 8 = 1, 2, 3-4 (G = 1, 2, 4: never launched there) and other members of the G = 8 and 16 buckets."""
    _flash_decode_matches_fp32(d, dtype, FLASH_LENGTHS[0])


# (padded d_k, true d_k, senses, d_out): G = 1, 16, 64 (NQ = 1) are never launched by tests/test_gpu_decode.py
BUCKET_SHAPES = [(8, 8, 4, 8), (32, 32, 20, 104), (72, 72, 8, 16), (128, 128, 2, 2048), (264, 264, 2, 384), (400, 400, 1, 1000),
                 (512, 512, 1, 640), (520, 513, 1, 768)]


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('form', ['table', 'cache'])
@pytest.mark.parametrize('shape', BUCKET_SHAPES, ids=[f'dk{s[1]}_k{s[2]}_dout{s[3]}' for s in BUCKET_SHAPES])
def test_sense_decode_matches_fp32_at_every_width_bucket(shape, form, dtype):
    _sense_decode_matches_fp32(shape, form, dtype)


# ---- B. properties at the model's decode shapes -------------------------------------------------------------------------

MAX_S = 4104
STAGGER = [4096, 0, 1, 63, 64, 65, 1000, 2047]


def _staggered(b):
    return [STAGGER[i] if i < len(STAGGER) else (i * 613) % 4097 for i in range(b)]


TRUNK_SHAPES = {'small': (12, 64), 'mini': (8, 80), 'micro': (6, 64)}


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('batch', [1, 8, 64])
@pytest.mark.parametrize('name', list(TRUNK_SHAPES))
def test_flash_decode_properties(name, batch, dtype):
    bp = _bp()
    h, d = TRUNK_SHAPES[name]
    g = torch.Generator(device=DEV).manual_seed(batch * 131 + d)
    full = torch.randn(batch + 3, MAX_S, 2, h, d, device=DEV, generator=g).to(dtype)
    off = 2
    cache = full[off:off + batch]                 # a cache at a non-zero batch_size_offset
    q, k_new, v_new = (torch.randn(batch, h, d, device=DEV, generator=g).to(dtype) * s for s in (2.0, 1.0, 1.0))
    lengths = _staggered(batch)
    seqlens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    Ls, bi = seqlens.long(), _ar(batch)
    before = full.clone()
    scale = d ** -0.5
    out, lse = bp.flash_decode(q, k_new, v_new, cache, seqlens, scale, return_lse=True)
    # only row L of each sample changed, in the whole backing buffer
    want_full = before.clone()
    want_full[off + bi, Ls, 0], want_full[off + bi, Ls, 1] = k_new, v_new
    assert torch.equal(full, want_full)
    # the same bits again, from the wrapper and with a workspace that held NaN on entry
    out2, lse2 = bp.flash_decode(q, k_new, v_new, cache, seqlens, scale, return_lse=True)
    assert torch.equal(out2, out) and torch.equal(lse2, lse)
    ws = torch.full((bp.lib().bp_flash_decode_ws_floats(batch, h, d, MAX_S),), NAN, device=DEV)
    out3, lse3 = torch.empty_like(out), torch.empty_like(lse)
    _flash_abi(bp, q, k_new, v_new, cache, seqlens, scale, out3, lse3, ws)
    assert torch.equal(out3, out) and torch.equal(lse3, lse)
    # louder rows behind L (row L included: it is overwritten, never read)
    behind = (_ar(MAX_S)[None, :] >= Ls[:, None])[:, :, None, None, None]
    full.copy_(before)
    cache.copy_(torch.where(behind, cache * 6, cache))
    out4, lse4 = bp.flash_decode(q, k_new, v_new, cache, seqlens, scale, return_lse=True)
    assert torch.equal(out4, out) and torch.equal(lse4, lse)
    assert torch.equal(cache[bi, Ls], want_full[off + bi, Ls])
    # permuting the samples permutes the result
    perm = torch.randperm(batch, device=DEV, generator=g)
    pcache = before[off:off + batch][perm].contiguous()
    out5, lse5 = bp.flash_decode(q[perm], k_new[perm], v_new[perm], pcache, seqlens[perm].contiguous(), scale,
                                 return_lse=True)
    assert torch.equal(out5, out[perm]) and torch.equal(lse5, lse[perm])
    assert torch.equal(pcache, want_full[off:off + batch][perm])


# (padded d_k, senses, d_out): Small, Mini k = 64 / 4 / 1, Micro
SENSE_MODEL_SHAPES = {'small': (48, 16, 768), 'mini_k64': (16, 64, 640), 'mini_k4': (160, 4, 640),
                      'mini_k1': (640, 1, 640), 'micro': (24, 16, 384)}
# (the cache form stops at batch 8: its per-position content table at batch 64 is 6.5 GB for Small, 13 GB while drawn in
# fp32; the table form runs batch 64, so nsplit = 1 is covered)
SENSE_PROPERTY_CASES = [(n, b, 'table') for n in SENSE_MODEL_SHAPES for b in (1, 8, 64)] \
    + [(n, b, 'cache') for n in SENSE_MODEL_SHAPES for b in (1, 8)]


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('name,batch,form', SENSE_PROPERTY_CASES)
def test_sense_decode_properties(name, batch, form, dtype):
    bp = _bp()
    dk, k, dout = SENSE_MODEL_SHAPES[name]
    g = torch.Generator(device=DEV).manual_seed(batch * 17 + dk)
    off, vocab = 1, 997
    kc_full = torch.randn(batch + 2, MAX_S, k, dk, device=DEV, generator=g).to(dtype)
    k_cache = kc_full[off:off + batch]
    q, k_new = (torch.randn(batch, k, dk, device=DEV, generator=g).to(dtype) * s for s in (2.0, 1.0))
    lengths = _staggered(batch)
    seqlens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    Ls, bi, pos = seqlens.long(), _ar(batch), _ar(MAX_S)
    rows_full = torch.randint(0, vocab, (batch + 2, MAX_S), device=DEV, generator=g, dtype=torch.int32)
    rows = rows_full[off:off + batch]
    if form == 'table':
        table = torch.randn(vocab, k, dout, device=DEV, generator=g).to(dtype)
        new_row = torch.randint(0, vocab, (batch,), device=DEV, generator=g, dtype=torch.int32)
    else:
        table = torch.randn(batch * MAX_S, k, dout, device=DEV, generator=g).to(dtype)
        rows.copy_((bi[:, None] * MAX_S + pos[None, :]).int())
        new_row = (bi * MAX_S + Ls).int()
    kc_before, rows_before = kc_full.clone(), rows_full.clone()
    scale = dk ** -0.5
    out = bp.sense_decode(q, k_new, k_cache, table, rows, new_row, seqlens, scale)
    want_kc, want_rows = kc_before.clone(), rows_before.clone()
    want_kc[off + bi, Ls], want_rows[off + bi, Ls] = k_new, new_row
    assert torch.equal(kc_full, want_kc) and torch.equal(rows_full, want_rows)
    assert torch.equal(bp.sense_decode(q, k_new, k_cache, table, rows, new_row, seqlens, scale), out)
    ws = torch.full((bp.lib().bp_sense_decode_ws_floats(batch, k, dout, MAX_S),), NAN, device=DEV)
    assert torch.equal(_sense_abi(bp, q, k_new, k_cache, table, rows, new_row, seqlens, scale, torch.empty_like(out), ws),
                       out)
    # behind L: louder keys, other (valid) row indices and, in the cache form, louder content rows
    behind = pos[None, :] >= Ls[:, None]
    kc_full.copy_(kc_before)
    rows_full.copy_(rows_before)
    k_cache.copy_(torch.where(behind[:, :, None, None], k_cache * 6, k_cache))
    rows.copy_(torch.where(behind, (rows + 1) % table.shape[0], rows))
    table4 = table
    if form == 'cache':
        table4 = torch.where((pos[None, :] > Ls[:, None]).flatten()[:, None, None], table * 6, table)
    assert torch.equal(bp.sense_decode(q, k_new, k_cache, table4, rows, new_row, seqlens, scale), out)
    assert torch.equal(k_cache[bi, Ls], k_new) and torch.equal(rows[bi, Ls], new_row)
    del table4
    # permutation (the cache form keeps its table: row_index and new_row carry the sample's rows along)
    perm = torch.randperm(batch, device=DEV, generator=g)
    pkc = kc_before[off:off + batch][perm].contiguous()
    prows = rows_before[off:off + batch][perm].contiguous()
    out5 = bp.sense_decode(q[perm], k_new[perm], pkc, table, prows, new_row[perm].contiguous(), seqlens[perm].contiguous(),
                           scale)
    assert torch.equal(out5, out[perm])
    assert torch.equal(pkc, want_kc[off:off + batch][perm]) and torch.equal(prows, want_rows[off:off + batch][perm])


# ---- C. multi-step ------------------------------------------------------------------------------------------------------

STEPS, STARTS = 200, [0, 1, 60, 63]


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_flash_decode_200_steps_from_its_own_appends(dtype):
    bp = _bp()
    b, h, d, max_s = len(STARTS), 4, 64, 272
    g = torch.Generator(device=DEV).manual_seed(7)
    cache = torch.full((b, max_s, 2, h, d), NAN, device=DEV, dtype=dtype)
    for i, s in enumerate(STARTS):
        cache[i, :s] = torch.randn(s, 2, h, d, device=DEV, generator=g).to(dtype)
    want_cache = cache.clone()
    qs, ks, vs = (torch.randn(STEPS, b, h, d, device=DEV, generator=g).to(dtype) * s for s in (2.0, 1.0, 1.0))
    seqlens = torch.tensor(STARTS, dtype=torch.int32, device=DEV)
    scale = d ** -0.5
    for t in range(STEPS):
        out = bp.flash_decode(qs[t], ks[t], vs[t], cache, seqlens, scale)
        for i, s in enumerate(STARTS):
            want_cache[i, s + t, 0], want_cache[i, s + t, 1] = ks[t, i], vs[t, i]
            keys, values = want_cache[i, :s + t + 1, 0], want_cache[i, :s + t + 1, 1]
            _within_2x(out[i], _attend(qs[t, i], keys, values, scale, torch.float32),
                       _attend(qs[t, i], keys, values, scale, dtype), f'step {t} sample {i}')
        seqlens += 1
    assert _same_bits(cache, want_cache)
    for i, s in enumerate(STARTS):
        assert torch.equal(cache[i, s:s + STEPS, 0], ks[:, i]) and torch.equal(cache[i, s:s + STEPS, 1], vs[:, i])


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_sense_decode_200_steps_from_its_own_appends(dtype):
    bp = _bp()
    b, k, dk, dout, max_s, vocab = len(STARTS), 16, 48, 768, 272, 997
    g = torch.Generator(device=DEV).manual_seed(8)
    k_cache = torch.full((b, max_s, k, dk), NAN, device=DEV, dtype=dtype)
    rows = torch.full((b, max_s), INT32_MAX, device=DEV, dtype=torch.int32)
    for i, s in enumerate(STARTS):
        k_cache[i, :s] = torch.randn(s, k, dk, device=DEV, generator=g).to(dtype)
        rows[i, :s] = torch.randint(0, vocab, (s,), device=DEV, generator=g, dtype=torch.int32)
    want_kc, want_rows = k_cache.clone(), rows.clone()
    table = torch.randn(vocab, k, dout, device=DEV, generator=g).to(dtype)
    qs, ks = (torch.randn(STEPS, b, k, dk, device=DEV, generator=g).to(dtype) * s for s in (2.0, 1.0))
    new_rows = torch.randint(0, vocab, (STEPS, b), device=DEV, generator=g, dtype=torch.int32)
    seqlens = torch.tensor(STARTS, dtype=torch.int32, device=DEV)
    scale = dk ** -0.5
    for t in range(STEPS):
        out = bp.sense_decode(qs[t], ks[t], k_cache, table, rows, new_rows[t], seqlens, scale)
        for i, s in enumerate(STARTS):
            want_kc[i, s + t], want_rows[i, s + t] = ks[t, i], new_rows[t, i]
            keys, content = want_kc[i, :s + t + 1], table[want_rows[i, :s + t + 1].long()]
            _within_2x(out[i], _sense_ref(qs[t, i], keys, content, scale, torch.float32),
                       _sense_ref(qs[t, i], keys, content, scale, dtype), f'step {t} sample {i}')
        seqlens += 1
    assert _same_bits(k_cache, want_kc) and torch.equal(rows, want_rows)
    for i, s in enumerate(STARTS):
        assert torch.equal(k_cache[i, s:s + STEPS], ks[:, i]) and torch.equal(rows[i, s:s + STEPS], new_rows[:, i])


# ---- D. drawn shapes ----------------------------------------------------------------------------------------------------

MAX_SEQLENS = [1, 2, 63, 64, 65, 200, 1000, 4104]


def _drawn_lengths(rnd, b, max_s, nsplit):
    """Per-sample lengths: 0, 1, max - 1, 64-key tile borders, split borders ((L + 1) a multiple of nsplit, +- 1), uniform."""
    out = []
    for _ in range(b):
        m = nsplit * rnd.randint(1, max(max_s // nsplit, 1))
        cands = [0, 1, max_s - 1, max_s - 2, 63, 64, 65, 127, 128, 129, m - 2, m - 1, m, rnd.randint(0, max_s - 1),
                 rnd.randint(0, max_s - 1)]
        out.append(rnd.choice([c for c in cands if 0 <= c <= max_s - 1]))
    return out


@pytest.mark.parametrize('seed', SEEDS)
def test_flash_decode_on_drawn_shapes(seed):
    bp = _bp()
    rnd = random.Random(5000 + seed)
    g = torch.Generator(device=DEV).manual_seed(seed)
    dtype = rnd.choice(DTYPES)
    b, h, d = rnd.randint(1, 9), rnd.randint(1, 12), 8 * rnd.randint(1, 16)
    max_s = rnd.choice(MAX_SEQLENS)
    nsplit = _flash_nsplit(bp, b, h, d, max_s)
    lengths = _drawn_lengths(rnd, b, max_s, nsplit)
    scale = d ** -0.5 / rnd.choice([1, 1, 2, 7, 12])
    packed = rnd.random() < 0.5
    off, extra = rnd.randint(0, 3), rnd.randint(0, 2)
    name = f'seed {seed}: {dtype} b={b} h={h} d={d} max_s={max_s} nsplit={nsplit} L={lengths} packed={packed} off={off}'
    if packed:     # views of one packed projection, as qkv[:, 0].unbind(dim=1) in flash_attn/modules/mha.py
        qkv = torch.randn(b, 3, h, d, device=DEV, generator=g).to(dtype)
        q, k_new, v_new = qkv.unbind(dim=1)
    else:
        q, k_new, v_new = (torch.randn(b, h, d, device=DEV, generator=g).to(dtype) for _ in range(3))
    full = torch.randn(off + b + extra, max_s, 2, h, d, device=DEV, generator=g).to(dtype)
    cache = full[off:off + b]
    before = full.clone()
    out_full = torch.full((b, h, d + 8), NAN, device=DEV, dtype=dtype)
    out = out_full[:, :, :d]                                         # a strided out=
    seqlens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    got, lse = bp.flash_decode(q, k_new, v_new, cache, seqlens, scale, out=out, return_lse=True)
    assert got.data_ptr() == out.data_ptr() and torch.isnan(out_full[:, :, d:]).all(), name
    want = before.clone()
    for i, L in enumerate(lengths):
        want[off + i, L, 0], want[off + i, L, 1] = k_new[i], v_new[i]
    assert torch.equal(full, want), name + ': the append, and nothing else'
    for i, L in enumerate(lengths):
        keys, values = want[off + i, :L + 1, 0], want[off + i, :L + 1, 1]
        _close(out[i], _attend(q[i], keys, values, scale, torch.float32), _attend(q[i], keys, values, scale, dtype),
               name + f' out[{i}]')
        ref_lse = torch.logsumexp(torch.einsum('hd,shd->hs', q[i].float(), keys.float()) * scale, dim=-1)
        torch.testing.assert_close(lse[i], ref_lse, rtol=1e-5, atol=1e-4, msg=name + f' lse[{i}]')


@pytest.mark.parametrize('seed', SEEDS)
def test_sense_decode_on_drawn_shapes(seed):
    bp = _bp()
    rnd = random.Random(6000 + seed)
    g = torch.Generator(device=DEV).manual_seed(seed)
    dtype = rnd.choice(DTYPES)
    form = rnd.choice(['table', 'cache'])
    b, k = rnd.randint(1, 4), rnd.choice([1, 2, 4, 16, 20, 64])
    dkp = rnd.choice([8 * rnd.randint(1, 16), 8 * rnd.randint(1, 16), 160, 264, 400, 512, 640])
    dk = dkp - rnd.choice([0, 0, rnd.randint(1, 7)])                 # zero columns, as ContextSelfAttn.project pads
    dout = rnd.choice([8, 16, 104, 384, 640, 768, 1000, 2048])
    # (the fp32 oracle materialises (L + 1, k, d_out) content rows per sample: keep that under 2^27 elements)
    max_s = rnd.choice([m for m in MAX_SEQLENS if m * k * dout <= 2 ** 27])
    nsplit = _sense_nsplit(bp, b, k, dout, max_s)
    lengths = _drawn_lengths(rnd, b, max_s, nsplit)
    scale = dk ** -0.5 * rnd.choice([1, 1, 2, 0.5])
    packed = rnd.random() < 0.5
    name = (f'seed {seed}: {dtype} {form} b={b} k={k} dk={dk}/{dkp} dout={dout} max_s={max_s} nsplit={nsplit} L={lengths} '
            f'packed={packed}')
    pad = (_ar(dkp) < dk).float()

    def senses(*lead):
        return (torch.randn(*lead, k, dkp, device=DEV, generator=g) * pad).to(dtype)
    if packed:     # views of the packed projection, as qk[:, 0, 0] / qk[:, 0, 1] in src/models/backpack.py
        qk = senses(b, 2)
        q, k_new = qk[:, 0], qk[:, 1]
    else:
        q, k_new = senses(b), senses(b)
    k_cache = senses(b, max_s)
    rows_full = torch.full((b, max_s + rnd.randint(1, 9)), INT32_MIN, device=DEV, dtype=torch.int32)
    rows = rows_full[:, :max_s]                                      # batch stride > max_seqlen
    if form == 'table':
        vocab = rnd.choice([1, 50, 997])
        table = torch.randn(vocab, k, dout, device=DEV, generator=g).to(dtype)
        rows.copy_(torch.randint(0, vocab, (b, max_s), device=DEV, generator=g, dtype=torch.int32))
        new_row = torch.randint(0, vocab, (b,), device=DEV, generator=g, dtype=torch.int32)
    else:
        table = torch.randn(b * max_s, k, dout, device=DEV, generator=g).to(dtype)
        rows.copy_((_ar(b)[:, None] * max_s + _ar(max_s)[None, :]).int())
        new_row = (_ar(b) * max_s + torch.tensor(lengths, device=DEV)).int()
    seqlens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    want_kc, want_rows = k_cache.clone(), rows_full.clone()
    out = bp.sense_decode(q, k_new, k_cache, table, rows, new_row, seqlens, scale)
    for i, L in enumerate(lengths):
        want_kc[i, L], want_rows[i, L] = k_new[i], new_row[i]
    assert torch.equal(k_cache, want_kc) and torch.equal(rows_full, want_rows), name + ': the appends, and nothing else'
    for i, L in enumerate(lengths):
        keys, content = want_kc[i, :L + 1], table[want_rows[i, :L + 1].long()]
        _close(out[i], _sense_ref(q[i], keys, content, scale, torch.float32),
               _sense_ref(q[i], keys, content, scale, dtype), name + f' out[{i}]')


# ---- E. the contracts of include/bp_hip.h -------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_lengths_outside_the_cache_are_clamped(dtype):
    """cache_seqlens = (-5, max, max + 100, INT32_MAX) behave exactly as (0, max - 1, max - 1, max - 1); the guard samples
    before and behind the cache view stay untouched."""
    bp = _bp()
    g = torch.Generator(device=DEV).manual_seed(11)
    b, max_s = 4, 200
    wild = torch.tensor([-5, max_s, max_s + 100, INT32_MAX], dtype=torch.int32, device=DEV)
    tame = torch.tensor([0, max_s - 1, max_s - 1, max_s - 1], dtype=torch.int32, device=DEV)
    h, d = 3, 64
    q, k_new, v_new = (torch.randn(b, h, d, device=DEV, generator=g).to(dtype) for _ in range(3))
    base = torch.randn(b + 2, max_s, 2, h, d, device=DEV, generator=g).to(dtype)
    res = []
    for seqlens in (wild, tame):
        full = base.clone()
        out, lse = bp.flash_decode(q, k_new, v_new, full[1:b + 1], seqlens, d ** -0.5, return_lse=True)
        assert torch.equal(full[0], base[0]) and torch.equal(full[-1], base[-1])
        res.append((out, lse, full))
    assert all(torch.equal(x, y) for x, y in zip(*res))
    assert torch.equal(res[0][2][1, 0, 0], k_new[0]) and torch.equal(res[0][2][2:5, max_s - 1, 1], v_new[1:])
    assert torch.isfinite(res[0][0]).all()

    k, dk, dout, vocab = 4, 48, 104, 50
    q, k_new = (torch.randn(b, k, dk, device=DEV, generator=g).to(dtype) for _ in range(2))
    kc_base = torch.randn(b + 2, max_s, k, dk, device=DEV, generator=g).to(dtype)
    rows_base = torch.randint(0, vocab, (b + 2, max_s), device=DEV, generator=g, dtype=torch.int32)
    table = torch.randn(vocab, k, dout, device=DEV, generator=g).to(dtype)
    new_row = torch.randint(0, vocab, (b,), device=DEV, generator=g, dtype=torch.int32)
    res = []
    for seqlens in (wild, tame):
        kc, rows = kc_base.clone(), rows_base.clone()
        out = bp.sense_decode(q, k_new, kc[1:b + 1], table, rows[1:b + 1], new_row, seqlens, dk ** -0.5)
        for buf, ref in ((kc, kc_base), (rows, rows_base)):
            assert torch.equal(buf[0], ref[0]) and torch.equal(buf[-1], ref[-1])
        res.append((out, kc, rows))
    assert all(torch.equal(x, y) for x, y in zip(*res))
    assert torch.equal(res[0][1][1, 0], k_new[0]) and torch.equal(res[0][2][2:5, max_s - 1], new_row[1:])
    assert torch.isfinite(res[0][0]).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_sense_decode_clamps_rows_outside_the_table(dtype):
    """row_index and new_row outside the table (the values of test_sense_mix_gather_clamps_indices_outside_the_table) read
    the table's last row.  The STORED row_index[b, L] is new_row as given, unclamped: that is what the kernel does, and a
    later step clamps it again on reading; asserted so that changing it is a decision."""
    bp = _bp()
    g = torch.Generator(device=DEV).manual_seed(5)
    b, max_s, k, dk, dout, vocab = 4, 200, 4, 16, 256, 50
    lengths = [150, 199, 80, 0]
    q, k_new = (torch.randn(b, k, dk, device=DEV, generator=g).to(dtype) for _ in range(2))
    kc_base = torch.randn(b, max_s, k, dk, device=DEV, generator=g).to(dtype)
    table = torch.randn(vocab, k, dout, device=DEV, generator=g).to(dtype)
    index = torch.randint(0, vocab, (b, max_s), device=DEV, generator=g, dtype=torch.int32)
    bad = index.clone()
    bad[0, 3], bad[0, 77], bad[1, 198], bad[1, 0], bad[2, 64] = -1, 50, INT32_MAX, INT32_MIN, 51
    good = bad.clone()
    good[0, 3], good[0, 77], good[1, 198], good[1, 0], good[2, 64] = 49, 49, 49, 49, 49
    bad_new = torch.tensor([7, -1, 50, INT32_MAX], dtype=torch.int32, device=DEV)
    good_new = torch.tensor([7, 49, 49, 49], dtype=torch.int32, device=DEV)
    seqlens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    bad_rows, good_rows = bad.clone(), good.clone()
    out_bad = bp.sense_decode(q, k_new, kc_base.clone(), table, bad_rows, bad_new, seqlens, dk ** -0.5)
    out_good = bp.sense_decode(q, k_new, kc_base.clone(), table, good_rows, good_new, seqlens, dk ** -0.5)
    assert torch.equal(out_bad, out_good)
    # not vacuous: the last row carries weight in every sample
    other = table.clone()
    other[49] = -other[49]
    assert not (bp.sense_decode(q, k_new, kc_base.clone(), other, good.clone(), good_new, seqlens, dk ** -0.5)
                == out_good).all(dim=1).any()
    for i, L in enumerate(lengths):
        bad[i, L], good[i, L] = bad_new[i], good_new[i]
    assert torch.equal(bad_rows, bad) and torch.equal(good_rows, good)


WS_TRUNK = [(1, 1, 8, 64, [63]), (1, 1, 128, 4104, [4096]), (9, 12, 128, 4104, None), (2, 3, 80, 65, [64, 0])]
WS_SENSE = [(1, 1, 8, 8, 64, [63]), (1, 1, 8, 2048, 4104, [4096]), (1, 64, 16, 2048, 4104, [4000]),
            (2, 64, 16, 8, 200, [199, 0]), (3, 2, 640, 104, 4104, [4096, 4095, 1])]
SENTINEL = -7.25


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_the_workspace_query_is_enough(dtype):
    """`ws` is exactly *_ws_floats() elements inside a sentinel-filled buffer: the sentinels on both sides survive (the
    wrappers allocate exactly that size, so an overrun would land in a neighbour unnoticed), and the result equals the
    wrapper's.  nsplit = 1 and 64, d_out = 8 and 2048, 64 senses."""
    bp = _bp()
    g = torch.Generator(device=DEV).manual_seed(13)
    pad = 4096
    for b, h, d, max_s, lengths in WS_TRUNK:
        lengths = lengths or [(i * 509) % 4097 for i in range(b)]
        n = bp.lib().bp_flash_decode_ws_floats(b, h, d, max_s)
        assert n == b * h * _flash_nsplit(bp, b, h, d, max_s) * (d + 2)
        buf = torch.full((pad + n + pad,), SENTINEL, device=DEV)
        q, k_new, v_new = (torch.randn(b, h, d, device=DEV, generator=g).to(dtype) for _ in range(3))
        cache = torch.randn(b, max_s, 2, h, d, device=DEV, generator=g).to(dtype)
        seqlens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
        want = bp.flash_decode(q, k_new, v_new, cache.clone(), seqlens, d ** -0.5)
        got = _flash_abi(bp, q, k_new, v_new, cache, seqlens, d ** -0.5, torch.empty_like(want), None, buf[pad:pad + n])
        assert torch.equal(got, want)
        assert (buf[:pad] == SENTINEL).all() and (buf[pad + n:] == SENTINEL).all(), (b, h, d, max_s)
    for b, k, dk, dout, max_s, lengths in WS_SENSE:
        n = bp.lib().bp_sense_decode_ws_floats(b, k, dout, max_s)
        assert n == b * k * _sense_nsplit(bp, b, k, dout, max_s) * (dout + 2)
        buf = torch.full((pad + n + pad,), SENTINEL, device=DEV)
        q, k_new = (torch.randn(b, k, dk, device=DEV, generator=g).to(dtype) for _ in range(2))
        k_cache = torch.randn(b, max_s, k, dk, device=DEV, generator=g).to(dtype)
        table = torch.randn(997, k, dout, device=DEV, generator=g).to(dtype)
        rows = torch.randint(0, 997, (b, max_s), device=DEV, generator=g, dtype=torch.int32)
        new_row = torch.randint(0, 997, (b,), device=DEV, generator=g, dtype=torch.int32)
        seqlens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
        want = bp.sense_decode(q, k_new, k_cache.clone(), table, rows.clone(), new_row, seqlens, dk ** -0.5)
        got = _sense_abi(bp, q, k_new, k_cache, table, rows, new_row, seqlens, dk ** -0.5, torch.empty_like(want),
                         buf[pad:pad + n])
        assert torch.equal(got, want)
        assert (buf[:pad] == SENTINEL).all() and (buf[pad + n:] == SENTINEL).all(), (b, k, dk, dout, max_s)


def test_softmax_lse_with_a_wider_batch_stride():
    """lse_batch_stride > nheads: only [b, :nheads] is written, with the values of the dense call."""
    bp = _bp()
    g = torch.Generator(device=DEV).manual_seed(17)
    b, h, d, max_s = 5, 6, 64, 1000
    q, k_new, v_new = (torch.randn(b, h, d, device=DEV, generator=g).bfloat16() for _ in range(3))
    cache = torch.randn(b, max_s, 2, h, d, device=DEV, generator=g).bfloat16()
    seqlens = torch.tensor([0, 999, 64, 500, 63], dtype=torch.int32, device=DEV)
    want_out, want_lse = bp.flash_decode(q, k_new, v_new, cache.clone(), seqlens, 0.125, return_lse=True)
    wide = torch.full((b, h + 5), SENTINEL, device=DEV)
    out = _flash_abi(bp, q, k_new, v_new, cache, seqlens, 0.125, torch.empty_like(want_out), wide)
    assert torch.equal(out, want_out) and torch.equal(wide[:, :h], want_lse) and (wide[:, h:] == SENTINEL).all()


def test_sense_decode_content_cache_beyond_4_gib():
    """The per-position content cache (batch * max_seqlen, k, d_out) passes 4 GiB at batch 256 of Small.  Here 5 samples
    x 4104 positions x 64 senses x 2048 = 5.0 GiB: sample 1 holds byte 2^31, sample 3 holds byte 2^32, so their visible rows
    lie on both sides of the marks.  Needle inputs: every output row must equal its own rows' sum bit for bit, which a
    32-bit row offset (rows 2^31 or 2^32 bytes too low) cannot give."""
    bp = _bp()
    dtype = torch.bfloat16
    b, max_s, k, dkp, dout = 5, 4104, 64, 16, 2048
    case = dict(max_seqlen=max_s)
    row_bytes = k * dout * 2
    table = torch.empty(b * max_s, k, dout, device=DEV, dtype=dtype)
    assert table.numel() * 2 > 2 ** 32
    li = _ar(k)[None, :]
    for r0 in range(0, b * max_s, 1026):                                            # filled in slices (fp32 temporaries)
        r1 = min(r0 + 1026, b * max_s)
        table[r0:r1] = N.sense_value(_ar(r1 - r0)[:, None] + r0, li, dout).to(dtype)
    marks = [2 ** 31 // row_bytes, 2 ** 32 // row_bytes]                           # rows holding the two marks
    assert marks[0] // max_s == 1 and marks[1] // max_s == 3
    L = 4096
    pos, bi = _ar(max_s), _ar(b)[:, None]
    keys = N.code(pos, 16, dkp).to(dtype)
    k_cache = keys[None, :, None, :].expand(b, max_s, k, dkp).contiguous()
    k_cache[:, L:] = NAN
    rows = N.sense_row(case, 'cache', bi, pos[None, :]).contiguous()
    new_row = rows[:, L].contiguous()
    seqlens = torch.full((b,), L, dtype=torch.int32, device=DEV)
    # needles: per sample the rows around each mark that falls into it, the ends, and spread positions
    jstar = ((_ar(k)[None, :] * 61 + bi * 7) % (L + 1))
    for m in marks:
        s, j = m // max_s, m % max_s
        assert 2 < j < L - 2
        jstar[s, :5] = torch.tensor([j - 2, j - 1, j, j + 1, j + 2], device=DEV)
    jstar[:, 5], jstar[:, 6] = 0, L
    q = N.code(jstar, 16, dkp).to(dtype)
    out = bp.sense_decode(q, keys[L].expand(b, k, dkp).contiguous(), k_cache, table, rows, new_row, seqlens, N.scale(16))
    r = N.sense_row(case, 'cache', bi, jstar).long()
    assert (r * row_bytes >= 2 ** 32).any() and ((r * row_bytes >= 2 ** 31) & (r * row_bytes < 2 ** 32)).any()
    want = torch.stack([table[r[i], li[0]].float().sum(dim=0) for i in range(b)]).to(dtype)
    assert torch.equal(out, want)


def test_flash_decode_kv_cache_beyond_2_31_elements():
    """A KV cache buffer of 180 samples x (4104, 2, 12, 128) holds 2.27e9 elements (4.5 GB): the call runs on its last 8
    samples, whose base offset alone is past 2^31 elements and 2^32 bytes, with needle inputs, so an element offset kept in
    32 bits reads other rows (NaN, or another position's value row) and changes bits."""
    bp = _bp()
    dtype = torch.float16
    nb, b, max_s, h, d = 180, 8, 4104, 12, 128
    case = dict(heads=h)
    full = torch.empty(nb, max_s, 2, h, d, device=DEV, dtype=dtype)
    off = nb - b
    assert off * full.stride(0) > 2 ** 31
    full.fill_(NAN)
    L = 4000
    pos, bi, hi = _ar(max_s), _ar(b)[:, None], _ar(h)[None, :]
    keys = N.code(pos, d).to(dtype)
    vals = N.values(N.trunk_value_ids(case, bi[:, :, None], hi[:, None, :], pos[None, :, None]), d).to(dtype)
    cache = full[off:]
    cache[:, :L, 0] = keys[None, :L, None, :]
    cache[:, :L, 1] = vals[:, :L]
    jstar = (hi * 331 + bi * 37) % (L + 1)
    jstar[:, 0], jstar[:, 1], jstar[:, 2] = 0, L, L - 1
    q = N.code(jstar, d).to(dtype)
    seqlens = torch.full((b,), L, dtype=torch.int32, device=DEV)
    k_new, v_new = keys[L].expand(b, h, d).contiguous(), vals[:, L].contiguous()
    out, lse = bp.flash_decode(q, k_new, v_new, cache, seqlens, N.scale(d), return_lse=True)
    assert torch.equal(out, vals[bi, jstar, hi])
    torch.testing.assert_close(lse, torch.full_like(lse, N.needle_score(d)), rtol=1e-5, atol=1e-4)
    assert torch.equal(cache[:, L, 0], k_new) and torch.equal(cache[:, L, 1], v_new)
    assert torch.isnan(full[:off]).all() and torch.isnan(cache[:, L + 1:]).all()
