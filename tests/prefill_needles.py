"""Needle inputs (tests/decode_needles.py) for the PREFILL forward and the BACKWARD kernels: tests/test_gpu_prefill_needles.py
and its CPU pre-check tests/test_prefill_needles_host.py share the maps, the case lists, the expected results and the
criteria below.

Key j is the +-1 code of its position within its sequence, query row i the code of a needle position j*(i) (a "map": a
fixed integer function of the row), softmax_scale = 24 / reps(width), values non-zero integers of magnitude 1 ... 8.  The
needle beats every other visible key by >= 48 nats, so in fp32 the output row is the needle's value row, the row LSE is
needle_score(width), P is 1.0 at (i, j*(i)) and < 1.5e-21 elsewhere.  Backward, with integer dO in {1, 2}:
dV[j] = sum of dO_i over {i : j*(i) = j} exactly (dust, ~1e-19, for a key that is nobody's needle), and dQ, dK are dust
because dS = P (dP - D) vanishes at the needle.  The same holds per sense for the sense mix: out = sum_l C[j*_l(i), l, :]
and dC[s, l, :] = sum of dout_t over {t : j*_l(t) = s}.

What a single needle cannot see is the NON-ZERO arithmetic of dQ, dK and dqk: with P = 1, dS = P (dP - D) vanishes.  The PAIR
problems in the second half of this file see it: two needles per row with bit-equal scores give P = 1/2, 1/2, dS = +- n / 4
with n = dP[i, j1] - dP[i, j2] an integer, and closed forms for O, LSE, dQ, dK, dV (per sense: dqk, dC) that the flash kernels
must return bit for bit and the sense backward within a derived rounding bound (pair_dqk_bounds) -- so one (query tile, key
tile) term of dK dropped or doubled, a dS term on the neighbouring key, scale misplaced in one tile and a wrong D for a slab
all change bits.  Partly seen now: a row that takes the LSE of another row (row 0 has one needle, hence another LSE than the
paired rows; among the paired rows of a call it is still one number); another row's D is seen (D_i = dO_i . O_i differs from
row to row).  Dropout, forward and backward, has its own exact tests: the pair problems run under p = 1/2 in
tests/test_gpu_dropout_exact.py (tests/dropout_exact.py).  A key tile with non-negligible weight that does not hold a needle --
the P V accumulation of a steady-state tile with 64 live probabilities, alpha = 1 across several live tiles, the ring
accumulation of the mix, more than one decode split that matters, dV / dC sums over dense P -- is what tests/tie_blocks.py builds
(tests/test_gpu_tie_blocks.py): up to 2048 keys tied bit for bit.  Still unseen: key_weight in the fused sense
backward, which has none (a weighted call takes the alpha-rebuilding route; the pair problem runs that route unweighted), and
non-unit rescale factors between live tiles (score steps between tiles are not exact powers of two under fl(scale log2e)).
tests/test_gpu_backward.py keeps the job on random data.

Everything is a fixed integer function of its indices (no generator state), on any device.
"""
import torch

import decode_needles as N
from decode_needles import _hash, code, max_length, needle_score, reps, scale, values

POS_STRIDE = N.POS_STRIDE
VOCAB = N.VOCAB
LOG2E = 1.4426950408889634
LSE_TOL = dict(rtol=1e-5, atol=1e-4)        # the decode tests' LSE tolerance (tests/test_gpu_decode_edges.py)
HALF_ULP = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}   # of a number just below 1.0: 1 - e rounds to 1.0 below it
ROUNDING = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}   # largest relative error of one rounding
DUST = 1e-12                                # |dV|, |dC| of a key that is nobody's needle (truth < 1e-18, a wrong row >= 1)
GRAD_DUST = 1e-6                            # |dQ|, |dK| (truth < 1e-15; 16-bit dS pipeline: 24 * 4096 * 2^-55 = 3e-12)

# ---- needle maps ----------------------------------------------------------------------------------------------------------

BWD_MAPS = ('diag', 'prev', 'tile0', 'prevtile_last', 'back128', 'hashwin')    # fan-in sums representable in 16 bit
FWD_MAPS = BWD_MAPS + ('first', 'hash')
CROSS_MAPS = ('mirror', 'last')                                                # non-causal only: j* may exceed the row
STALE_MAP = 'tile1'                                                            # see FLASH_STALE


def jstar(name, i, sk=None):
    """Needle position of rows i (integer tensor) under map `name`; sk: the number of keys (the non-causal maps)."""
    i = i.long()
    if name == 'diag':
        return i.clone()
    if name == 'prev':
        return (i - 1).clamp(min=0)
    if name == 'tile0':
        return i - i % 64
    if name == 'prevtile_last':
        return (i - i % 64 - 1).clamp(min=0)
    if name == 'back128':
        return (i - 128).clamp(min=0)
    if name == 'hashwin':
        return i - _hash(i) % (i + 1).clamp(max=192)
    if name == 'first':
        return torch.zeros_like(i)
    if name == 'hash':
        return _hash(i + 7919) % (i + 1)
    if name == 'mirror':
        return sk - 1 - i % sk
    if name == 'last':
        return torch.full_like(i, sk - 1)
    if name == 'tile1':
        return torch.where(i >= 128, 64 + i % 64, i)
    raise KeyError(name)


def slot_maps(maps, nslots, rot=0):
    """The map of each of `nslots` (sample, head) slots: the list rotated by `rot`."""
    return [maps[(s + rot) % len(maps)] for s in range(nslots)]


def rotations(maps, nslots):
    """Rotations after which every map has had a slot."""
    return range(0, len(maps), nslots)


def grad_rows(ids, width):
    """ids: integer tensor (...) -> float32 (..., width) of 1 or 2, a hash of (id, column): an upstream gradient."""
    h = _hash(ids.long()[..., None] * 4099 + torch.arange(width, device=ids.device) + 1237)
    return (1 + ((h >> 5) & 1)).float()


def fan_in(js, src, sk):
    """js (b, g, sq) needle of every row, src (b, sq, g, w) -> (sums (b, sk, g, w) fp64 of the rows whose needle each key
    is, count (b, sk, g))."""
    b, g, sq = js.shape
    idx = js.permute(0, 2, 1)
    sums = torch.zeros(b, sk, g, src.shape[-1], dtype=torch.float64, device=src.device)
    sums.scatter_add_(1, idx[..., None].expand(b, sq, g, src.shape[-1]), src.double())
    count = torch.zeros(b, sk, g, dtype=torch.int64, device=src.device)
    count.scatter_add_(1, idx, torch.ones_like(idx))
    return sums, count


# ---- attention problems ---------------------------------------------------------------------------------------------------

def attn_problem(maps, b, h, sq, sk, d, device='cpu', scale_num=24.0, slot0=0, cols=None):
    """One fixed-length call, all fp32: q (b, sq, h, d), k (b, sk, h, d), v / want / dout (b, s, h, w), js (b, h, sq),
    want_dv (fp64) and fan (count) (b, sk, h[, w]).  maps: one per (sample, head) slot; slot0: the first slot's number in
    the value ids (a key read from a neighbouring slot or sequence changes bits); cols: the first value columns only."""
    assert len(maps) == b * h and sk - 1 <= max_length(d)
    w = cols or d
    i, pos = torch.arange(sq, device=device), torch.arange(sk, device=device)
    js = torch.stack([jstar(m, i, sk) for m in maps]).view(b, h, sq).clamp(max=sk - 1)      # more rows than keys: the last key
    assert int(js.min()) >= 0
    slot = slot0 + torch.arange(b * h, device=device).view(b, 1, h)
    v = values(slot * POS_STRIDE + pos[None, :, None], w)
    dout = grad_rows(slot * POS_STRIDE + i[None, :, None], w)
    want_dv, fan = fan_in(js, dout, sk)
    s = scale_num / reps(d)
    return dict(q=code(js, d).permute(0, 2, 1, 3).contiguous(), k=code(pos, d)[None, :, None, :].expand(b, sk, h, d).contiguous(),
                v=v, js=js, want=torch.gather(v, 1, js.permute(0, 2, 1)[..., None].expand(b, sq, h, w)), dout=dout,
                want_dv=want_dv, fan=fan, scale=s, lse=s * d)


def ragged_problem(lens, h, d, maps, rot=0, device='cpu', cols=None):
    """A cu_seqlens batch (self-attention: the same lengths for queries and keys), tensors (total, h, .): position codes
    are relative to each sequence, value ids carry the sequence index.  Sequence n takes the maps rotated by rot + n."""
    parts = [attn_problem(slot_maps(maps, h, rot + n), 1, h, L, L, d, device, slot0=n * h, cols=cols)
             for n, L in enumerate(lens) if L > 0]
    out = {key: torch.cat([p[key][0] for p in parts]) for key in ('q', 'k', 'v', 'want', 'dout', 'want_dv', 'fan')}
    out['cu'] = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=device)
    out['scale'], out['lse'], out['parts'] = parts[0]['scale'], parts[0]['lse'], parts
    return out


FLASH_SEQLENS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 384, 385, 641)
FLASH_BWD_SEQLENS = (1, 64, 65, 128, 129, 256, 257, 384, 385, 641)
# d = 36 is not a multiple of 8: the register-staged csrc/flash_fwd.hip (32 code columns, the other four +1)
FLASH_FWD_CASES = [dict(d=d, seqlens=[s for s in FLASH_SEQLENS if s <= max_length(d)]) for d in (8, 16, 36, 40, 64, 80, 128)]
FLASH_BWD_CASES = [dict(d=d, seqlens=[s for s in FLASH_BWD_SEQLENS if s <= max_length(d)]) for d in (8, 16, 40, 64, 80, 128)]
FLASH_BH9 = dict(d=64, s=385, b=3, h=3)                 # 9 (sample, head) pairs: not a multiple of the 8 XCDs
FLASH_CROSS = dict(d=64, sq=150, sk=333, b=1, h=3)      # as test_flash_bwd_cross_lengths
FLASH_RAGGED = dict(d=64, h=2, lens=[70, 1, 130, 257, 5])
FLASH_BWD_RAGGED = dict(d=64, h=2, lens=[70, 1, 0, 130, 257, 5])
# softmax_scale = 9 / reps: rows i >= 128 with j* = 64 + i % 64 differ from key i % 64 of the first tile in one bit, so the
# needle's p is e^18 ~ 2^26 against the row's first-tile reference: under the 2^30 limit of the steady-state body of
# csrc/flash_fwd_dma.hip, which therefore keeps the stale reference (no retry).  bf16 only (the fp16 limit is 2^14).
FLASH_STALE = dict(d=64, s=641, b=1, h=3, scale_num=9.0)
# ... whose LSE is the logarithm of a sum of ROUNDED p (csrc/flash_fwd_dma.hip:282-285, 487): here of one bf16 number,
# e^18 = 250.4 * 2^18 -> 250 * 2^18, i.e. off by up to half a bf16 ulp, 2^-9, where a real row averages many roundings
STALE_LSE_TOL = dict(rtol=1e-5, atol=1e-4 + 2.0 ** -9)


def bh_of(s):
    """(batch, heads) with batch * heads = 3: the three slots as heads at even lengths, as samples at odd ones."""
    return (1, 3) if s % 2 == 0 else (3, 1)


def flash_failures(out, lse, prob, dtype, lse_tol=LSE_TOL):
    """Criterion of the forward: out == V[j*] bit for bit, LSE within the decode tolerance.  out (..., w) any float dtype
    (compared after rounding to `dtype`), lse broadcastable to prob rows or None.  Returns a list of complaints."""
    bad = []
    wrong = (out.to(dtype).float() != prob['want'].to(out.device)).any(dim=-1)
    if wrong.any():
        bad.append(f'{int(wrong.sum())} rows differ from their needle\'s value row, first at {wrong.nonzero()[0].tolist()}')
    if lse is not None:
        off = (lse.float() - prob['lse']).abs()
        tol = lse_tol['atol'] + lse_tol['rtol'] * abs(prob['lse'])
        if not (off <= tol).all():          # NaN fails too
            bad.append(f'LSE off by {off.max().item():.3e} > {tol:.3e}')
    return bad


def grad_failures(got, want, fan, dtype, name):
    """Criterion of an exact reduction (dV, dC): got (..., w) == want bit for bit where fan (...) > 0, |got| <= DUST
    elsewhere.  `want` is fp64 and must be representable in dtype (the host check asserts it)."""
    bad = []
    got = got.double()
    has = (fan > 0)[..., None].to(got.device)
    want = want.to(got.device)
    wrong = (has & (got.to(dtype).double() != want)).any(dim=-1)
    if wrong.any():
        bad.append(f'{name}: {int(wrong.sum())} rows with a fan-in differ from the sum of their rows, first at {wrong.nonzero()[0].tolist()}')
    loud = (~has & ~(got.abs() <= DUST)).any(dim=-1)
    if loud.any():
        bad.append(f'{name}: {int(loud.sum())} rows without a fan-in exceed {DUST}, first at {loud.nonzero()[0].tolist()}')
    return bad


def dust_failures(got, bound, name):
    """Criterion of a gradient that vanishes: |got| <= bound everywhere (bound: a number or a broadcastable tensor)."""
    got = got.double()
    bound = bound.to(got.device) if torch.is_tensor(bound) else bound
    ok = got.abs() <= bound
    if ok.all():
        return []
    return [f'{name}: {int((~ok).sum())} entries beyond their bound, max |.| {got.abs().nan_to_num(nan=float("inf")).max().item():.3e}']


# ---- sense problems -------------------------------------------------------------------------------------------------------

def value_cap(k):
    """Largest content value with k senses: every sum over senses stays an integer <= 256 (exact in bf16)."""
    return min(8, 256 // k)


def sense_problem(s, k, dk, dout, b=2, device='cpu', maps=FWD_MAPS, form='dense', weighted=False, cols=None, sparse=False,
                  pad=False):
    """One sense-mix call, all fp32.  Sense l of sample n takes maps[(l + n) % len(maps)].  qk (b, s, 2, k, dk), content
    (b, s, k, w) ('dense') or table (VOCAB, k, w) + rows (b, s) int32 ('gather', even rows only), key_weight (b, k, s)
    powers of two in {0.5, 1, 2} or None, want (b, s, w), js (b, k, s), dout (b, s, w) in {1, 2} (sparse: at most four
    non-zero columns per row), want_dc (fp64) / fan (b, s, k[, w]).  pad: qk zero-padded to a multiple of 8 columns, as
    ContextSelfAttn.project hands a narrow width to the backward kernels."""
    assert s - 1 <= max_length(dk)
    dkp = -(-dk // 8) * 8 if pad else dk
    w = cols or dout
    t = torch.arange(s, device=device)
    js = torch.stack([torch.stack([jstar(maps[(l + n) % len(maps)], t) for l in range(k)]) for n in range(b)])   # (b, k, s)
    qk = torch.empty(b, s, 2, k, dkp, device=device)
    qk[:, :, 0] = code(js, dk, dkp).permute(0, 2, 1, 3)
    qk[:, :, 1] = code(t, dk, dkp)[None, :, None, :]
    ids = torch.arange(b, device=device)[:, None] * POS_STRIDE + t[None, :]                                        # (b, s)
    senses = torch.arange(k, device=device)
    cap = value_cap(k)
    prob = dict(qk=qk, js=js, dk=dk, scale=scale(dk), lse=needle_score(dk), key_weight=None)
    if form == 'gather':
        rows = N.table_rows_of(ids, VOCAB)
        prob['rows'] = rows
        prob['table'] = (N.sense_value(torch.arange(VOCAB, device=device)[:, None], senses[None, :], w) - 1) % cap + 1
        content = prob['table'][rows.long()]
    else:
        content = (N.sense_value(ids[:, :, None], senses[None, None, :], w) - 1) % cap + 1
    prob['content'] = content                                                                                     # (b, s, k, w)
    picked = torch.gather(content, 1, js.permute(0, 2, 1)[..., None].expand(b, s, k, w))                          # C[b, j*_l(t), l, :]
    if weighted:
        kw = 2.0 ** ((_hash((ids[:, None, :] * 64 + senses[None, :, None])) % 3).float() - 1)                     # (b, k, s)
        prob['key_weight'] = kw
        picked = picked * torch.gather(kw, 2, js).permute(0, 2, 1)[..., None]
    prob['want'] = picked.sum(dim=2)
    if sparse:
        g = torch.zeros(b, s, w, device=device)
        for r in range(4):
            hsh = _hash(ids * 4 + r + 31337)
            g.scatter_(2, (hsh % w)[..., None], (1 + ((hsh >> 9) & 1)).float()[..., None])
        prob['dout'] = g
    else:
        prob['dout'] = grad_rows(ids, w)
    prob['want_dc'], prob['fan'] = fan_in(js, prob['dout'][:, :, None, :].expand(b, s, k, w), s)
    return prob


# (S, k, d_k, d_out): the narrow LDS-DMA ring (csrc/sense_mix_dma.hip) -- 257 = one 256-row tile + 1, 1100 = five tiles with
# a partial last one and a partial last 256-column chunk, d_k = 10 a zero-padded width
MIX_NARROW = [(257, 16, 48, 768), (641, 16, 48, 256), (1100, 4, 24, 104), (320, 64, 10, 640)]
MIX_STAGED = (200, 4, 24, 104)                       # content viewed at a 2-byte offset: csrc/sense_mix.hip
MIX_WIDE = [(352, 4, 160, 640), (352, 1, 640, 640), (333, 4, 160, 640)]   # ring, ring, staged (S % 32 != 0)
MIX_GATHER = [(641, 16, 48, 256), (352, 4, 160, 640)]
MIX_WEIGHTED = (1100, 4, 24, 104)
MIX_DC = MIX_NARROW + [(130, 64, 16, 640)]          # d_k = 10 zero-padded to 16 (sense_problem: pad)
MIX_DQK = [(200, 4, 24, 104), (257, 16, 48, 256), (641, 16, 16, 64)]
ALPHA_CASES = [(200, 4, 24), (320, 16, 48), (257, 64, 10), (96, 4, 160)]
PROBS_SK = (64, 200, 204, 333)                       # 16-byte, 16-byte, 8-byte and scalar stores of csrc/attn_probs.hip
PROBS_D = (16, 64, 80, 128)
PROBS_CROSS_SQ = 150


def probs_failures(p, js, causal, name):
    """Criterion of a probability matrix p (b, g, sq, sk): exactly 1.0 at (i, j*(i)), exactly 0 where masked (j > i when
    causal), <= 2e-21 elsewhere (e^-48 = 1.4e-21)."""
    bad = []
    p = p.float()
    js = js.to(p.device)
    sq, sk = p.shape[-2:]
    at = torch.gather(p, 3, js[..., None])
    if not (at == 1.0).all():
        bad.append(f'{name}: {int((at != 1.0).sum())} needle entries are not 1.0')
    rest = p.scatter(3, js[..., None], 0.0)
    if causal:
        upper = torch.triu(torch.ones(sq, sk, dtype=torch.bool, device=p.device), 1)
        if not (p[..., upper] == 0).all():
            bad.append(f'{name}: non-zero entries above the diagonal')
    if not (rest.abs() <= 2e-21).all():
        bad.append(f'{name}: max entry off the needles {rest.abs().nan_to_num(nan=float("inf")).max().item():.3e} > 2e-21')
    return bad


# ---- what 16-bit rounding does to the needle's own probability -----------------------------------------------------------------

def needle_p_error(width, softmax_scale=None):
    """Bound on |P - 1| of a needle in a kernel that rebuilds P = exp2(s * c2 - lse * log2e) in fp32 from the saved LSE
    (c2 = fl(scale * log2e), s = q . k = width exactly): the two fp32 products round apart unless scale and width are powers
    of two.  The exponent's rounding as the kernels compute it, + 2^-21 for the hardware exp2 and the fma."""
    s = torch.tensor(softmax_scale or scale(width), dtype=torch.float32)
    log2e = torch.tensor(LOG2E, dtype=torch.float32)
    c2 = (s * log2e).double()
    lse = torch.tensor((softmax_scale or scale(width)) * width, dtype=torch.float32)
    lse2 = (lse * log2e).double()
    worst = max(abs(float(width * c2 - lse2)), abs(float(width * c2 - lse.double() * LOG2E)),
                abs(float((width - (lse / s).double()) * c2)))
    return abs(2.0 ** worst - 1.0) + 2.0 ** -21


def dqk_bounds(prob, dtype):
    """Bounds on |dq| (a number) and |dk| (b, s, k, 1) of bp.sense_dqk on a needle problem, from an fp64 model of the
    arithmetic of csrc/sense_mix_bwd.hip (sense_dq_kernel, 'Row reference r[t]': lines 380-386 and 463-466).  With P_n =
    1 - e the needle's fp32 probability (e <= needle_p_error), dP_n its integer dP and r the row's 16-bit reference (a
    P-weighted mean of dP over the first 32 keys, so 0 <= r <= max dP):
        g_n = P_n (dP_n - r) is ROUNDED to 16 bit for the product with k,  D - r = g_n + r (P_n - 1) is not, so
        dq / scale = (rnd16(g_n) - g_n + r e) k_n:  |dq| <= scale (u (1 + e) max dP + e max dP), u = one rounding;
        dk: dS_n = P_n (dP_n - D), D = (1 - e) dP_n in fp32:  |dk[s]| <= scale * sum over the fan-in of (e dP_n + 64 * 2^-20).
    Both + GRAD_DUST for the other keys, and one more rounding of the stored result.  A row that takes the D of another row
    is off by scale * |dP_n - dP_n'| >= scale whenever the two differ, 1 / (64 u) = 4 (bf16) or 32 (fp16) times the dq bound."""
    u, e = ROUNDING[dtype], needle_p_error(prob['dk'], prob['scale'])
    dp = torch.einsum('btw,bslw->blts', prob['dout'].double(), prob['content'].double())          # (b, k, t, s)
    dp_n = torch.gather(dp, 3, prob['js'][..., None])[..., 0]                                     # (b, k, t)
    top = float(dp.max())
    assert top <= 64
    dq = prob['scale'] * top * (u * (1 + e) + e) * (1 + 2 * u) + GRAD_DUST
    per_row = (e * dp_n + 64 * 2.0 ** -20).permute(0, 2, 1)[..., None]                            # (b, t, k, 1)
    dk, _ = fan_in(prob['js'], per_row, dp.shape[-1])
    return dq, prob['scale'] * dk * (1 + 2 * u) ** 2 + GRAD_DUST


# ---- two needles per row: the NON-ZERO arithmetic of dQ, dK and dqk ------------------------------------------------------------
#
# The query of row i is code(j1) + code(j2), j1 = jstar(map, i), j2 = j1 ^ (1 << b): entries 0 (the reps columns of bit b) or
# +-2.  Keys j1 and j2 tie bit for bit at q . k = 2 (width - reps); a key that differs from j1 in another bit loses
# 4 reps scale = 48 nats or more.  So P = 1/2, 1/2 and < 1e-20 elsewhere, and with n_i = dP[i, j1] - dP[i, j2], an integer:
#     O_i = (V[j1] + V[j2]) / 2                    LSE_i = scale 2 (width - reps) + ln 2
#     dS[i, j1] = n_i / 4 = -dS[i, j2]             dQ_i = scale (n_i / 4) (K[j1] - K[j2])
#     dK_j = scale sum of (+- n_i / 4) Q_i         dV_j = sum of P dO_i       over the rows that have j as a needle
# A row without a partner (row 0 of a causal call) keeps one needle, q = 2 code(j1), P = 1, LSE = scale 2 width: another LSE
# than the paired rows have, so a row that takes row 0's LSE (or row 0 a neighbour's) is seen.

LN2 = 0.6931471805599453
# Where an expected entry is 0 the criterion is a bound, of three kinds (exact_failures takes it entry by entry):
#   * nothing but the < 1e-20 weights of the other keys contributes (a key that is nobody's needle, rows with n = 0: D comes from
#     the given O and is exact, so their dS is exactly 0): DUST for dV / dC / out, GRAD_DUST for dQ / dK, as for single needles;
#   * NON-ZERO terms t_i cancel (the tied columns of dQ, where dS_1 k_1 + dS_2 k_2 = n / 4 - n / 4; a key whose rows' n sum to 0;
#     V[j1] = -V[j2]): the exact sum is 0, but an fp32 accumulation that also takes in the others' -1e-21 is not obliged to return
#     it.  The matrix unit adds the products of one instruction in one aligned, truncating step: on bf16 inputs (fp16 cannot hold
#     1e-21 and gives exact zeros) the measured residue is -2^-24 of the group's largest product, e.g. 12 * 2^-23 = 1.4e-6 for
#     the terms 1, -2, 1 at scale 12.  Bound: FP32_SUM * sum |t_i| on top of the dust, which is what any fp32 summation of the t_i
#     with one-ulp steps may leave and 2^-21 of the smallest change a wrong term makes.
FP32_SUM = 2.0 ** -22
# value magnitude, non-zero dO columns per row, largest dO: what keeps every expected gradient representable (the host test
# asserts it case by case).  fp16 has 11 bits for the fan-in sums (|n| <= 16 keeps every map's dK exact; magnitude 8 with two
# dO columns does not: back128 reaches 10530), bf16 has 8, so its problem is the smaller one (|n| <= 4).
PAIR_MAGS = {torch.float16: dict(mag=4, ncols=1, top=2), torch.bfloat16: dict(mag=2, ncols=1, top=1)}
# the sense backward rebuilds D = sum P dP from P = (1 + e) / 2, so its dS is n / 4 + e (n / 4 - mean dP / 2): that rounds to
# n / 4 in 16 bit only while |e| |1 - 2 mean dP / n| stays under half an ulp, which the small problem does in both dtypes
PAIR_SENSE_MAGS = {torch.float16: dict(mag=2, ncols=1, top=1), torch.bfloat16: dict(mag=2, ncols=1, top=1)}
PAIR_FWD_MAGS = dict(mag=8, ncols=2, top=2)          # forward only: nothing but (V[j1] + V[j2]) / 2 has to be representable


def pair_scale(width):
    """Softmax scale of a pair problem: 12 / reps where that has one or two significant bits (12, 6, 4, 3, 2, 1.5: every
    product with the integers below stays exact), else the next power of two above it (widths 80, 160, 640: 4, 2, 0.5).
    4 reps scale >= 48 either way."""
    x = 12.0 / reps(width)
    m = x / 2.0 ** torch.tensor(x).log2().floor().item()
    return x if m in (1.0, 1.5) else 2.0 ** torch.tensor(x).log2().ceil().item()


def partner(js, i, nbits, limit=None):
    """Second needle of rows i whose first one is js: js ^ (1 << b) for the first bit b, counted DOWNWARDS (and around) from
    a start bit, whose partner is <= limit (default: i, the causal rule); js itself where there is none.  The start bit is
    _hash(31 i + 5) % nbits for half of the rows and one of the bits >= 6 for the other half, and a bit too high for the row
    falls to the next lower one: both so that pairs straddle 64-key tile borders often enough at S = 129 already, where only
    the rows >= 64 can (tests/test_prefill_needles_host.py asserts the shares)."""
    js, i = js.long(), i.long().expand_as(js)
    limit = i if limit is None else torch.as_tensor(limit, device=js.device).expand_as(js)
    h = _hash(31 * i + 5)
    start = h % nbits
    if nbits > 6:
        start = torch.where(((h >> 16) & 1) == 1, 6 + (h >> 17) % (nbits - 6), start)
    out = js.clone()
    found = torch.zeros_like(js, dtype=torch.bool)
    for step in range(nbits):
        cand = js ^ (1 << ((start - step) % nbits))
        take = ~found & (cand <= limit)
        out = torch.where(take, cand, out)
        found |= take
    return out


def pair_values(ids, width, mag):
    """decode_needles.values folded to magnitudes 1 ... mag (signs kept)."""
    v = values(ids, width)
    return v.sign() * ((v.abs() - 1) % mag + 1)


def sparse_grad(ids, width, ncols, top):
    """ids (...) -> float32 (..., width): an upstream gradient with at most `ncols` non-zero columns per row, each 1 ...
    top: dP = dO . V stays a small integer."""
    g = torch.zeros(*ids.shape, width, device=ids.device)
    for r in range(ncols):
        hsh = _hash(ids.long() * 4 + r + 31337)
        g.scatter_(-1, (hsh % width)[..., None], (1 + ((hsh >> 9) % top)).float()[..., None])
    return g


def _rows_of(x, js):
    """x (b, s, g, w), js (b, g, t) -> x[b, js[b, g, t], g, :] as (b, t, g, w)."""
    return torch.gather(x, 1, js.permute(0, 2, 1)[..., None].expand(js.shape[0], js.shape[2], js.shape[1], x.shape[-1]))


def _pair_closed_forms(q, k, v, dout, js, js2, s, sk, keep=None):
    """fp64 closed forms of a pair problem: q, dout (b, t, g, .), k, v (b, sk, g, .), js / js2 (b, g, t).

    keep: None (no dropout) or the keep bits (k1, k2) of every row's two needles, bool (b, g, t), under dropout with p = 1/2
    (tests/dropout_exact.py): Z = 2 k is 0 or 2 and, with P = w (1/2, 1/2; 1, 0 for a row without a partner),
        O = w1 Z1 V[j1] + w2 Z2 V[j2]      D = dO . O = w1 Z1 dP1 + w2 Z2 dP2      dS_x = w_x (Z_x dP_x - D)
        dQ = scale (dS1 K[j1] + dS2 K[j2])      dK_j = scale sum dS Q_i      dV_j = sum w Z dO_i
    i.e. O = k1 V[j1] + k2 V[j2], dS1 = k1 dP1 - D / 2 for a paired row and O = 2 k V[j1], dS = 0 for an unpaired one.  Z = 1
    gives the forms of the head of this section: dS1 = (dP1 - dP2) / 4 = -dS2."""
    q, k, v, dout = q.double(), k.double(), v.double(), dout.double()
    paired = (js2 != js).permute(0, 2, 1)[..., None]                                # (b, t, g, 1)
    w1, w2 = torch.where(paired, 0.5, 1.0), torch.where(paired, 0.5, 0.0)
    z1 = z2 = torch.ones_like(w1)
    if keep is not None:
        z1, z2 = (2.0 * kk.permute(0, 2, 1)[..., None].to(w1) for kk in keep)
    v1, v2 = _rows_of(v, js), _rows_of(v, js2)
    dp1, dp2 = (v1 * dout).sum(-1, keepdim=True), (v2 * dout).sum(-1, keepdim=True)
    n = torch.where(paired, dp1 - dp2, 0.0)                                         # dP[i, j1] - dP[i, j2]
    dd = w1 * z1 * dp1 + w2 * z2 * dp2                                              # D
    ds1, ds2 = w1 * (z1 * dp1 - dd), w2 * (z2 * dp2 - dd)
    dk1, _ = fan_in(js, ds1 * q, sk)
    dk2, _ = fan_in(js2, ds2 * q, sk)
    dv1, c1 = fan_in(js, w1 * z1 * dout, sk)
    dv2, c2 = fan_in(js2, w2 * z2 * dout, sk)
    k1, k2 = _rows_of(k, js), _rows_of(k, js2)
    abs_dk = fan_in(js, ds1.abs() * q.abs(), sk)[0] + fan_in(js2, ds2.abs() * q.abs(), sk)[0]
    return dict(want=w1 * z1 * v1 + w2 * z2 * v2, n=n[..., 0], want_dq=s * (ds1 * k1 + ds2 * k2), want_dk=s * (dk1 + dk2),
                want_dv=dv1 + dv2, fan=c1 + c2, zero_out=DUST + FP32_SUM * (w1 * z1 * v1.abs() + w2 * z2 * v2.abs()),
                zero_dq=GRAD_DUST + s * FP32_SUM * (ds1.abs() * k1.abs() + ds2.abs() * k2.abs()),
                zero_dk=GRAD_DUST + s * FP32_SUM * abs_dk)


def pair_lse(js, js2, width, s):
    """Natural-log LSE of every row (fp64, shaped like js): two tied needles, or the single needle of an unpaired row."""
    return torch.where(js2 != js, s * 2 * (width - reps(width)) + LN2, s * 2.0 * width).double()


def pair_attn_problem(maps, b, h, sq, sk, d, device='cpu', mag=8, ncols=2, top=2, causal=True, slot0=0, cols=None):
    """attn_problem with two needles per row (mag, ncols, top: PAIR_MAGS[dtype]).  The same keys, plus js2 (b, h, sq), n
    (b, sq, h), lse PER ROW (b, h, sq) and the fp64 closed forms want_dq (b, sq, h, d), want_dk (b, sk, h, d), want_dv."""
    assert len(maps) == b * h and sk - 1 <= max_length(d)
    w = cols or d
    i, pos = torch.arange(sq, device=device), torch.arange(sk, device=device)
    js = torch.stack([jstar(m, i, sk) for m in maps]).view(b, h, sq).clamp(max=sk - 1)
    assert int(js.min()) >= 0
    js2 = partner(js, i, max((sk - 1).bit_length(), 1), None if causal else sk - 1)
    slot = slot0 + torch.arange(b * h, device=device).view(b, 1, h)
    v = pair_values(slot * POS_STRIDE + pos[None, :, None], w, mag)
    dout = sparse_grad(slot * POS_STRIDE + i[None, :, None], w, ncols, top)
    s = pair_scale(d)
    q = (code(js, d) + code(js2, d)).permute(0, 2, 1, 3).contiguous()
    k = code(pos, d)[None, :, None, :].expand(b, sk, h, d).contiguous()
    prob = dict(q=q, k=k, v=v, js=js, js2=js2, dout=dout, scale=s, lse=pair_lse(js, js2, d, s), width=d)
    prob.update(_pair_closed_forms(q, k, v, dout, js, js2, s, sk))
    return prob


def pair_ragged_problem(lens, h, d, maps, rot=0, device='cpu', cols=None, **mags):
    """ragged_problem with two needles per row; 'lse' is a list, one (h, L) tensor per sequence (None for an empty one)."""
    parts = [pair_attn_problem(slot_maps(maps, h, rot + n), 1, h, L, L, d, device, slot0=n * h, cols=cols, **mags)
             if L > 0 else None for n, L in enumerate(lens)]
    full = [p for p in parts if p is not None]
    out = {key: torch.cat([p[key][0] for p in full]) for key in ('q', 'k', 'v', 'want', 'dout', 'want_dq', 'want_dk', 'want_dv', 'fan',
                                                                 'zero_out', 'zero_dq', 'zero_dk')}
    out['cu'] = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=device)
    out['scale'], out['parts'] = full[0]['scale'], full
    out['lse'] = [p['lse'][0] if p is not None else None for p in parts]
    return out


def pair_sense_problem(s, k, dk, dout, b=2, device='cpu', maps=BWD_MAPS, mag=2, ncols=1, top=1, pad=False):
    """sense_problem ('dense', no key_weight) with two needles per (sense, row): qk, content, js, dout (sparse), want as
    there, plus js2 (b, k, s), n (b, s, k), lse PER ROW (b, k, s) and the fp64 closed forms want_dqk (like qk) and want_dc.
    Content values are signed, of magnitude <= min(mag, 128 / k): a sum over senses of half-integers stays exact in bf16."""
    assert s - 1 <= max_length(dk)
    dkp = -(-dk // 8) * 8 if pad else dk
    t = torch.arange(s, device=device)
    js = torch.stack([torch.stack([jstar(maps[(l + n) % len(maps)], t) for l in range(k)]) for n in range(b)])   # (b, k, s)
    js2 = partner(js, t, max((s - 1).bit_length(), 1))
    sc = pair_scale(dk)
    q = (code(js, dk, dkp) + code(js2, dk, dkp)).permute(0, 2, 1, 3)
    key = code(t, dk, dkp)[None, :, None, :].expand(b, s, k, dkp)
    ids = torch.arange(b, device=device)[:, None] * POS_STRIDE + t[None, :]
    content = pair_values(ids[:, :, None] * 64 + torch.arange(k, device=device), dout, min(mag, max(128 // k, 1)))
    g = sparse_grad(ids, dout, ncols, top)
    forms = _pair_closed_forms(q, key, content, g[:, :, None, :].expand(b, s, k, dout), js, js2, sc, s)
    return dict(qk=torch.stack([q, key], dim=2).contiguous(), content=content, js=js, js2=js2, dk=dk, scale=sc, dout=g,
                lse=pair_lse(js, js2, dk, sc), key_weight=None, want=forms['want'].sum(dim=2), n=forms['n'],
                want_dqk=torch.stack([forms['want_dq'], forms['want_dk']], dim=2), want_dc=forms['want_dv'], fan=forms['fan'],
                zero_out=DUST + (forms['zero_out'] - DUST).sum(dim=2), zero_dqk=torch.stack([forms['zero_dq'], forms['zero_dk']], dim=2))


def exact_failures(got, want, dtype, name, zero_bound=DUST):
    """Criterion of an exactly known result: where want != 0, got rounded to `dtype` == want bit for bit; where want == 0,
    |got| <= zero_bound (a number or a broadcastable tensor: what the 1e-20 weights of the other keys may leave, and where
    non-zero terms cancel the zero_* entry of the problem, see FP32_SUM).  `want` is
    fp64 and must be representable in dtype (the host check asserts it)."""
    got = got.double()
    want = want.to(got.device)
    bound = zero_bound.to(got.device) if torch.is_tensor(zero_bound) else zero_bound
    bad = []
    wrong = (want != 0) & (got.to(dtype).double() != want)
    if wrong.any():
        at = wrong.nonzero()[0].tolist()
        bad.append(f'{name}: {int(wrong.sum())} non-zero entries differ from the closed form, first at {at}: '
                   f'{got[tuple(at)].item()!r} for {want[tuple(at)].item()!r}')
    loud = (want == 0) & ~(got.abs() <= bound)
    if loud.any():
        at = loud.nonzero()[0].tolist()
        bad.append(f'{name}: {int(loud.sum())} entries that should vanish exceed their bound, first at {at}: {got[tuple(at)].item()!r}')
    return bad


def near_failures(got, want, bound, name):
    """|got - want| <= bound (broadcastable) everywhere."""
    off = (got.double() - want.to(got.device)).abs()
    ok = off <= (bound.to(got.device) if torch.is_tensor(bound) else bound)
    if ok.all():
        return []
    at = (~ok).nonzero()[0].tolist()
    return [f'{name}: {int((~ok).sum())} entries further from the closed form than their bound, first at {at}: off by '
            f'{off[tuple(at)].item():.3e}']


def lse_failures(lse, want, name='LSE'):
    off = (lse.double() - want.to(lse.device)).abs()
    ok = off <= LSE_TOL['atol'] + LSE_TOL['rtol'] * want.to(lse.device).abs()
    return [] if ok.all() else [f'{name} off by {off.nan_to_num(nan=float("inf")).max().item():.3e}']


def pair_p_error(width, softmax_scale):
    """needle_p_error for the scores of a pair problem: the largest relative error of a probability rebuilt in fp32 as
    exp2(s c2 - lse log2e) from the closed-form LSE, over the paired rows (s = 2 (width - reps), P = 1/2) and the unpaired
    ones (s = 2 width, P = 1)."""
    sc = torch.tensor(softmax_scale, dtype=torch.float32)
    log2e = torch.tensor(LOG2E, dtype=torch.float32)
    c2 = (sc * log2e).double()
    worst = 0.0
    for score, extra, ideal in ((2 * (width - reps(width)), LN2, -1.0), (2 * width, 0.0, 0.0)):
        lse = torch.tensor(softmax_scale * score + extra, dtype=torch.float32)
        lse2 = (lse * log2e).double()
        worst = max(worst, abs(float(score * c2 - lse2) - ideal), abs(float(score * c2 - lse.double() * LOG2E) - ideal))
    return abs(2.0 ** worst - 1.0) + 2.0 ** -21


def pair_dqk_bounds(prob, dtype):
    """What bp.sense_dqk may legitimately leave on a pair problem, from an fp64 model of csrc/sense_mix_bwd.hip (the host
    test runs that model).  P_1 = P_2 = (1 + e) / 2, |e| <= E = pair_p_error; u = one 16-bit rounding; r the row's 16-bit
    reference, between the smallest and the largest dP the row can see (spread = their difference, top = max |dP|).

    dq (sense_dq_kernel): g_j = P_j (dP_j - r) is rounded to 16 bit for A1 = sum g_j k_j but not inside D - r = g_1 + g_2 +
    r (P_1 + P_2 - 1), which multiplies A2 = (k_1 + k_2) / 2.  |g_1| + |g_2| <= (1 + E) spread, g_1 - g_2 = n / 2 up to
    E spread, so  |dq / scale - closed form| <= u (1 + E) spread + E spread + E top =: err  in every column, the tied ones
    (closed form 0) and the reps columns of the flipped bit alike; fp32 products add 2^-20 of the same.  The stored 16-bit
    number is then within 2 err of a representable closed form.  -> bound (b, s, k, 1), to be < scale / 8: a wrong term
    moves dq by a multiple of scale / 2.

    dk (sense_dk_kernel): dS_j = P_j (dP_j - D) with D = fmaf(r, sum P, sum g) = (1 + e) mean dP, so dS = +- n / 4 + e (+- n / 4
    - mean dP / 2), rounded to 16 bit.  A row with n != 0 snaps to +- n / 4 there, but a row with n = 0 leaves e mean dP / 2, which
    16 bit hold, and the key's sum collects one such term per row: next to a NON-ZERO closed form as well, where fp16 (ulp 2^-8
    at 6) shows what bf16 rounds away.  So dk is held to |dk - closed form| <= bound (b, s, k, 1) = 2 scale * sum over the key's
    rows of 2 E (1 + E) (|n| / 4 + |mean| / 2), not to bit equality; the bound is < scale / 8 as well, and wherever it is below
    the spacing of the 16-bit numbers around the closed form it IS bit equality, the result being such a number."""
    u, e = ROUNDING[dtype], pair_p_error(prob['dk'], prob['scale'])
    dp = torch.einsum('btw,bslw->blts', prob['dout'].double(), prob['content'].double())          # (b, k, t, s)
    s = dp.shape[-1]
    seen = torch.tril(torch.ones(s, s, dtype=torch.bool, device=dp.device))
    inf = torch.tensor(float('inf'), dtype=torch.float64, device=dp.device)
    hi, lo = torch.where(seen, dp, -inf).max(-1).values, torch.where(seen, dp, inf).min(-1).values   # (b, k, t)
    top = torch.maximum(hi.abs(), lo.abs())
    err = (u * (1 + e) + e) * (hi - lo) + e * top + 2.0 ** -20 * (hi - lo + top)
    dq = (2 * prob['scale'] * err + GRAD_DUST).permute(0, 2, 1)[..., None]
    dp1 = torch.gather(dp, 3, prob['js'][..., None])[..., 0]
    dp2 = torch.gather(dp, 3, prob['js2'][..., None])[..., 0]
    per_row = 2 * (e * (1 + e) * ((dp1 - dp2).abs() / 4 + (dp1 + dp2).abs() / 4) + 2.0 ** -20 * top) * (1 + u)
    per_row = per_row.permute(0, 2, 1)[..., None]
    dk = fan_in(prob['js'], per_row, s)[0] + fan_in(prob['js2'], per_row, s)[0]
    return dq, 2 * prob['scale'] * dk * (1 + 2 * u) + GRAD_DUST


def pair_maps(d, dtype, s):
    """The backward maps whose expected dK a causal pair problem of head dimension d and length s can hold in `dtype`: all
    of them in fp16; in bf16 (8 bits) a high fan-in map drops out at the (d, s) where the host check
    (test_pair_bf16_exclusions_are_the_unrepresentable_ones) finds a sum that is not representable."""
    if dtype == torch.float16:
        return BWD_MAPS
    return tuple(m for m in BWD_MAPS if (m, d, s) not in PAIR_BF16_LEFT_OUT)


# (map, d, S) left out in bf16: with the map in any of the three slots some dK sum needs more than 8 bits.  tile0 and
# prevtile_last (the fan-in of a whole 64-row tile) stay at d = 64 for most lengths and at d = 80, 128 for all.
PAIR_BF16_LEFT_OUT = frozenset([
    ('tile0', 8, 129), ('back128', 8, 129), ('tile0', 16, 129), ('back128', 16, 129), ('tile0', 16, 257), ('back128', 16, 257),
    ('tile0', 16, 385), ('back128', 16, 385), ('tile0', 16, 641), ('prevtile_last', 16, 641), ('back128', 16, 641),
    ('back128', 40, 129), ('tile0', 40, 257), ('back128', 40, 257), ('tile0', 40, 385), ('back128', 40, 385), ('tile0', 40, 641),
    ('back128', 40, 641), ('tile0', 64, 385), ('prevtile_last', 64, 641)])
PAIR_RAGGED_BF16_LEFT_OUT = ('prevtile_last',)      # key 63 of the 257-row sequence (slot 7): not representable in bf16
PAIR_SEQLENS = (65, 129, 257, 385, 641)
PAIR_BWD_CASES = [dict(d=c['d'], seqlens=[s for s in c['seqlens'] if s in PAIR_SEQLENS]) for c in FLASH_BWD_CASES]
PAIR_CHAIN = dict(d=64, s=385)
PAIR_FWD_CASES = [dict(d=d, seqlens=[s for s in (129, 385, 641) if s <= max_length(d)]) for d in (8, 36, 64, 128)]
PAIR_MIX_DQK = [(200, 4, 24, 104), (257, 16, 48, 256), (641, 16, 16, 64), (130, 64, 10, 640)]     # d_k = 10 zero-padded to 16
PAIR_SENSE_BF16_LEFT_OUT = {(641, 16, 16, 64): ('tile0', 'prevtile_last')}   # dk sums that bf16 cannot hold (the host test shows it)


def pair_sense_maps(shape, dtype):
    left_out = PAIR_SENSE_BF16_LEFT_OUT.get(tuple(shape), ()) if dtype == torch.bfloat16 else ()
    return tuple(m for m in BWD_MAPS if m not in left_out)


PAIR_MIX_FWD = [(257, 16, 48, 768), (352, 4, 160, 640)]
PAIR_MIX_WIDE = (352, 4, 160, 640)                                                                  # the alpha-rebuilding route


def pair_fixed_problems(dtype, device='cpu', cases=None, mags=None):
    """(tag, problem) of every fixed-length causal pair call in `dtype`: per (d, S) the admissible maps three at a time."""
    for case in PAIR_BWD_CASES if cases is None else cases:
        for s in case['seqlens']:
            maps = pair_maps(case['d'], dtype, s)
            b, h = bh_of(s)
            for rot in rotations(maps, 3):
                yield (f"d={case['d']} S={s} maps from {rot}",
                       pair_attn_problem(slot_maps(maps, 3, rot), b, h, s, s, case['d'], device, **(mags or PAIR_MAGS[dtype])))


def pair_cross_problems(dtype, device='cpu'):
    """FLASH_CROSS without the causal mask: partners anywhere among the keys, needles behind the row included."""
    c = FLASH_CROSS
    maps = CROSS_MAPS + BWD_MAPS           # sq = 150 rows: every map's sums are representable in both dtypes
    for rot in rotations(maps, 3):
        yield (f'cross maps from {rot}', pair_attn_problem(slot_maps(maps, 3, rot), c['b'], c['h'], c['sq'], c['sk'], c['d'],
                                                          device, causal=False, **PAIR_MAGS[dtype]))


def pair_ragged_problems(dtype, device='cpu'):
    c = FLASH_BWD_RAGGED
    maps = tuple(m for m in BWD_MAPS if dtype == torch.float16 or m not in PAIR_RAGGED_BF16_LEFT_OUT)
    for rot in rotations(maps, c['h']):
        yield f'ragged maps from {rot}', pair_ragged_problem(c['lens'], c['h'], c['d'], maps, rot, device, **PAIR_MAGS[dtype])
