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

What the construction cannot see: the NON-ZERO arithmetic of dQ, dK and dqk (tests/test_gpu_backward.py keeps that job),
dropout, and a row that takes the LSE of another row (all rows of a call have the same LSE).  A row that takes another
row's D is seen: D_i = dO_i . O_i differs from row to row.

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
# ... whose LSE is the logarithm of a sum of ROUNDED p (csrc/flash_fwd_dma.hip:282-285, 484): here of one bf16 number,
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
