"""Softmax problems with MANY equal weights, for tests/test_gpu_tie_blocks.py and its CPU proof tests/test_tie_blocks_host.py.

The needle and pair problems (tests/prefill_needles.py) put a row's weight on one key or two; every other visible key weighs
< 1.5e-21, so a key tile that does not hold the needle may be weighted wrongly without a bit changing.  Here a row's weight
lies on up to 2048 keys, equal bit for bit, so every live tile, every 16-key group of it and every split counts.

Construction.  Keys keep the +-1 position codes of decode_needles.code (of position + `off`: an offset of 32 puts the aligned
64-blocks of the code across two 64-key tiles).  A TIE QUERY OF ORDER m is the code of a position with the columns of the low m
position bits set to 0 in every repetition and the filler columns behind nbits * reps set to 0 as well.  Its dot product with
a key is an integer, reps * (number of agreeing - disagreeing high bits): the 2^m keys of the aligned block that shares the
high bits score reps * (nbits - m), bit-equal, every other key at least 2 reps less, i.e. 2 reps scale = 48 nats.  Rows:

  full block   row i names the last aligned 2^m-block wholly at or before i (map 'full<m>'; 'early<m>': an earlier one by a
               hash of the row; 'head<m>': the first one; a row with no such block yet takes the largest order below m that has one, down to the single
               key i): P = 2^-m' exactly on 2^m' keys, LSE = scale reps (nbits - m') + m' ln 2
  own block    row i names the block that contains i ('own<m>'): causality cuts it to its first r = i % 2^m + 1 keys, P = 1 / r
  flat         order m = nbits: the query is 0, every visible key scores 0, P = 1 / (i + 1), LSE = ln(i + 1)

Values are non-zero integers of magnitude 1 ... mag (TIE_MAGS: 8 in fp16, 2 in bf16, so that the mean of up to 128 of them,
sum / 2^m with |sum| <= 2^m mag, is REPRESENTABLE in the dtype: the expected output of a full-block row is then the exact mean,
no rounding, hence no rounding tie that the matrix unit's truncating add of a few 1e-21 weights could break the other way --
prefill_needles.FP32_SUM has the measurement).  Flat and own-block problems carry in their first eight value columns the +-1
code of the key's low eight position bits: a prefix sum of column c stays within +-2^c, so one key lost, doubled or taken
from another position moves sum / n by 1 / n, 2^-c of the entry or more: an ulp of bf16 at c = 7, more below.

Expected results come from the dense fp64 P (b, g, sq, sk), known exactly; `mean_failures` holds a result to bit equality with
the 16-bit rounding of the fp64 number wherever that rounding is the same over the whole interval a correct fp32 evaluation can
land in, and to one of the two neighbours where it is not (1 / n rows only; the host test counts those rows: <= 10 %).

Everything is a fixed integer function of its indices (no generator state), on any device.
"""
import functools
import math
import re

import torch

import decode_needles as N
import prefill_needles as P
from decode_needles import _hash, code, max_length, reps, scale

POS_STRIDE = N.POS_STRIDE
TIE_MAGS = {torch.float16: 8, torch.bfloat16: 2}
# What a correct fp32 evaluation of sum / n may be off by, relatively: the sum of <= 2048 integers of magnitude <= 8 is exact
# (< 2^24); 1.f / l (csrc/flash_fwd_dma.hip:483, one rounding, or one ulp of a hardware reciprocal: 2^-23), the product with it
# (:501, 2^-24) and the matrix unit's truncating add next to 1e-21 weights (2^-24, prefill_needles.FP32_SUM): 2^-22 in all.
FP32_MEAN = 2.0 ** -21

FULL_MAPS = ('full4', 'full6+32', 'full7')          # m = 4; m = 6 across two tiles; m = 7: two whole tiles
EARLY_MAPS = ('early4', 'early6+32', 'early7')
FWD_MAPS = FULL_MAPS + ('own6', 'flat') + EARLY_MAPS + ('own6',)      # nine: three calls of three slots
BWD_MAPS = FULL_MAPS + EARLY_MAPS
CROSS_MAPS = EARLY_MAPS + FULL_MAPS[:2] + ('flat',)


def parse(name):
    """'full6+32' -> (kind, m, off)."""
    kind, m, off = re.fullmatch(r'([a-z]+)(\d*)(?:\+(\d+))?', name).groups()
    return kind, int(m or 0), int(off or 0)


def tie_query(pos, m, width, padded=None):
    """pos, m integer tensors (...) -> float32 (..., padded or width): the tie query of order m of each position (m >= nbits: 0)."""
    nbits, r = min(width, 16), reps(width)
    q = code(pos, width, padded)
    bit = torch.arange(nbits, device=pos.device).repeat(r)
    q[..., :nbits * r] *= (bit >= m.long()[..., None]).float()
    q[..., nbits * r:] = 0.0
    return q


def rows_of(name, sq, sk, width, causal=True, device='cpu'):
    """The tied keys of every row under map `name`: (pos, m, base, n), integer tensors (sq,).  The query of row i is
    tie_query(pos, m) in the code space of its slot (key j has the code of j + off) and its tied keys are base ... base + n - 1."""
    return rows_at(name, torch.arange(sq, device=device), sk, width, causal)


def rows_at(name, i, sk, width, causal=True, salt=0):
    """rows_of for the rows i (integer tensor); salt (a number or a tensor like i) varies the block an 'early' map picks."""
    kind, m, off = parse(name)
    nbits = min(width, 16)
    assert sk - 1 + off < 2 ** nbits and m <= nbits          # distinct codes
    last = i.clamp(max=sk - 1) if causal else torch.full_like(i, sk - 1)
    if kind == 'flat':
        return torch.zeros_like(i), torch.full_like(i, nbits), torch.zeros_like(i), last + 1
    if kind == 'own':
        assert causal and off == 0
        base = last - last % (1 << m)
        return base, torch.full_like(i, m), base, last - base + 1
    x = last + off
    pos, order = x.clone(), torch.zeros_like(i)                    # order 0: the single key `last` ('head0': key 0)
    if kind == 'head':
        pos = torch.full_like(x, off)
    for mm in range(1, m + 1):
        first = -(-off >> mm) << mm                                # first aligned block wholly behind the offset
        base_c = (((x + 1) >> mm) - 1) << mm
        ok = base_c >= first
        if kind == 'head':
            base_c = torch.full_like(base_c, first)                     # the first block of the sequence
        if kind == 'early':
            base_c = base_c - ((_hash(i * 131 + mm + salt * 7919) % (((base_c - first) >> mm).clamp(min=0) + 1)) << mm)
        pos, order = torch.where(ok, base_c, pos), torch.where(ok, mm, order)
    return pos, order, pos - off, 1 << order


def dense_p(base, n, sk):
    """fp64 (..., sq, sk): 1 / n on base ... base + n - 1, 0 elsewhere."""
    j = torch.arange(sk, device=base.device)
    live = (j >= base[..., None]) & (j < (base + n)[..., None])
    return live.double() / n[..., None].double()


def _mean(p, n, x, pattern):
    """sum_j p x as (sum over the tied keys of x) / n: the integer sum first, so that a sum of 0 is 0 and not 1e-17."""
    return torch.einsum(pattern, (p > 0).double(), x) / n.double().permute(0, 2, 1)[..., None]


def tie_values(ids, pos, width, mag, coded):
    """Value rows (..., width): decode_needles.values folded to magnitude <= mag; coded: the first eight columns (all of a
    narrower row) are the +-1 code of the low eight bits of `pos`."""
    v = P.pair_values(ids, width, mag)
    if coded:
        c = min(8, width)
        v[..., :c] = code(pos, 8)[..., :c]
    return v


def attn_problem(maps, b, h, sq, sk, d, dtype, device='cpu', causal=True, slot0=0, cols=None, sparse=False):
    """One fixed-length call, inputs fp32: q (b, sq, h, d), k (b, sk, h, d), v / dout (b, s, h, w); p (b, h, sq, sk) fp64, the
    exact probabilities; lse (b, h, sq) fp64; n (b, h, sq) the tie counts; the fp64 closed forms want, want_dq, want_dk,
    want_dv and abs_* (the same sums over magnitudes, for the bounds).  maps: one per (sample, head) slot; coded value columns
    where a slot's map is not a full-block one; sparse: dout has ONE non-zero column per row, a 1 (prefill_needles.sparse_grad),
    which keeps dP - D short: exact_grad_slots."""
    assert len(maps) == b * h
    w = cols or d
    i, pos = torch.arange(sq, device=device), torch.arange(sk, device=device)
    q, k, v, pp, lse, cnt, dots = [], [], [], [], [], [], []
    s = scale(d)
    for slot, name in enumerate(maps):
        kind, _, off = parse(name)
        qpos, m, base, n = rows_of(name, sq, sk, d, causal, device)
        q.append(tie_query(qpos, m, d))
        k.append(code(pos + off, d))
        v.append(tie_values((slot0 + slot) * POS_STRIDE + pos, pos, w, TIE_MAGS[dtype], kind in ('own', 'flat')))
        pp.append(dense_p(base, n, sk))
        lse.append(s * reps(d) * (min(d, 16) - m).double() + n.double().log())
        cnt.append(n)
        dots.append(reps(d) * (min(d, 16) - m))
    shape = lambda xs: torch.stack(xs).view(b, h, *xs[0].shape)
    q, k, v = (shape(x).permute(0, 2, 1, 3).contiguous() for x in (q, k, v))
    slot = slot0 + torch.arange(b * h, device=device).view(b, 1, h)
    ids = slot * POS_STRIDE + i[None, :, None]
    dout = P.sparse_grad(ids, w, 1, 1) if sparse else P.grad_rows(ids, w)
    prob = dict(q=q, k=k, v=v, dout=dout, p=shape(pp), lse=shape(lse), n=shape(cnt), dot=shape(dots), width=d, scale=s, maps=tuple(maps), causal=causal)
    prob.update(closed_forms(prob))
    return prob


def closed_forms(prob):
    """fp64: O = P V, D = dO . O, dS = P (dO V^T - D), dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO."""
    p = prob['p']
    q, k, v, do = (prob[x].double() for x in ('q', 'k', 'v', 'dout'))
    want = _mean(p, prob['n'], v, 'bhts,bshw->bthw')
    dp = torch.einsum('bthw,bshw->bhts', do, v)
    dd = (do * want).sum(-1).permute(0, 2, 1)
    ds = p * (dp - dd[..., None])
    return dict(want=want, abs_want=_mean(p, prob['n'], v.abs(), 'bhts,bshw->bthw'),
                want_dq=prob['scale'] * torch.einsum('bhts,bshd->bthd', ds, k),
                abs_dq=prob['scale'] * torch.einsum('bhts,bshd->bthd', ds.abs(), k.abs()),
                want_dk=prob['scale'] * torch.einsum('bhts,bthd->bshd', ds, q),
                abs_dk=prob['scale'] * torch.einsum('bhts,bthd->bshd', ds.abs(), q.abs()),
                want_dv=torch.einsum('bhts,bthw->bshw', p, do), ds=ds)


def ragged_problem(lens, h, d, maps, rot, dtype, device='cpu', cols=None):
    """A cu_seqlens batch as prefill_needles.ragged_problem: tensors (total, h, .), 'parts' the per-sequence problems (their
    p, lse and n stay per part); sequence n takes the maps rotated by rot + n and value ids that carry its index."""
    parts = [attn_problem(P.slot_maps(maps, h, rot + n), 1, h, L, L, d, dtype, device, slot0=n * h, cols=cols)
             if L > 0 else None for n, L in enumerate(lens)]
    full = [x for x in parts if x is not None]
    out = {key: torch.cat([x[key][0] for x in full]) for key in ('q', 'k', 'v', 'dout', 'want', 'abs_want', 'want_dq', 'abs_dq',
                                                                 'want_dk', 'abs_dk', 'want_dv')}
    out['cu'] = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=device)
    out['scale'], out['parts'] = full[0]['scale'], parts
    return out


# ---- criteria -------------------------------------------------------------------------------------------------------------

def candidates(want, dtype, rel):
    """The 16-bit roundings of want (1 - rel) and want (1 + rel), as fp64: equal where the rounding is unambiguous."""
    return (want * (1 - rel)).to(dtype).double(), (want * (1 + rel)).to(dtype).double()


def ambiguous_rows(want, dtype, rel=FP32_MEAN):
    """bool (...): rows (all but the last axis) with an entry whose 16-bit rounding depends on an error of `rel`."""
    lo, hi = candidates(want, dtype, rel)
    return (lo != hi).any(dim=-1)


def mean_failures(got, want, dtype, name, zero_bound=P.DUST, rel=FP32_MEAN):
    """Criterion of a result known as an exact fp64 number of which a correct kernel holds an fp32 value within `rel`: got,
    rounded to `dtype`, == the 16-bit rounding of want where every number of want (1 +- rel) rounds alike, one of the two
    roundings where not; |got| <= zero_bound (a number or a tensor) where want == 0."""
    got = got.double()
    want = want.to(got.device)
    bound = zero_bound.to(got.device) if torch.is_tensor(zero_bound) else zero_bound
    lo, hi = candidates(want, dtype, rel)
    g = got.to(dtype).double()
    bad = []
    wrong = (want != 0) & (g != lo) & (g != hi)
    if wrong.any():
        at = wrong.nonzero()[0].tolist()
        bad.append(f'{name}: {int(wrong.sum())} non-zero entries ({int(wrong.any(dim=-1).sum())} rows) differ from the rounded closed '
                   f'form, first at {at}: {got[tuple(at)].item()!r} for {want[tuple(at)].item()!r}')
    loud = (want == 0) & ~(got.abs() <= bound)
    if loud.any():
        at = loud.nonzero()[0].tolist()
        bad.append(f'{name}: {int(loud.sum())} entries that should vanish exceed their bound, first at {at}: {got[tuple(at)].item()!r}')
    return bad


def zero_out(prob):
    """Bound on an output entry whose exact value is 0: the other keys' weights (DUST) and, where non-zero terms cancel, what
    an fp32 summation of them may leave (prefill_needles.FP32_SUM of their magnitudes)."""
    return P.DUST + P.FP32_SUM * prob['abs_want']


def lse_failures(lse, want, name='LSE'):
    return P.lse_failures(lse, want, name)


def lse_resolution(prob):
    """Largest ratio, over the rows, of the LSE tolerance to ln(1 + 1 / n): <= 1/2 tells n from n +- 1."""
    tol = P.LSE_TOL['atol'] + P.LSE_TOL['rtol'] * prob['lse'].abs()
    return float((tol / torch.log1p(1.0 / prob['n'].double())).max())


def probs_failures(p, prob, dtype, name, p_error):
    """Criterion of a probability matrix rebuilt from an LSE in fp32 with relative error <= p_error and rounded to `dtype`:
    bit for bit the rounding of 1 / n on the tied keys where unambiguous (a power of two always is), exactly 0 where masked,
    <= 2e-21 on the other keys."""
    want = prob['p'].to(p.device)
    got = p.double()
    bad = mean_failures(got, want, dtype, name, zero_bound=2e-21, rel=p_error)
    if prob['causal']:
        sq, sk = got.shape[-2:]
        upper = torch.triu(torch.ones(sq, sk, dtype=torch.bool, device=p.device), 1)
        if not (got[..., upper] == 0).all():
            bad.append(f'{name}: non-zero entries above the diagonal')
    return bad


def grad_bounds(prob, dtype, p_error):
    """Bounds on |dQ - closed form| and |dK - closed form| of csrc/flash_bwd.hip on a tie problem, from its roundings: P is
    rebuilt from the LSE in fp32 (relative error e <= p_error), dS = P (dP - D) is rounded to 16 bit once (u) for the products
    with K and Q, whose fp32 sums add 2^-22 of the magnitudes (FP32_SUM), and the result is rounded once more:
        |err| <= (e + u (1 + e) + FP32_SUM) sum |dS| |k| scale  +  u |closed form|  +  GRAD_DUST.
    One wrong term moves an entry by |dS| scale = scale / (n 2^m) or more -- compare in the host test."""
    if 'parts' in prob:                  # a ragged batch: sequence by sequence
        each = [grad_bounds(x, dtype, p_error) for x in prob['parts'] if x is not None]
        return torch.cat([x[0][0] for x in each]), torch.cat([x[1][0] for x in each])
    u = P.ROUNDING[dtype]
    f = p_error + u * (1 + p_error) + P.FP32_SUM
    # D = dO . O is taken from the 16-bit O the kernel is handed; on 1 / n rows that is not the exact mean: dS moves by P |D16 - D|
    dd = ((prob['dout'].double() * (prob['want'].to(dtype).double() - prob['want'])).sum(-1).abs()).permute(0, 2, 1)     # (b, h, sq)
    pd = prob['p'] * dd[..., None]
    extra_q = prob['scale'] * torch.einsum('bhts,bshd->bthd', pd, prob['k'].double().abs())
    extra_k = prob['scale'] * torch.einsum('bhts,bthd->bshd', pd, prob['q'].double().abs())
    return (f * prob['abs_dq'] + (1 + u) * extra_q + u * prob['want_dq'].abs() + P.GRAD_DUST,
            f * prob['abs_dk'] + (1 + u) * extra_k + u * prob['want_dk'].abs() + P.GRAD_DUST)


EXACT_GRAD_MAPS = (('full1', 'full2', 'full3'), ('full4', 'full5', 'full6+32'), ('full7', 'early5', 'early3'))


def exact_grad_slots(prob, dtype):
    """bool (b, h): the slots of a sparse-dout full-block problem in which csrc/flash_bwd.hip owes dQ and dK bit for bit: dS =
    2^-m (V[j, c] - O[c]), scale dS (wherever the kernel folds the scale), and the closed forms of dQ and dK are all representable
    in `dtype`.  Then the one rounding of dS returns it exactly (the rebuilt P's error, < 5e-5, is far inside half an ulp of an
    8-bit number), the fp32 sums over keys and query tiles are sums of representable numbers with a representable result, and the
    stored value is that result."""
    def fits(x, dims):
        return (x.to(dtype).double() == x).flatten(dims).all(-1)
    ok = fits(prob['ds'], 2) & fits(prob['scale'] * prob['ds'], 2)                               # (b, h)
    return ok & fits(prob['want_dq'].permute(0, 2, 1, 3), 2) & fits(prob['want_dk'].permute(0, 2, 1, 3), 2)


def row_p_error(prob):
    """p_error row by row, (b, g, sq, 1): each row's own integer score q . k and closed-form LSE (as handed to the kernel, fp32)."""
    sc = torch.tensor(prob['scale'], dtype=torch.float32)
    log2e = torch.tensor(P.LOG2E, dtype=torch.float32)
    c2 = float((sc * log2e).double())
    lse = prob['lse'].float()
    ideal = -prob['n'].double().log2()
    x = prob['dot'].double() * c2
    worst = torch.maximum((x - (lse * log2e.to(lse.device)).double() - ideal).abs(), (x - lse.double() * P.LOG2E - ideal).abs())
    return ((2.0 ** worst - 1.0).abs() + 2.0 ** -21)[..., None]


@functools.lru_cache(maxsize=None)
def p_error(width):
    """prefill_needles.needle_p_error over the scores and LSEs a tie problem of this width has: scale reps (nbits - m) + ln n for
    m = 0 ... nbits and n = 1 ... 130, 2^8 ... 2^11 and a few long rows.  Bound on the relative error of a P rebuilt in fp32 as
    exp2(s c2 - lse log2e), c2 = fl(scale log2e)."""
    nbits = min(width, 16)
    worst = 0.0
    sc = torch.tensor(scale(width), dtype=torch.float32)
    log2e = torch.tensor(P.LOG2E, dtype=torch.float32)
    c2 = (sc * log2e).double()
    for m in range(nbits + 1):
        dot = reps(width) * (nbits - m)
        for n in (*range(1, 131), 256, 257, 333, 385, 512, 641, 1000, 1024, 2047, 2048):
            lse = torch.tensor(scale(width) * dot + math.log(n), dtype=torch.float32)
            ideal = -math.log2(n)
            worst = max(worst, abs(float(dot * c2 - (lse * log2e).double()) - ideal), abs(float(dot * c2 - lse.double() * P.LOG2E) - ideal))
    return abs(2.0 ** worst - 1.0) + 2.0 ** -21


# ---- the cases (shared by the GPU test and the host proof) -----------------------------------------------------------------

FLASH_FWD_CASES = [dict(d=d, seqlens=[s for s in (129, 257, 385, 641) if s - 1 + 32 <= max_length(d)]) for d in (8, 36, 64, 128)]
FLASH_BWD_CASES = [dict(d=d, seqlens=[129, 257, 641]) for d in (64, 128)]
FLASH_RAGGED = P.FLASH_RAGGED
FLASH_CROSS = [dict(P.FLASH_CROSS, sk=256), dict(P.FLASH_CROSS, sk=333)]
PROBS_SK = P.PROBS_SK


def fixed_problems(case, maps, dtype, device='cpu', cols=None):
    """(tag, problem) of every fixed-length causal call of a case: per S the maps three at a time (prefill_needles.bh_of)."""
    for s in case['seqlens']:
        b, h = P.bh_of(s)
        for rot in P.rotations(maps, 3):
            yield (f"d={case['d']} S={s} maps from {rot}",
                   attn_problem(P.slot_maps(maps, 3, rot), b, h, s, s, case['d'], dtype, device, cols=cols))


def cross_problems(c, dtype, device='cpu', cols=None, maps=CROSS_MAPS):
    for rot in P.rotations(maps, 3):
        yield (f"cross sk={c['sk']} maps from {rot}",
               attn_problem(P.slot_maps(maps, 3, rot), c['b'], c['h'], c['sq'], c['sk'], c['d'], dtype, device, causal=False, cols=cols))


def ragged_problems(dtype, device='cpu', cols=None, maps=FWD_MAPS):
    c = FLASH_RAGGED
    for rot in P.rotations(maps, c['h']):
        yield f'ragged maps from {rot}', ragged_problem(c['lens'], c['h'], c['d'], maps, rot, dtype, device, cols=cols)


# ---- sense problems ---------------------------------------------------------------------------------------------------------

SENSE_KW = (0.0, 0.5, 1.0, 2.0)


def sense_problem(s, k, dk, dout, b=2, device='cpu', maps=BWD_MAPS, form='dense', weighted=False, cols=None, pad=False, rot=0,
                  sparse=False):
    """One sense-mix call, inputs fp32, as prefill_needles.sense_problem: qk (b, s, 2, k, dkp), content (b, s, k, w) or table +
    rows ('gather'), key_weight (b, k, s) in {0, 1/2, 1, 2} or None, dout (b, s, w) in {1, 2}.  Sense l of sample n takes
    maps[(l + n + rot) % len(maps)] -- another order m, another block and (the '+32' maps) another code offset than its
    neighbours, so a sense's result landing in another sense's sum changes bits.  p (b, k, s, s), lse, n, dot as attn_problem.
    Content values are POSITIVE integers <= prefill_needles.value_cap(k) (the 1e-21 weights of the other keys then only add, and
    an fp32 sum of positive terms absorbs them), so with full-block maps
        want = sum_l w 2^-m_l sum C[j, l, :]      want_dc[s, l, :] = sum_t 2^-m_l dout[t, :]
    are multiples of 2^-8 below 2^11: exact fp32 numbers in any order of summation, and the expected 16-bit result is their one
    rounding (the host test asserts both)."""
    dkp = -(-dk // 8) * 8 if pad else dk
    w = cols or dout
    t = torch.arange(s, device=device)
    qk = torch.empty(b, s, 2, k, dkp, device=device)
    p = torch.empty(b, k, s, s, dtype=torch.float64, device=device)
    lse = torch.empty(b, k, s, dtype=torch.float64, device=device)
    cnt = torch.empty(b, k, s, dtype=torch.int64, device=device)
    dot = torch.empty(b, k, s, dtype=torch.int64, device=device)
    cache = {}
    for n in range(b):
        for l in range(k):
            name = maps[(l + n + rot) % len(maps)]
            if name not in cache:
                pos, m, base, c = rows_of(name, s, s, dk, True, device)
                cache[name] = (tie_query(pos, m, dk, dkp), code(t + parse(name)[2], dk, dkp), dense_p(base, c, s),
                               scale(dk) * reps(dk) * (min(dk, 16) - m).double() + c.double().log(), c, reps(dk) * (min(dk, 16) - m))
            qk[n, :, 0, l], qk[n, :, 1, l], p[n, l], lse[n, l], cnt[n, l], dot[n, l] = cache[name]
    ids = torch.arange(b, device=device)[:, None] * POS_STRIDE + t[None, :]
    senses = torch.arange(k, device=device)
    cap = P.value_cap(k)
    prob = dict(qk=qk, p=p, lse=lse, n=cnt, dot=dot, dk=dk, scale=scale(dk), causal=True, key_weight=None)
    if form == 'gather':
        prob['rows'] = N.table_rows_of(ids, P.VOCAB)
        prob['table'] = (N.sense_value(torch.arange(P.VOCAB, device=device)[:, None], senses[None, :], w) - 1) % cap + 1
        content = prob['table'][prob['rows'].long()]
    else:
        content = (N.sense_value(ids[:, :, None], senses[None, None, :], w) - 1) % cap + 1
    prob['content'] = content
    pw = p
    if weighted:
        kw = torch.tensor(SENSE_KW, device=device)[_hash(ids[:, None, :] * 64 + senses[None, :, None] + 4243) % 4]        # (b, k, s)
        prob['key_weight'] = kw
        pw = p * kw[:, :, None, :].double()
    prob['want'] = torch.einsum('blts,bslw->btw', pw, content.double())
    prob['dout'] = P.sparse_grad(ids, w, 1, 1) if sparse else P.grad_rows(ids, w)      # sparse: a single 1 per row, dP <= value_cap
    prob['want_dc'] = torch.einsum('blts,btw->bslw', p, prob['dout'].double())
    return prob


def dqk_forms(prob, dtype):
    """fp64 closed forms of bp.sense_dqk on a sense problem and the bounds on what csrc/sense_mix_bwd.hip may leave, after the
    model of prefill_needles.pair_dqk_bounds (sense_dq_kernel lines 380-386, 416-420, 463-466; sense_dk_kernel) -> (want_dqk
    like qk, bound_q (b, t, k, 1), bound_k (b, s, k, 1)).  E = the rebuilt P's relative error, u = one 16-bit rounding, spread /
    top = the range / largest magnitude of the dP a row can see.
      dq: g_j = P_j (dP_j - r) is rounded to 16 bit for A1 = sum g_j k_j (sum |g_j| <= (1 + E) spread) but not inside D - r = sum g_j
          + r (sum P - 1), which multiplies A2 = sum P_j k_j (|A2| <= 1 + E):  |dq / scale - closed form| <= (u (1 + E) + E) spread + E
          (spread + top) =: err, fp32 products 2^-20 of the same, the stored number one more rounding.  On a 1 / n row A2's operand,
          the 16-bit P (lines 419, 433), is rounded too: + u (1 + E) |D - r| <= u (1 + E) ((1 + E) spread + E top).
      dk: dS_tj = P_tj (dP_tj - D_t) with D = (1 + e) sum P dP, rounded to 16 bit: off by P (E (|dP - D| + |D|) + 2^-20 top) + u
          |dS|; the key's sum over its rows (|q| <= 1) in fp32 (FP32_SUM), stored with one more rounding.
    One wrong term moves an entry by scale |dS| = scale 2^-m |dP - D|."""
    u, e = P.ROUNDING[dtype], float(row_p_error(prob).max())
    q, key = prob['qk'][:, :, 0].double(), prob['qk'][:, :, 1].double()
    p, sc = prob['p'], prob['scale']
    dp = torch.einsum('btw,bslw->blts', prob['dout'].double(), prob['content'].double())
    dd = (p * dp).sum(-1)
    ds = p * (dp - dd[..., None])
    want = torch.stack([sc * torch.einsum('blts,bsld->btld', ds, key), sc * torch.einsum('blts,btld->bsld', ds, q)], dim=2)
    n = dp.shape[-1]
    seen = torch.tril(torch.ones(n, n, dtype=torch.bool, device=dp.device))
    inf = torch.tensor(float('inf'), dtype=torch.float64, device=dp.device)
    hi, lo = torch.where(seen, dp, -inf).max(-1).values, torch.where(seen, dp, inf).min(-1).values
    spread, top = hi - lo, torch.maximum(hi.abs(), lo.abs())
    err = (u * (1 + e) + e) * spread + e * (spread + top) + 2.0 ** -20 * (spread + top)
    odd = (prob['n'] & (prob['n'] - 1)) != 0                     # P = 1 / n is not a 16-bit number: A2's operand is pack2(P) (line 419, 433)
    err = err + odd * u * (1 + e) * ((1 + e) * spread + e * top)
    bound_q = (sc * err * (1 + u)).permute(0, 2, 1)[..., None] + u * want[:, :, 0].abs() + P.GRAD_DUST
    per = p * ((e * ((dp - dd[..., None]).abs() + dd.abs()[..., None]) + 2.0 ** -20 * top[..., None]) * (1 + u)) + (u + P.FP32_SUM) * ds.abs()
    bound_k = (sc * per.sum(2) * (1 + u)).permute(0, 2, 1)[..., None] + u * want[:, :, 1].abs() + P.GRAD_DUST
    return want, bound_q, bound_k, ds


def rebuild_dqk_bounds(prob, dtype):
    """Bounds on |dqk - closed form| of the alpha-rebuilding backward (bp_hip._sense_mix_backward_rebuild) on a full-block problem
    with a single 1 per dO row -> (want_dqk, bound_q (b, t, k, 1), bound_k (b, s, k, 1)).  Its steps: sense_alpha from the
    forward's LSE, 16 bit: 2^-m exactly (lse_error + row_p_error < half an ulp, the host test asserts it); dalpha = dout C^T
    through the BLAS, 16 bit: a content value, exact; csrc/softmax_bwd.hip:40-42 D = sum alpha dalpha by fma, exact (multiples of
    2^-7 below 2^4); :57-60 dS = (scale * alpha) * (dalpha - D) in fp32 -- fl(scale) 2^-24, the product 2^-24 -- rounded to 16 bit
    ONCE (u); dq = dS k and dk = dS^T q through the BLAS, fp32 sums (FP32_SUM) stored with one more rounding:
        |err| <= (u (1 + 2^-22) + 2^-22 + FP32_SUM) scale sum |dS| |k|  +  u |closed form|  +  GRAD_DUST.
    One wrong term moves an entry by scale |dS|; the D of a neighbouring row moves every term of the row."""
    u = P.ROUNDING[dtype]
    want, _, _, ds = dqk_forms(prob, dtype)
    f = u * (1 + 2.0 ** -22) + 2.0 ** -22 + P.FP32_SUM
    q, key = prob['qk'][:, :, 0].double().abs(), prob['qk'][:, :, 1].double().abs()
    abs_q = prob['scale'] * torch.einsum('blts,bsld->btld', ds.abs(), key)
    abs_k = prob['scale'] * torch.einsum('blts,btld->bsld', ds.abs(), q)
    return want, f * abs_q + u * want[:, :, 0].abs() + P.GRAD_DUST, f * abs_k + u * want[:, :, 1].abs() + P.GRAD_DUST


def sense_varlen_problem(lens, k, dk, dout, device='cpu', maps=BWD_MAPS, cols=None):
    """A packed batch of sense problems: qk (total, 2, k, dk), content (total, k, w), want (total, w), cu; 'parts' per sequence
    (their lse stays per part); sequence n takes the maps rotated by n."""
    parts = [sense_problem(L, k, dk, dout, 1, device, maps, cols=cols, rot=n) for n, L in enumerate(lens)]
    out = {key: torch.cat([x[key][0] for x in parts]) for key in ('qk', 'content', 'want')}
    out['cu'] = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=device)
    out['scale'], out['parts'] = parts[0]['scale'], parts
    return out


def lse_error(prob):
    """Relative error a P rebuilt from a kernel's OWN fp32 LSE may carry on top of row_p_error: lse = (fl(m c2) + log2 l) ln 2
    (csrc/flash_fwd_dma.hip:369, 487) is three fp32 roundings of a number of the LSE's size in log2 units, the consumer's
    fl(lse log2e) a fourth: four half-ulps in the exponent."""
    top = float(prob['lse'].abs().max()) * P.LOG2E
    return 4 * 2.0 ** (math.floor(math.log2(max(top, 1.0))) - 24) * P.LN2


def mix_bound(prob, dtype, want, own_lse=True):
    """Bound on |got - want| of a sum of P-weighted POSITIVE terms (the mix's out, dC, dV) whose P = 1 / n is rebuilt in fp32 from
    an LSE (relative error e: row_p_error, + lse_error where the LSE is the kernel's own) and rounded to 16 bit (u) before the
    matrix unit (csrc/mix_ring.h:154, 188-189; sense_mix_bwd.hip:135-136; flash_bwd.hip sub_block): every term is off by at most
    e + u (1 + e) of itself, the fp32 sum by FP32_SUM, the stored result by u:  (e + u (1 + e) + FP32_SUM + u (1 + ...)) want.
    One key of n lost or doubled moves a sense's term by 1 / n of it: seen where n < 1 / (2 u + e), i.e. on every own-block row of
    fp16, on those with r < 120 in bf16, and on flat rows up to that length; the full-block senses next to them stay bit for bit
    where the result separates them (dC, dV), and the LSE criterion counts the keys of every row."""
    u = P.ROUNDING[dtype]
    e = float(row_p_error(prob).max()) + (lse_error(prob) if own_lse else 0.0)
    return ((e + u * (1 + e) + P.FP32_SUM) * (1 + u) + u) * want.abs() + P.DUST


def full_senses(prob):
    """bool (b, k): the senses of a sense problem whose map is a full-block one (every tie count a power of two)."""
    return ((prob['n'] & (prob['n'] - 1)) == 0).all(dim=-1)


# (S, k, d_k, d_out): the narrow ring, the zero-padded d_k = 10, the wide ring, the staged wide kernel (S % 32 != 0)
MIX_SHAPES = [(257, 16, 48, 256), (320, 64, 10, 640), (352, 4, 160, 640), (333, 4, 160, 640)]
MIX_STAGED = P.MIX_STAGED
MIX_GATHER = [(257, 16, 48, 256), (352, 4, 160, 640)]
MIX_WEIGHTED = MIX_SHAPES                          # key_weight on every route: narrow ring, padded d_k = 10, wide ring, staged wide
MIX_VARLEN = dict(lens=[70, 1, 130, 257, 5], k=16, dk=48, dout=256)
MIX_DC = [(129, 16, 48, 256), (257, 16, 48, 256), (641, 4, 24, 104), (130, 64, 10, 640)]
MIX_WIDE_AUTOGRAD = (352, 4, 160, 640)
MIX_DQK = [(200, 4, 24, 104), (257, 16, 48, 256), (641, 16, 16, 64)]            # prefill_needles.MIX_DQK: slabs that start at 128 ... 640
ALPHA_CASES = [(200, 4, 24), (320, 16, 48), (257, 64, 10), (96, 4, 160)]
MIX_MIXED = [(257, 16, 48, 256), (352, 4, 160, 640)]     # own-block and flat senses next to full-block ones: the narrow and the wide ring


# ---- decode: one query per (sample, head) against a cache of L keys plus the appended one ---------------------------------------

DECODE_MAPS = ('full4', 'own6', 'early6+32', 'full7', 'early4', 'head0', 'flat', 'head4', 'full6+32', 'early7', 'early6+32')
DECODE_LENGTHS = (63, 64, 65, 1000, 2047, 4096)
DECODE_CASES = [c for c in N.TRUNK_CASES if c['d'] in (64, 128)]


def decode_maps(L):
    """DECODE_MAPS with the 1 / n rows kept only where n is a power of two (flat: L + 1 = 64, 2048; own6: L % 64 + 1): the
    split kernel keeps P in fp32, so then, as on every full block, 1 / l, every split's weight and every product of the combine
    (csrc/decode_core.h:259-261, 278) are exact and the result is ONE rounding of an exact number; any other n leaves an fp32
    error per split: those rows have a test and a bound of their own (DECODE_FLAT_MAPS, decode_bound).  Flat rows stop at 2048 keys (the LSE condition)."""
    pow2 = lambda n: n & (n - 1) == 0
    return tuple('early4' if m == 'flat' and not (pow2(L + 1) and L + 1 <= 2048) else 'full7' if m == 'own6' and not pow2(L % 64 + 1)
                 else m for m in DECODE_MAPS)


def decode_problem(case, L, dtype, device='cpu', cols=None, maps=None):
    """flash_decode at cache length L: q (b, h, d), keys / vals (b, L + 1, h, .) fp32 (row L is the appended key), p (b, h, L + 1)
    fp64, n, lse (b, h), want and abs_want (b, h, w).  Row r = (sample, head) takes decode_maps(L)[r % 11] with salt r: blocks
    inside one split, across split borders (every 2^m > chunk block is), and, for the last-block maps, next to or around the
    appended key."""
    b, h, d = case['batch'], case['heads'], case['d']
    w = cols or d
    maps = maps or decode_maps(L)
    r = torch.arange(b * h, device=device)
    pos_all = torch.arange(L + 1, device=device)
    q = torch.empty(b * h, d, device=device)
    keys = torch.empty(b * h, L + 1, d, device=device)
    base, n, lse = (torch.empty(b * h, dtype=dt, device=device) for dt in (torch.int64, torch.int64, torch.float64))
    coded = torch.zeros(b * h, dtype=torch.bool, device=device)
    for idx, name in enumerate(maps):
        rows = r[r % len(maps) == idx]
        if rows.numel() == 0:
            continue
        qp, m, bs, cnt = rows_at(name, torch.full_like(rows, L), L + 1, d, True, salt=rows)
        q[rows] = tie_query(qp, m, d)
        keys[rows] = code(pos_all + parse(name)[2], d)
        base[rows], n[rows] = bs, cnt
        lse[rows] = scale(d) * reps(d) * (min(d, 16) - m).double() + cnt.double().log()
        coded[rows] = parse(name)[0] in ('own', 'flat')
    ids = r[:, None] * POS_STRIDE + pos_all[None, :]
    vals = P.pair_values(ids, w, TIE_MAGS[dtype])
    c = min(8, w)
    vals[..., :c] = torch.where(coded[:, None, None], code(pos_all, 8)[None, :, :c], vals[..., :c])
    p = dense_p(base, n, L + 1)
    live = (p > 0).double()
    want = torch.einsum('rs,rsw->rw', live, vals.double()) / n.double()[:, None]
    abs_want = torch.einsum('rs,rsw->rw', live, vals.double().abs()) / n.double()[:, None]
    shape = lambda x: x.view(b, h, *x.shape[1:])
    return dict(q=shape(q), keys=shape(keys).transpose(1, 2), vals=shape(vals).transpose(1, 2), p=shape(p), n=shape(n), lse=shape(lse),
                want=shape(want), abs_want=shape(abs_want), scale=scale(d), maps=maps)


SENSE_DECODE_CASES = [c for c in N.SENSE_CASES if (c['dkp'], c['k'], c['dout']) in ((48, 16, 768), (160, 4, 640))]


def sense_decode_problem(case, L, form, weighted=False, device='cpu', cols=None):
    """sense_decode at cache length L: q (b, k, dk), keys (b, L + 1, k, dk) (row L is the appended key), table (rows, k, w) of
    POSITIVE integers <= value_cap(k), rows (b, L + 1) int32 ('table': even rows of a 1024-row table; 'cache': b * max_seqlen +
    j), key_weight (b, k, L + 1) in {0, 1/2, 1, 2} or None, p (b, k, L + 1), n, lse (b, k), vals (b, L + 1, k, w) = the weighted
    content rows, want (b, w).  Row r = (sample, sense) takes decode_maps(L)[r % 11] with salt r, as decode_problem: every tie
    count is a power of two, so every split weight is one and want is ONE rounding of an exact fp32 sum."""
    b, k, dk, ms = case['batch'], case['k'], case['dk'], case['max_seqlen']
    w = cols or case['dout']
    maps = decode_maps(L)
    r = torch.arange(b * k, device=device)
    pos_all = torch.arange(L + 1, device=device)
    q = torch.empty(b * k, dk, device=device)
    keys = torch.empty(b * k, L + 1, dk, device=device)
    base, n, lse = (torch.empty(b * k, dtype=dt, device=device) for dt in (torch.int64, torch.int64, torch.float64))
    for idx, name in enumerate(maps):
        rows = r[r % len(maps) == idx]
        if rows.numel() == 0:
            continue
        qp, m, bs, cnt = rows_at(name, torch.full_like(rows, L), L + 1, dk, True, salt=rows)
        q[rows] = tie_query(qp, m, dk)
        keys[rows] = code(pos_all + parse(name)[2], dk)
        base[rows], n[rows] = bs, cnt
        lse[rows] = scale(dk) * reps(dk) * (min(dk, 16) - m).double() + cnt.double().log()
    senses = torch.arange(k, device=device)
    cap = P.value_cap(k)
    samples = torch.arange(b, device=device)[:, None]
    if form == 'cache':
        idx = (samples * ms + pos_all[None, :]).int()
        nrows = b * ms
    else:
        idx = N.table_rows_of(samples * POS_STRIDE + pos_all[None, :], P.VOCAB)
        nrows = P.VOCAB
    table = (N.sense_value(torch.arange(nrows, device=device)[:, None], senses[None, :], w) - 1) % cap + 1
    vals = table[idx.long()]                                                            # (b, L + 1, k, w)
    p = dense_p(base, n, L + 1).view(b, k, L + 1)
    kw = None
    if weighted:
        kw = torch.tensor(SENSE_KW, device=device)[_hash((samples[:, :, None] * 64 + senses[None, :, None]) * POS_STRIDE + pos_all + 4243) % 4]
        vals = vals * kw.permute(0, 2, 1)[..., None]
    want = torch.einsum('bls,bslw->bw', p, vals.double())
    return dict(q=q.view(b, k, dk), keys=keys.view(b, k, L + 1, dk).transpose(1, 2), table=table, rows=idx, key_weight=kw, vals=vals,
                p=p, n=n.view(b, k), lse=lse.view(b, k), want=want, scale=scale(dk), maps=maps)


DECODE_FLAT_MAPS = ('flat', 'own6', 'full7')
DECODE_FLAT_LENGTHS = (64, 65, 1000, 2047)


def decode_bound(prob, dtype, nsplit):
    """Bound on |out - want| of the split decode where a tie count is NO power of two: P stays fp32 and every tied key has p = 1, so
    a split's l and acc are exact integers, but inv = 1 / lsum, the weights exp2(m_s - M) * inv and the nsplit products and adds
    of the combine (csrc/decode_core.h:259-261, 274-279, 287-292) each round once: (nsplit + 3) 2^-24 of sum |terms| = of the
    mean of |v|, plus the rounding of the stored result.  One key of n lost moves an entry by |v| / n."""
    return (nsplit + 3) * 2.0 ** -24 * prob['abs_want'] + P.ROUNDING[dtype] * prob['want'].abs() + P.DUST
