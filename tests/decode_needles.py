"""Inputs for which single-query decode attention is exact in fp32 ("needles"), for tests/test_gpu_decode_edges.py and
its CPU pre-check in tests/test_kv_cache_host.py (the way tests/philox_ref.py serves the dropout tests).

Key j is a +-1 code of its position: the 16 bits of j, repeated reps = width // 16 times (a width under 16: its low
`width` bits once, reps = 1, so such a width takes lengths under 2^width), the remaining columns +1, the columns of a
zero-padded width (ContextSelfAttn.project) 0.  The query of an output row is the code of its needle position j*, and
softmax_scale = 24 / reps.  Two different positions differ in at least one bit, so the needle's score exceeds every
other by at least 2 * reps * scale = 48: every other weight is below e^-48 = 1.5e-21, 4097 of them stay below 1e-17, and
the needle's probability is 1.0 in fp32.  Values are non-zero integers of magnitude 1 ... 8 (exact in fp16 and bf16), so
the fp32 answer of a row is exactly the value row of its needle, and the sum over up to 64 senses (positive values:
see sense_value) is an exact fp32 integer.  A dropped, duplicated or stale key then changes bits, at any length.

Everything is a fixed integer function of its indices (no generator state), so the CPU check and the GPU test build the
same numbers independently, on any device, for any subset of rows.  Nothing here needs a device or the built library.
"""
import torch

MAX_SEQLEN = 4104          # cache capacity of the long cases (the step at L = 4096 still fits)
SHORT_SEQLEN = 1008        # ... of the nsplit = 1 cases (512 output rows) that stop at L = 1000 to keep the CPU check short
POS_STRIDE = 8192          # > any length: (row, position) -> one integer id


def reps(width):
    return max(width // 16, 1)


def scale(width):
    return 24.0 / reps(width)


def max_length(width):
    """Longest cache length L (keys 0 ... L) whose positions have distinct codes."""
    return min(4096, 2 ** min(width, 16) - 1)


def code(pos, width, padded=None):
    """pos: integer tensor (...) -> float32 (..., padded or width) code of each position."""
    padded = padded or width
    nbits = min(width, 16)
    bits = (pos.long()[..., None] >> torch.arange(nbits, device=pos.device)) & 1
    sign = (2 * bits - 1).float()
    out = torch.zeros(*pos.shape, padded, device=pos.device)
    out[..., :width] = 1.0
    out[..., :nbits * reps(width)] = sign.repeat(*([1] * pos.dim()), reps(width))
    return out


def needle_score(width):
    """softmax_scale * q . k of a needle with itself (the row's natural-log LSE, all other weights being < 1e-17)."""
    return scale(width) * width


def _hash(ids):
    x = (ids.long() * 2654435761 + 40503) & 0xffffffff
    x = ((x ^ (x >> 15)) * 2246822519) & 0xffffffff
    return x ^ (x >> 13)


def values(ids, width):
    """ids: integer tensor (...) -> float32 (..., width) of non-zero integers in [-8, 8], a hash of (id, column)."""
    h = _hash(ids.long()[..., None] * 4099 + torch.arange(width, device=ids.device))
    return (((h & 7) + 1) * (1 - 2 * ((h >> 3) & 1))).float()


def table_rows_of(ids, vocab):
    """ids: integer tensor -> an EVEN row of a `vocab`-row table (the odd rows are never named: the tests poison them)."""
    return (2 * (_hash(ids.long() + 977) % (vocab // 2))).int()


def lengths(nsplit, width, max_seqlen):
    """Cache lengths of a needle case: the tile borders, the long ones, (L + 1) % nsplit in {0, 1, nsplit - 1}, and the
    longest one whose last active split holds a single key (n = (nact - 1) * chunk + 1)."""
    top = min(max_length(width), max_seqlen - 8)
    ls = {L for L in (0, 1, 63, 64, 65, 1000, 4096) if L <= top}
    ls.add(top)
    for r in {0, 1 % nsplit, nsplit - 1}:
        ls.add(max(L for L in range(top + 1) if (L + 1) % nsplit == r))
    if nsplit > 1:
        ls.add(max(L for L in range(1, top + 1) if L % -(-(L + 1) // nsplit) == 0))
    return sorted(ls)


def needle_positions(L, nsplit):
    """Positions worth a needle at cache length L: 0, the appended key L, L - 1, every 64-key tile border +-1 inside the
    first and the last active split, and the first and last key of several splits (chunk = ceil((L + 1) / nsplit))."""
    n = L + 1
    chunk = -(-n // nsplit)
    nact = -(-n // chunk)
    want = {0, 1, L, L - 1, L - 2}
    for s in {0, nact - 1}:
        j0, j1 = s * chunk, min(n, (s + 1) * chunk)
        for t in range(j0, j1, 64):
            want |= {t - 1, t, t + 1, t + 62, t + 63}
        want |= {j1 - 2, j1 - 1, j1}
    for s in {0, 1, 2, nact // 2, nact - 2, nact - 1}:
        want |= {s * chunk - 1, s * chunk, s * chunk + 1, (s + 1) * chunk - 1}
    return sorted(j for j in want if 0 <= j <= L)


# ---- the cases (one list, shared by the GPU test and the CPU check) ------------------------------------------------------

# nsplit = min(ceil(512 / (batch * groups)), ceil(max_seqlen / 64), 64): 8 rows -> 64, 64 rows -> 8, 512 rows -> 1.
# One workgroup walking all 65 tiles of L = 4096 (nsplit = 1 at the full capacity) runs at d = 64 and 128, one head dim of
# each of the model's G buckets; the other head dims take nsplit = 1 up to L = 1000 (d = 8 stops at 255 anyway).
TRUNK_CASES = [dict(d=d, batch=b, heads=h, max_seqlen=ms, regime=name)
               for d in (8, 16, 64, 80, 128)
               for name, b, h, ms in (('split64', 2, 4, MAX_SEQLEN), ('split8', 8, 8, MAX_SEQLEN),
                                      ('split1', 64, 8, MAX_SEQLEN if d in (64, 128) else SHORT_SEQLEN))]

# (padded d_k, true d_k, senses, d_out, batch, max_seqlen): every G bucket of launch_decode (d_k / 8 = 1, 2, 3-4, 5-8,
# 9-16, 17-32, 33-64, 65-80), d_out = 8 (one chunk), 104 (13 chunks: a partial last combine block), 2048 (R = 1), the
# model shapes of tests/test_gpu_decode.py, and nsplit = 64 / between / 1 by batch x senses
SENSE_CASES = [dict(dkp=dkp, dk=dk, k=k, dout=dout, batch=b, max_seqlen=ms)
               for dkp, dk, k, dout, b, ms in (
                   (8, 8, 4, 8, 2, MAX_SEQLEN),              # nsplit 64
                   (16, 10, 20, 16, 3, MAX_SEQLEN),          # padded width, nsplit 9
                   (16, 16, 64, 640, 8, SHORT_SEQLEN),       # Mini k = 64, nsplit 1 up to L = 1000 (a 2.7 GB content cache at 4104)
                   (24, 24, 16, 104, 32, MAX_SEQLEN),        # nsplit 1 up to L = 4096: one workgroup, 65 tiles
                   (24, 24, 16, 384, 2, MAX_SEQLEN),         # Micro, nsplit 16
                   (48, 48, 16, 768, 1, MAX_SEQLEN),         # Small, nsplit 32
                   (128, 128, 2, 104, 3, MAX_SEQLEN),        # nsplit 64
                   (160, 160, 4, 640, 2, MAX_SEQLEN),        # Mini k = 4, nsplit 64
                   (264, 264, 1, 8, 5, MAX_SEQLEN),          # G = 64, NQ = 1
                   (400, 400, 1, 2048, 7, MAX_SEQLEN),       # G = 64, NQ = 1
                   (640, 640, 1, 640, 4, MAX_SEQLEN))]       # Mini k = 1, G = 64, NQ = 2
VOCAB = 1024


def trunk_value_ids(case, b, h, pos):
    """Integer id of the value row of (sample b, head h, position pos); b, h, pos broadcast."""
    return (b * case['heads'] + h) * POS_STRIDE + pos


def sense_row(case, form, b, pos):
    """Table row that position `pos` of sample b names ('table': a token-like even row, 'cache': b * max_seqlen + pos)."""
    if form == 'cache':
        return (b * case['max_seqlen'] + pos).int()
    return table_rows_of(b * POS_STRIDE + pos, VOCAB)


def sense_value(rows, sense, width):
    """table[rows, sense, :width]; rows, sense broadcast.  Positive, unlike the trunk's values: an output row is the SUM of
    its senses' needle rows, and every partial also carries its ~1e-20 of other keys; where the integers cancel to zero
    that dust would be the result (4e-21 instead of 0).  A sum >= the number of senses absorbs it in any order."""
    return values(rows.long() * 64 + sense, width).abs()


def assign(needles, rows):
    """Needle position of each of `rows` output rows per call: the list in chunks of `rows`, the last chunk cycled full."""
    calls = []
    for i in range(0, len(needles), rows):
        part = needles[i:i + rows]
        calls.append([part[r % len(part)] for r in range(rows)])
    return calls


# ---- references -----------------------------------------------------------------------------------------------------------

def attend_fp32(q, keys, vals, softmax_scale):
    """Plain fp32 softmax attention of rows q (r, d) over keys (n, d) with per-row values (r, n, w)."""
    p = torch.softmax(softmax_scale * (q.float() @ keys.float().T), dim=-1)
    return torch.einsum('rn,rnw->rw', p, vals.float())


def attend_splitwise(q, keys, vals, softmax_scale, chunk=65):
    """The same through an online softmax over 64-key tiles inside splits of `chunk` keys and a combine of the splits'
    partials (m, l, acc), as a split-KV kernel orders it (base-2 exponentials of log2(e)-scaled scores).  All splits at
    once: the key axis is padded to whole splits with -inf scores."""
    s = (softmax_scale * 1.4426950408889634) * (q.float() @ keys.float().T)
    r, n = s.shape
    ns = -(-n // chunk)
    s = torch.nn.functional.pad(s, (0, ns * chunk - n), value=float('-inf')).view(r, ns, chunk)
    v = torch.nn.functional.pad(vals.float(), (0, 0, 0, ns * chunk - n)).view(r, ns, chunk, -1)
    m = torch.full((r, ns), float('-inf'))
    l = torch.zeros(r, ns)
    acc = torch.zeros(r, ns, v.shape[-1])
    for t in range(0, chunk, 64):
        x = s[:, :, t:t + 64]
        m_new = torch.maximum(m, x.max(dim=-1).values)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(x - m_new[..., None])
        l = l * alpha + p.sum(dim=-1)
        acc = acc * alpha[..., None] + torch.einsum('rsn,rsnw->rsw', p, v[:, :, t:t + 64])
        m = m_new
    w = torch.exp2(m - m.max(dim=1, keepdim=True).values)
    lsum = (w * l).sum(dim=1, keepdim=True)
    return ((w / lsum)[..., None] * acc).sum(dim=1)
