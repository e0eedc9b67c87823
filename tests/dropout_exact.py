"""Exact inputs for in-kernel dropout: tests/test_gpu_dropout_exact.py and its CPU pre-check tests/test_dropout_exact_host.py
share the problems, the expected results and the criteria below (the style of tests/prefill_needles.py).

Five places draw the dropout mask, each with its own code: the flash forward (csrc/flash_fwd_dma.hip, DROP: lane = query), the
dQ kernel (csrc/flash_bwd.hip, flash_bwd_dq_tile<..., DROP>: lane = query), the dK/dV kernel (flash_bwd_dkdv_tile<..., DROP>:
lane = key, with a DPP quad exchange), the probability dump (csrc/attn_probs.hip: the sign bit) and the add + LayerNorm pair
(csrc/add_layer_norm.hip: one stream, index 0).  The mask is a pure function of (seed, offset, stream, row, column),
restated in tests/philox_ref.py, and the state is always given explicitly: STATES.

A. READ-OUTS.  Each attention use of the mask is read through a one-hot operand, so that one output entry depends on exactly
   one mask bit: (sample, head) slot n reads the window of d positions that starts at n d (ragged: head n of every sequence),
   and b h is chosen so that the windows cover the sequence.  q and k are small drawn values (every visible P stays far above
   the dtype's smallest normal number).
       forward  V[j] = e_(j - w0) inside the window:                  out[i, c] = Z[i, w0 + c] P[i, w0 + c]
       dV       dO[i] = e_(i - w0) over a window of rows:             dV[j, c]  = Z[w0 + c, j] P[w0 + c, j]
       dQ       K one-hot over a window of keys, dO = V = 1, O = 0:   dQ[i, c]  = scale d P[i, w0 + c] Z[i, w0 + c]
       dK       Q one-hot over a window of rows, dO = V = 1, O = 0:   dK[j, c]  = scale d P[w0 + c, j] Z[w0 + c, j]
   (O handed in as zeros makes D = dO . O exactly 0, so dS = P Z dP with dP = d.)  The forward read-out reads the forward's
   mask, dV and dK the dK/dV kernel's lane = key mask, dQ the dQ kernel's.  Criterion (readout_failures): exactly 0 where
   the restatement drops the pair or the causal mask hides it, non-zero everywhere else, and there within 4 u relative of the
   fp64 value, u one rounding of the dtype: the path has at most two 16-bit roundings (P or dS for the matrix unit, then the
   store; the host test runs an fp32 model with exactly those two and finds it within 2 u), the factor 2 on top covers the
   fp32 exponential and the rebuilt P.

B. PAIR PROBLEMS under p = 1/2 (prefill_needles.pair_attn_problem): Z is 0 or 2, everything stays a small integer or
   half-integer and the DROP bodies' arithmetic -- dneg[] and fmaf(dp, z, dneg) in the dK/dV tile, c_d = 0 in the dQ tile, the
   forward's row sum over the unrounded P -- has closed forms (prefill_needles._pair_closed_forms with the keep bits of every
   row's two needles) that the kernels must return bit for bit.  The LSE is unchanged: the mask acts after the row sum.

C. LAYERNORM.  dmask == rows_keep_mask on all rows at one width of every column class of the forward; at p = 1/2 with integer
   x0 and an fp32 residual the residual output is exactly 2 x0 where kept; backward: dx0 exactly 0 where dropped and, at
   p = 1/2 with an fp32 stream, (2 dx1).to(dtype) where kept.

Plain torch (numpy for the bit stream), any device, no generator state.
"""
import functools

import numpy as np
import torch

import philox_ref as R
import prefill_needles as P
from decode_needles import _hash

STATES = ((0x1234567, 99), (-0x1234567890ABCDEF, (7 << 32) + 12345))     # the second: offset >= 2^32
P_VALUES = (0.17, 0.5, 0.9, 1e-6)                 # 1e-6: the threshold clamps to 65535, only u16 = 65535 drops
ROUNDING = P.ROUNDING
READ_TOL = 4                                      # in units of one rounding, see the head of this file
MODEL_TOL = 2
SMALLEST_NORMAL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}
KINDS = ('fwd', 'dv', 'dq', 'dk')


def state_tensor(state, device):
    return torch.tensor(list(state), dtype=torch.int64, device=device)


# ---- the mask ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=64)
def _uniforms(state, streams, rows, cols):
    """(streams, rows, cols) uint16-valued uniforms of the streams 0 ... streams - 1, cached per (state, shape)."""
    return np.stack([R.uniforms16(state[0], state[1], n, rows, cols) for n in range(streams)])


def keep_mask(state, streams, rows, cols, p, mutant=None):
    """bool (streams, rows, cols), True = kept: philox_ref.attention_keep_mask with the (sample, head) pairs flattened.
    mutant: a wrong mask that the criteria must notice (the host test), None for the documented one."""
    thr = R.threshold(p)
    if mutant is None:
        u = _uniforms(state, streams, rows, cols)
    elif mutant == 'one key on':
        u = _uniforms(state, streams, rows, cols + 1)[:, :, 1:]
    elif mutant == 'one run of 4 on':
        u = _uniforms(state, streams, rows, cols + 4)[:, :, 4:]
    elif mutant == 'rows and columns swapped':
        u = _uniforms(state, streams, cols, rows).transpose(0, 2, 1)
    elif mutant == 'the neighbouring head':
        u = _uniforms(state, streams + 1, rows, cols)[1:]
    elif mutant == 'offset >> 32 ignored':
        u = _uniforms((state[0], state[1] & 0xFFFFFFFF), streams, rows, cols)
    else:
        raise KeyError(mutant)
    return torch.from_numpy(np.ascontiguousarray(u < thr))


MASK_MUTANTS = ('one key on', 'one run of 4 on', 'rows and columns swapped', 'the neighbouring head', 'offset >> 32 ignored')


# ---- A. read-outs -------------------------------------------------------------------------------------------------------------

# the smallest shapes that still have a full key tile, a partial one, a diagonal tile and a second 128-query tile
READ_CASES = [dict(d=16, sq=130, sk=130, causal=True), dict(d=40, sq=257, sk=257, causal=True),
              dict(d=64, sq=385, sk=385, causal=True), dict(d=80, sq=200, sk=200, causal=True),
              dict(d=128, sq=257, sk=257, causal=True),
              dict(d=P.FLASH_CROSS['d'], sq=P.FLASH_CROSS['sq'], sk=P.FLASH_CROSS['sk'], causal=False),   # dropout with sq != sk
              dict(d=P.FLASH_BWD_RAGGED['d'], lens=P.FLASH_BWD_RAGGED['lens'], causal=True)]


def case_id(c):
    return f"d{c['d']}-ragged" if 'lens' in c else f"d{c['d']}-{c['sq']}x{c['sk']}"


def case_layout(c):
    """(sequences [(lq, lk)], heads, ragged): b h = ceil(longest / d) slots, as samples x heads where that divides."""
    if 'lens' in c:
        return [(n, n) for n in c['lens']], -(-max(c['lens']) // c['d']), True
    slots = -(-max(c['sq'], c['sk']) // c['d'])
    b = 3 if slots % 3 == 0 else 2 if slots % 2 == 0 else 1
    return [(c['sq'], c['sk'])] * b, slots // b, False


def drawn(ids, width):
    """ids (...) -> float32 (..., width) of multiples of 1/8 in [-1, 1], a hash of (id, column)."""
    h = _hash(ids.long()[..., None] * 4099 + torch.arange(width, device=ids.device) + 977)
    return ((h >> 3) % 17 - 8).float() / 8


def _one_hot(pos, w0, d):
    """pos (n,), w0 (h,) -> float32 (n, h, d): e_(pos - w0) inside the window [w0, w0 + d), 0 elsewhere."""
    c = pos[:, None] - w0[None, :]
    return ((c[..., None] == torch.arange(d, device=pos.device)) & (c[..., None] >= 0)).float()


def readout_problem(c, kind, device='cpu'):
    """The operands of one read-out launch, fp32: q, dout (total_q, h, d), k, v (total_k, h, d), cu (int32, ragged only),
    scale, and per sequence n (None for an empty one) seqs[n] = dict(lq, lk, w0 (h,), p (h, lq, lk) fp64 probabilities,
    lse (h, lq) fp64).  The backward read-outs are handed O = 0 and the fp64 LSE rounded to fp32."""
    lay, h, ragged = case_layout(c)
    d, scale = c['d'], c['d'] ** -0.5
    parts, seqs = dict(q=[], k=[], v=[], dout=[]), []
    for n, (lq, lk) in enumerate(lay):
        if lq == 0:
            seqs.append(None)
            continue
        i, j = torch.arange(lq, device=device), torch.arange(lk, device=device)
        head = torch.arange(h, device=device)
        w0 = (head if ragged else n * h + head) * d
        ids_q = (n * h + head)[None, :] * P.POS_STRIDE + i[:, None]
        ids_k = (n * h + head)[None, :] * P.POS_STRIDE + j[:, None] + 500009
        q = _one_hot(i, w0, d) if kind == 'dk' else drawn(ids_q, d)
        k = _one_hot(j, w0, d) if kind == 'dq' else drawn(ids_k, d)
        v = _one_hot(j, w0, d) if kind == 'fwd' else torch.ones(lk, h, d, device=device)
        dout = _one_hot(i, w0, d) if kind == 'dv' else torch.ones(lq, h, d, device=device)
        s = scale * torch.einsum('ihd,jhd->hij', q.double(), k.double())
        if c['causal']:
            s = s.masked_fill(j[None, None, :] > i[None, :, None], float('-inf'))
        lse = torch.logsumexp(s, dim=-1)
        seqs.append(dict(lq=lq, lk=lk, w0=w0, p=torch.exp(s - lse[..., None]), lse=lse, s=s))
        for name, x in (('q', q), ('k', k), ('v', v), ('dout', dout)):
            parts[name].append(x)
    prob = {name: torch.cat(x) for name, x in parts.items()}
    prob.update(seqs=seqs, h=h, d=d, scale=scale, kind=kind, causal=c['causal'], ragged=ragged,
                max_q=max(a for a, _ in lay), max_k=max(b for _, b in lay))
    if ragged:
        prob['cu'] = torch.tensor([0] + torch.tensor([a for a, _ in lay]).cumsum(0).tolist(), dtype=torch.int32, device=device)
    return prob


def _window(m, w0, d, by_rows):
    """m (h, lq, lk) -> (lq, h, d) of m[hd, i, w0 + c] (by_rows False) or (lk, h, d) of m[hd, w0 + c, j] (True); 0 behind."""
    if by_rows:
        m = m.transpose(1, 2)
    h, n, width = m.shape
    m = torch.cat([m, torch.zeros(h, n, d, dtype=m.dtype, device=m.device)], dim=2)
    idx = (w0[:, None, None] + torch.arange(d, device=m.device)).clamp(max=width + d - 1).expand(h, n, d)
    return torch.gather(m, 2, idx).permute(1, 0, 2)


def readout_keep(prob, state, p, mutant=None):
    """Per sequence the keep mask (h, lq, lk) of its heads: stream sequence * h + head, rows and columns relative to the
    sequence."""
    streams = len(prob['seqs']) * prob['h']
    keep = keep_mask(state, streams, prob['max_q'], prob['max_k'], p, mutant).view(len(prob['seqs']), prob['h'], prob['max_q'], prob['max_k'])
    return [None if s is None else keep[n, :, :s['lq'], :s['lk']].to(s['p'].device) for n, s in enumerate(prob['seqs'])]


def readout_gather(prob, per_seq, factor=True):
    """per_seq[n] (h, lq, lk) -> what the read-out of `prob` shows of it: (total, h, d); factor: dQ and dK times scale d."""
    by_rows = prob['kind'] in ('dv', 'dk')
    out = torch.cat([_window(m, s['w0'], prob['d'], by_rows) for m, s in zip(per_seq, prob['seqs']) if s is not None])
    return out * (prob['scale'] * prob['d']) if factor and prob['kind'] in ('dq', 'dk') else out


def readout_want(prob, state, p, mutant=None):
    """fp64 expected result: forward (total_q, h, d), dV / dK (total_k, h, d), dQ (total_q, h, d)."""
    keeps = readout_keep(prob, state, p, mutant)
    return readout_gather(prob, [None if s is None else s['p'] * kp / (1.0 - p) for s, kp in zip(prob['seqs'], keeps)])


def readout_failures(got, want, dtype, name):
    """got (total, h, d) against the fp64 `want`: exactly 0 where want is, non-zero everywhere else and within READ_TOL
    roundings of it."""
    got, want = got.double(), want.to(got.device)
    bad = []
    ghost = (want == 0) & ~(got == 0)
    if ghost.any():
        at = ghost.nonzero()[0].tolist()
        bad.append(f'{name}: {int(ghost.sum())} entries of dropped or hidden pairs are not 0, first at {at}: {got[tuple(at)].item()!r}')
    lost = (want != 0) & ~(got != 0)
    if lost.any():
        bad.append(f'{name}: {int(lost.sum())} entries of kept pairs are 0 (or NaN), first at {lost.nonzero()[0].tolist()}')
    off = (want != 0) & (got != 0) & ~((got - want).abs() <= READ_TOL * ROUNDING[dtype] * want.abs())
    if off.any():
        at = off.nonzero()[0].tolist()
        bad.append(f'{name}: {int(off.sum())} entries beyond {READ_TOL} roundings, first at {at}: {got[tuple(at)].item()!r} for '
                   f'{want[tuple(at)].item()!r}')
    return bad


def readout_lse(prob, device, tail=float('nan')):
    """The (sequences, h, roundup(max_q, 16)) fp32 LSE the backward is handed: NaN behind the rows of every sequence."""
    lse = torch.full((len(prob['seqs']), prob['h'], -(-prob['max_q'] // 16) * 16), tail, device=device)
    for n, s in enumerate(prob['seqs']):
        if s is not None:
            lse[n, :, :s['lq']] = s['lse'].float()
    return lse


def probs_shapes():
    """(b, h, sq, sk, d, causal) of the probability dumps: the fixed-length read-out shapes."""
    for c in READ_CASES:
        if 'lens' not in c:
            lay, h, _ = case_layout(c)
            yield len(lay), h, c['sq'], c['sk'], c['d'], c['causal']


def probs_operands(b, h, sq, sk, d, device='cpu'):
    """q (b, sq, h, d), k (b, sk, h, d), fp32, drawn."""
    slot = torch.arange(b * h, device=device).view(b, 1, h)
    q = drawn(slot * P.POS_STRIDE + torch.arange(sq, device=device)[None, :, None], d)
    k = drawn(slot * P.POS_STRIDE + torch.arange(sk, device=device)[None, :, None] + 500009, d)
    return q, k


# ---- B. pair problems under p = 1/2 -------------------------------------------------------------------------------------------

PAIR_P = 0.5
PAIR_STATE = {'fixed': STATES[0], 'chain': STATES[0], 'cross': STATES[1], 'ragged': STATES[1]}
PAIR_MAGS = dict(P.PAIR_MAGS)          # per-dtype magnitudes of the values and of dO, as without dropout
# (map, d, S) of the fixed-length cases whose closed form bf16 cannot hold with the map in ITS slot of the rotation (the mask
# is a function of the slot): the host test asserts that this is exactly the unrepresentable set.  fp16: none.
PAIR_BF16_LEFT_OUT = frozenset([('back128', 8, 129), ('tile0', 16, 641)])      # both: a dK sum that needs more than 8 bits


def _needle_keep(keep, js):
    """keep (b, h, sq, sk) bool, js (b, h, sq) -> the keep bit of every row's needle (b, h, sq)."""
    return torch.gather(keep.to(js.device), 3, js[..., None])[..., 0]


def with_dropout(prob, keep):
    """A pair problem (prefill_needles.pair_attn_problem) with its closed forms under the mask `keep` (b, h, sq, sk) at
    p = 1/2; adds k1, k2 (b, h, sq).  The LSE stays."""
    k1, k2 = _needle_keep(keep, prob['js']), _needle_keep(keep, prob['js2'])
    out = dict(prob, k1=k1, k2=k2)
    out.update(P._pair_closed_forms(prob['q'], prob['k'], prob['v'], prob['dout'], prob['js'], prob['js2'], prob['scale'],
                                    prob['k'].shape[1], keep=(k1, k2)))
    return out


def pair_problem(maps, b, h, sq, sk, d, state, device='cpu', causal=True, slot0=0, streams=None, mutant=None, **mags):
    """pair_attn_problem under dropout: slot s of the call takes stream slot0 + s."""
    prob = P.pair_attn_problem(maps, b, h, sq, sk, d, device, causal=causal, slot0=slot0, **mags)
    keep = keep_mask(state, streams or slot0 + b * h, sq, sk, PAIR_P, mutant)[slot0:slot0 + b * h].view(b, h, sq, sk)
    return with_dropout(prob, keep)


def pair_slot_maps(d, dtype, s, rot):
    """The maps of the three slots of rotation `rot`: BWD_MAPS in place, 'diag' standing in for a left-out (map, d, S) -- a
    map keeps its slot, and with it its mask, whatever else is left out."""
    maps = P.slot_maps(P.BWD_MAPS, 3, rot)
    if dtype == torch.float16:
        return maps
    return ['diag' if (m, d, s) in PAIR_BF16_LEFT_OUT else m for m in maps]


def pair_fixed_problems(dtype, device='cpu', cases=None, left_out=True, mutant=None):
    """(tag, problem) of every fixed-length causal pair call in `dtype` under PAIR_STATE['fixed']."""
    for case in P.PAIR_BWD_CASES if cases is None else cases:
        for s in case['seqlens']:
            b, h = P.bh_of(s)
            for rot in P.rotations(P.BWD_MAPS, 3):
                maps = pair_slot_maps(case['d'], dtype, s, rot) if left_out else P.slot_maps(P.BWD_MAPS, 3, rot)
                yield (f"d={case['d']} S={s} maps from {rot}",
                       pair_problem(maps, b, h, s, s, case['d'], PAIR_STATE['fixed'], device, mutant=mutant, **PAIR_MAGS[dtype]))


def pair_cross_problems(dtype, device='cpu', mutant=None):
    c = P.FLASH_CROSS
    maps = P.CROSS_MAPS + P.BWD_MAPS
    for rot in P.rotations(maps, 3):
        yield (f'cross maps from {rot}', pair_problem(P.slot_maps(maps, 3, rot), c['b'], c['h'], c['sq'], c['sk'], c['d'],
                                                      PAIR_STATE['cross'], device, causal=False, mutant=mutant, **PAIR_MAGS[dtype]))


RAGGED_KEYS = ('q', 'k', 'v', 'want', 'dout', 'want_dq', 'want_dk', 'want_dv', 'fan', 'zero_out', 'zero_dq', 'zero_dk')


def pair_ragged_problems(dtype, device='cpu', mutant=None):
    """The ragged batch: every map in both dtypes (nothing is left out), stream = sequence * h + head, rows and columns of the
    mask relative to the sequence."""
    c = P.FLASH_BWD_RAGGED
    nseq, h = len(c['lens']), c['h']
    for rot in P.rotations(P.BWD_MAPS, h):
        parts = [pair_problem(P.slot_maps(P.BWD_MAPS, h, rot + n), 1, h, L, L, c['d'], PAIR_STATE['ragged'], device, slot0=n * h,
                              streams=nseq * h, mutant=mutant, **PAIR_MAGS[dtype]) if L > 0 else None
                 for n, L in enumerate(c['lens'])]
        full = [p for p in parts if p is not None]
        out = {key: torch.cat([p[key][0] for p in full]) for key in RAGGED_KEYS}
        out['cu'] = torch.tensor([0] + torch.tensor(c['lens']).cumsum(0).tolist(), dtype=torch.int32, device=device)
        out['scale'], out['parts'] = full[0]['scale'], full
        out['lse'] = [p['lse'][0] if p is not None else None for p in parts]
        yield f'ragged maps from {rot}', out



# ---- C. LayerNorm ---------------------------------------------------------------------------------------------------------------

LN_ROWS = (70, 257)
# one width of every column class of the forward in tests/rowwise_exact.py (LN_FWD_CH: 1, 2, 6, 8, 16, 24, 32 chunks of 256),
# 768 (3 chunks, the width of the model); 8192 is the widest the training kernel takes
LN_FWD_COLS = (252, 260, 768, 1028, 1540, 3076, 4100, 8192)
LN_BWD_COLS = (252, 260, 768, 1028, 1540, 2048)          # what add_layer_norm_bwd_supported admits, and its widest
LN_P = (0.5, 0.17)


def ln_x0(rows, cols, device='cpu'):
    """Non-zero integers of magnitude 1 ... 8, (rows, cols) fp32: 2 x0 is exact in both dtypes."""
    h = _hash(torch.arange(rows, device=device)[:, None] * 8209 + torch.arange(cols, device=device)[None, :] + 3)
    return ((h >> 4) % 8 + 1).float() * (1 - 2 * ((h >> 9) & 1)).float()


def ln_scales(rows, cols, device='cpu'):
    """Powers of two: rowscale (rows,) in {0.5, 1, 2}, colscale (cols,) in {0.25, 1, 4}."""
    r = 2.0 ** ((_hash(torch.arange(rows, device=device) + 71) % 3).float() - 1)
    c = 4.0 ** ((_hash(torch.arange(cols, device=device) + 113) % 3).float() - 1)
    return r, c


def ln_dz(rows, cols, device='cpu'):
    """An upstream gradient, multiples of 1/8 in [-1, 1]."""
    h = _hash(torch.arange(rows, device=device)[:, None] * 4099 + torch.arange(cols, device=device)[None, :] + 59)
    return ((h >> 3) % 17 - 8).float() / 8


def ln_keep(state, rows, cols, p, mutant=None):
    """philox_ref.rows_keep_mask as a bool tensor (rows, cols)."""
    return keep_mask(state, 1, rows, cols, p, mutant)[0]
