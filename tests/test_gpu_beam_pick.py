"""GPU: bp_beam_pick (csrc/beam_pick.hip) against the float64 restatement of tests/beam_ref.py.  Drawn groups that the
reference calls decided (its W + 1 best candidates further apart than the tolerances, beam_ref.decided) must match parent,
tokens and finished exactly and the scores within eps = (V + 64) 2^-24 + 2^-22 (1 + |score|); at most 5 % of the drawn
groups may be undecided (test_beam_host.py holds the reference alone to that).  Planted groups are decided by
construction and are checked at every size, Small's vocabulary included."""
import numpy as np
import pytest
import torch

import beam_ref as R
from decode_support import DEV, _bp

pytestmark = pytest.mark.gpu

INF = float('inf')
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
GUARD = 8


def _place(rows, dtype, pad=0, misalign=0):
    """(R, vocab) host fp32 rows -> a device tensor of `dtype` with row stride vocab + pad whose base is `misalign`
    elements behind a 16-byte boundary."""
    rows = torch.as_tensor(rows, dtype=torch.float32)
    b, v = rows.shape
    flat = torch.zeros(b * (v + pad) + 16, dtype=dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = flat[misalign:misalign + b * (v + pad)].view(b, v + pad)[:, :v]
    view.copy_(rows.to(dtype))
    return view


def _guarded(values, dtype, canary):
    """A device vector holding `values` between two runs of GUARD canaries: (the view, the whole buffer)."""
    values = torch.as_tensor(values).to(dtype)
    whole = torch.full((values.numel() + 2 * GUARD,), canary, dtype=dtype, device=DEV)
    whole[GUARD:-GUARD] = values.to(DEV)
    return whole[GUARD:-GUARD], whole


def _guards_intact(whole, canary):
    return bool((whole[:GUARD] == canary).all() and (whole[-GUARD:] == canary).all())


def _run(x, s, fin, W, dtype, eos=None, pad=None, layout='dense', counters=None, seq_cols=0):
    """bp_beam_pick on host arrays: (outputs (parent, tokens, scores, finished) as numpy, sequences or None, the logits as
    the kernel saw them (fp32 numpy)); every output sits between canaries, the logits must come back unchanged."""
    bp = _bp()
    rows = x.shape[0]
    if isinstance(layout, tuple):                                      # ('same-head', h): every row h elements behind a 16-byte boundary
        lpad, mis = (-x.shape[1]) % 8 + 8, layout[1]
    else:
        lpad, mis = (0, 0) if layout == 'dense' else (13, 3 if dtype != 'fp32' else 1)
    logits = _place(x, DTYPES[dtype], lpad, mis)
    assert layout == 'dense' or (logits.data_ptr() % 16 != 0 and logits.stride(0) > x.shape[1])
    assert not isinstance(layout, tuple) or logits.stride(0) * logits.element_size() % 16 == 0
    before = logits.clone()
    scores, scores_w = _guarded(s, torch.float32, -777.0)
    parent, parent_w = _guarded(np.full(rows, -5), torch.int32, -9)
    tokens, tokens_w = _guarded(np.full(rows, -5), torch.int64, -9)
    flags, flags_w = _guarded(fin, torch.int32, -9) if fin is not None else (None, None)
    seq = seq_w = cnt = None
    if seq_cols:
        seq_w = torch.full((rows + 2, seq_cols + 3), -9, dtype=torch.int64, device=DEV)
        seq = seq_w[1:-1, :seq_cols]                                   # strided rows, canaries all around
        cnt = torch.as_tensor(counters, dtype=torch.int32).to(DEV)
    out = bp.beam_pick(logits, scores, parent, W, finished=flags, tokens=tokens, sequences=seq, counters=cnt,
                       eos_token_id=eos, pad_token_id=pad)
    torch.cuda.synchronize()
    assert out.data_ptr() == tokens.data_ptr()
    assert torch.equal(logits.view(torch.int16 if dtype != 'fp32' else torch.int32),
                       before.view(torch.int16 if dtype != 'fp32' else torch.int32)), 'logits are only read'
    assert _guards_intact(scores_w, -777.0) and _guards_intact(parent_w, -9) and _guards_intact(tokens_w, -9)
    assert flags_w is None or _guards_intact(flags_w, -9)
    got = (parent.cpu().numpy(), tokens.cpu().numpy(), scores.cpu().numpy(), None if flags is None else flags.cpu().numpy())
    if seq_cols:
        cols = np.asarray(counters)
        want = np.full((rows + 2, seq_cols + 3), -9, dtype=np.int64)
        for r in range(rows):
            if 0 <= cols[r] < seq_cols:
                want[r + 1, cols[r]] = got[1][r]
        assert (seq_w.cpu().numpy() == want).all(), 'a row receives its token at column counters[r], nothing else is written'
    return got, logits.float().cpu().numpy()


# ---- drawn groups ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('W', [1, 2, 3, 8])
@pytest.mark.parametrize('vocab', R.DRAWN_VOCABS)
def test_drawn_groups_match_the_reference(vocab, W, dtype):
    groups = 40
    x, s, fin = R.draw(groups, W, vocab, seed=10 * vocab + W, finished_share=0.2)
    layout = 'strided-misaligned' if (vocab + W) % 2 else 'dense'
    counters = np.arange(groups * W) % 7 - 1                           # -1 and 5 fall outside the five columns
    got, seen = _run(x, s, fin, W, dtype, eos=1, pad=0, layout=layout, counters=counters, seq_cols=5)
    undecided = R.check(got, R.beam_pick(seen, s, fin, W, eos=1, pad=0), W, vocab, inputs=(seen, s, fin, 1, 0))
    print(f'V={vocab} W={W} {dtype}: {undecided} of {groups} groups undecided and left out')
    assert undecided <= R.UNDECIDED_CAP * groups
    again, _ = _run(x, s, fin, W, dtype, eos=1, pad=0, layout=layout, counters=counters, seq_cols=5)
    for a, b in zip(got, again):
        assert (a.view(np.int32 if a.dtype == np.float32 else a.dtype) == b.view(np.int32 if b.dtype == np.float32 else b.dtype)).all(), \
            'two calls give the same bits'


# ---- planted groups: exact at every size ------------------------------------------------------------------------------------------------

WAVES, LANES = 16, 64           # the 1024-thread workgroup of stage 1 (csrc/vocab_row.h: kPickWaves, RowView)
ALL_EDGES_BUDGET = 80_000_000   # logits of one needle case: below it every chunk edge is planted, above it the classes


def _owner(c, cpw):
    """(wave, step, lane) that reads 16-byte chunk c of a row: wave * cpw + step * 64 + lane (RowView::chunk)."""
    return c // cpw, c % cpw // LANES, c % cpw % LANES


def _edge_classes(nch, cpw):
    """The chunk edges c (between chunks c - 1 and c) that stand for every kind of boundary between two owners: every
    edge between the runs of two waves; in the first and the last wave every edge between two steps, in every other wave
    one of them; and for every lane l >= 1 one edge between lanes l - 1 and l of one step, the wave and step going round."""
    waves = (nch + cpw - 1) // cpw
    edges = set()
    for wave in range(waves):
        run = min(cpw, nch - wave * cpw)
        steps = (run + LANES - 1) // LANES
        if wave:
            edges.add(wave * cpw)
        between = list(range(1, steps))
        for st in between if wave in (0, waves - 1) else between[wave % max(len(between), 1):][:1]:
            edges.add(wave * cpw + st * LANES)
    for lane in range(1, min(LANES, cpw)):
        wave = lane % waves
        run = min(cpw, nch - wave * cpw)
        steps_with_lane = (run - lane + LANES - 1) // LANES            # steps st with st * 64 + lane < run
        if steps_with_lane < 1:
            wave, steps_with_lane = 0, (cpw - lane + LANES - 1) // LANES
        edges.add(wave * cpw + (lane // waves) % steps_with_lane * LANES + lane)
    return edges


def _assert_every_boundary_kind(edges, nch, cpw):
    """What _edge_classes promises, checked on the edges a case really plants (all of them or the classes)."""
    assert all(0 < c < nch for c in edges)
    waves = (nch + cpw - 1) // cpw
    owners = {c: (_owner(c - 1, cpw), _owner(c, cpw)) for c in edges}
    assert {hi[0] for lo, hi in owners.values() if lo[0] != hi[0]} == set(range(1, waves)), 'an edge between every two waves'
    step_edges = {(hi[0], hi[1]) for lo, hi in owners.values() if lo[0] == hi[0] and lo[1] != hi[1]}
    for wave in range(waves):
        steps = (min(cpw, nch - wave * cpw) + LANES - 1) // LANES
        have = {st for w, st in step_edges if w == wave}
        assert have == set(range(1, steps)) if wave in (0, waves - 1) else (have or steps < 2), (wave, have, steps)
    lanes = {hi[2] for lo, hi in owners.values() if lo[:2] == hi[:2]}
    assert lanes == set(range(1, min(LANES, cpw))), 'an edge between every two neighbouring lanes'


def _needle_cases(vocab, W, dtype, head):
    """(w0, v0) of every planted group.  In EVERY row w: v in {0, 7, 8, V - 1} and both sides of the first and of the
    last 16-byte chunk edge.  Both sides of chunk edges: when the case stays under ALL_EDGES_BUDGET logits (every V <= 4096 does), every edge of
    the row, in every row for V <= 257 and in rows that go round with the edge above that; else the edges of _edge_classes,
    rows going round.  Stage 1 runs one workgroup per row which reads that row alone, with the same (wave, step, lane)
    map in every row (all rows share `head` here: the row stride is a multiple of 16 bytes), so which row a chunk edge
    is probed in changes nothing about who owns it; what depends on w, the merge of stage 2 and the parent it writes,
    sees a needle in every row through the first group of columns."""
    n = 4 if dtype == 'fp32' else 8
    nch = (vocab + head + n - 1) // n
    cpw = (nch + WAVES - 1) // WAVES
    column = lambda c: c * n - head                                     # the first column of chunk c
    everywhere = {0, 7, 8, vocab - 1, column(1) - 1, column(1), column(nch - 1) - 1, column(nch - 1)}
    cases = [(w, v) for v in sorted(everywhere) if 0 <= v < vocab for w in range(W)]
    edges = set(range(1, nch))
    if 2 * len(edges) * W * vocab > ALL_EDGES_BUDGET:
        edges = _edge_classes(nch, cpw)
    _assert_every_boundary_kind(edges, nch, cpw)
    turn = 0
    for c in sorted(edges):
        for v in (column(c) - 1, column(c)):
            if 0 <= v < vocab:
                rows = range(W) if vocab <= 257 else [turn % W]
                cases += [(w, v) for w in rows]
                turn += 1
    return cases


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('vocab,W', [(8, 1), (8, 4), (8, 8), (63, 4), (64, 3), (65, 4), (257, 8), (4096, 4), (4096, 8),
                                     (50264, 4), (50264, 8)])
def test_a_needle_wins_with_its_parent(vocab, W, dtype):
    head = {'bf16': 3, 'fp16': 5, 'fp32': 1}[dtype]
    cases = _needle_cases(vocab, W, dtype, head)
    parent, tokens, scores = [], [], []
    for lo in range(0, len(cases), 256):                                # a batch of groups a launch: the logits stay small
        part = cases[lo:lo + 256]
        xs, ss = zip(*(R.planted(W, vocab, w0, v0, seed=vocab + 31 * (lo + i)) for i, (w0, v0) in enumerate(part)))
        x, s = np.concatenate(xs), np.concatenate(ss)
        fin = np.zeros(len(s), dtype=np.int32)
        got, seen = _run(x, s, fin, W, dtype, eos=None, layout=('same-head', head))
        assert R.check(got, R.beam_pick(seen, s, fin, W), W, vocab) == 0, 'planted groups are decided'
        assert not got[3].any()
        parent, tokens, scores = parent + [got[0]], tokens + [got[1]], scores + [got[2]]
    parent, tokens, scores = np.concatenate(parent), np.concatenate(tokens), np.concatenate(scores)
    for g, (w0, v0) in enumerate(cases):
        at = g * W + w0
        assert parent[at] == at - g // 256 * 256 * W and tokens[at] == v0, (g, w0, v0)   # parents count within their launch
        assert abs(scores[at]) <= R.eps(vocab, 0.0)


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('vocab', [8, 65, 50264])
def test_exact_cases(vocab, dtype):
    W = 4
    rng = np.random.default_rng(vocab)
    zero = np.zeros(W, dtype=np.float32)
    # all logits and scores equal: winners (0, 0 .. W - 1); slot 0 keeps (0, 0), the others fill slots 1 .. W - 1 in order
    (parent, tokens, scores, flags), _ = _run(np.full((W, vocab), 0.25, dtype=np.float32), zero, None, W, dtype)
    assert parent.tolist() == [0] * W and tokens.tolist() == list(range(W)) and flags is None
    assert np.abs(scores + np.log(vocab)).max() <= R.eps(vocab, np.log(vocab))
    # the -inf start: every winner comes from beam 0, in the order of its logits
    x = (0.01 * rng.uniform(-1, 1, size=(W, vocab))).astype(np.float32)
    cols = rng.permutation(vocab)[:W + 1]
    x[0, cols] = 10.0 - np.arange(W + 1)
    x[1:, cols[-1]] = 30.0                                              # what the dead beams like does not matter
    start = np.array([0.0] + [-INF] * (W - 1), dtype=np.float32)
    got, seen = _run(x, start, np.zeros(W, dtype=np.int32), W, dtype, eos=int(cols[1]), pad=0, layout='strided-misaligned')
    assert got[0].tolist() == [0] * W and got[1].tolist() == cols[:W].tolist()
    assert got[3].tolist() == [0, 1] + [0] * (W - 2)                    # the EOS pick sets the flag of its slot
    assert R.check(got, R.beam_pick(seen, start, np.zeros(W, dtype=np.int32), W, eos=int(cols[1])), W, vocab) == 0
    # a finished row keeps its score, bit for bit, and emits the pad; a NaN score and a dead row rank as -inf
    x, s = R.planted(W, vocab, 1, 5, seed=vocab)
    s[0], fin = -0.3203125, np.array([1, 0, 0, 0], dtype=np.int32)
    got, seen = _run(x, s, fin, W, dtype, eos=2, pad=6)
    assert got[0][0] == 0 and got[1][0] == 6 and got[2][0] == np.float32(-0.3203125) and got[3][0] == 1
    assert R.check(got, R.beam_pick(seen, s, fin, W, eos=2, pad=6), W, vocab) == 0
    s2 = s.copy()
    s2[2] = np.nan
    x2 = x.copy()
    x2[3, 1] = np.nan
    got, seen = _run(x2, s2, fin, W, dtype, eos=2, pad=6)
    ref = R.beam_pick(seen, s2, fin, W, eos=2, pad=6)
    assert R.check(got, ref, W, vocab) == 0 and not np.isnan(got[2]).any()
    assert sorted(set(got[0].tolist())) == [0, 1]                       # rows 2 and 3 have nothing above -inf


def test_a_pick_of_the_eos_sets_the_flag_of_its_slot():
    W, V = 3, 16
    x = R.logprob_group(W, V, {(1, 3): -0.5, (1, 2): -1.0, (2, 4): -1.2})
    for dtype in sorted(DTYPES):
        (parent, tokens, scores, flags), _ = _run(x, np.array([-30.0, 0.0, 0.0], dtype=np.float32),
                                                  np.zeros(W, dtype=np.int32), W, dtype, eos=2, pad=0)
        assert parent.tolist() == [1, 1, 2] and tokens.tolist() == [2, 3, 4] and flags.tolist() == [1, 0, 0]
