"""numpy float64 restatement of the contracts of bp_beam_pick and bp_beam_copy_rows (include/bp_hip.h), shared by
test_beam_host.py and test_gpu_beam_*.py.  Importing it touches no GPU."""
import numpy as np


def eps(vocab, score):
    """Score tolerance per candidate: (V + 64) 2^-24, the bound tests/test_gpu_pick.py uses for an fp32 sum over V terms,
    plus 2^-22 (1 + |score|) for the two fp32 roundings of s + (x - lse)."""
    score = np.where(np.isfinite(score), np.abs(score), 0.0)
    return (vocab + 64) * 2.0 ** -24 + 2.0 ** -22 * (1.0 + score)


def row_scores(x, s):
    """The scores of all candidates of one live row, float64 (vocab,): s + (x - lse), all -inf for a degenerate row."""
    x = np.asarray(x, dtype=np.float64)
    m = np.max(x) if not np.isnan(x).any() else np.nan
    if np.isnan(m) or np.isinf(m):
        return np.full(x.shape, -np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        lse = m + np.log(np.sum(np.exp(x - m)))
        score = float(s) + (x - lse)
    return np.where(np.isnan(score), -np.inf, score)


def row_candidates(x, s, finished, n, pad):
    """The n best candidates [(score, v)] of one row, ranked (score descending, v ascending)."""
    if finished:
        return [(-np.inf if np.isnan(s) else float(s), int(pad))]
    score = row_scores(x, s)
    if score.size > 4 * n:                    # only the columns at or above the n-th best score need sorting
        at = np.flatnonzero(score >= np.partition(score, score.size - n)[score.size - n])
    else:
        at = np.arange(score.size)
    order = at[np.argsort(-score[at], kind='stable')][:n]
    return [(float(score[v]), int(v)) for v in order]


def group_ranking(logits, scores, finished, n, pad):
    """The n best candidates [(score, w, v)] of one group of W rows, ranked (score descending, w, v ascending)."""
    cands = []
    for w in range(logits.shape[0]):
        fin = finished is not None and finished[w] != 0
        cands += [(sc, w, v) for sc, v in row_candidates(logits[w], scores[w], fin, n, pad)]
    cands.sort(key=lambda c: (-c[0], c[1], c[2]))
    return cands[:n]


def assign_slots(winner_rows, W):
    """Slot of every winner, given the parent slot w of each in rank order: its parent's slot when free, else the lowest
    free one (those after all keepers are placed)."""
    free = [True] * W
    slot = [-1] * len(winner_rows)
    for j, w in enumerate(winner_rows):
        if free[w]:
            slot[j], free[w] = w, False
    for j in range(len(winner_rows)):
        if slot[j] < 0:
            slot[j] = free.index(True)
            free[slot[j]] = False
    return slot


def beam_pick(logits, scores, finished, W, eos=-1, pad=0):
    """dict(parent, tokens, scores, finished, ranking): the outputs of bp_beam_pick for logits (groups * W, V) and, per
    group, the W + 1 best candidates (what `decided` looks at).  finished may be None."""
    logits = np.asarray(logits, dtype=np.float64)
    rows, vocab = logits.shape
    groups = rows // W
    parent = np.zeros(rows, dtype=np.int64)
    tokens = np.zeros(rows, dtype=np.int64)
    new_scores = np.zeros(rows, dtype=np.float64)
    new_fin = np.zeros(rows, dtype=np.int64)
    rankings = []
    for g in range(groups):
        sl = slice(g * W, (g + 1) * W)
        fin = None if finished is None else np.asarray(finished)[sl]
        ranking = group_ranking(logits[sl], np.asarray(scores, dtype=np.float64)[sl], fin, W + 1, pad)
        rankings.append(ranking)
        winners = ranking[:W]
        for (sc, w, v), t in zip(winners, assign_slots([c[1] for c in winners], W)):
            was = fin is not None and fin[w] != 0
            parent[g * W + t] = g * W + w
            tokens[g * W + t] = v
            new_scores[g * W + t] = sc
            new_fin[g * W + t] = int(was or (eos >= 0 and not was and v == eos))
    return dict(parent=parent, tokens=tokens, scores=new_scores, finished=new_fin, ranking=rankings)


def decided(ranking, vocab):
    """Whether fp32 arithmetic within eps of these float64 scores must produce this very ranking: among the W + 1 best
    candidates every pair differs by more than the sum of the two tolerances.  Pairs from the same row with exactly equal
    scores are ordered by the tie rule in any arithmetic that is monotone in the logit, and count as decided; so do two
    candidates at -inf (a -inf score stays -inf under every rounding, and then the tie rule orders them)."""
    for i in range(len(ranking)):
        for j in range(i + 1, len(ranking)):
            a, b = ranking[i], ranking[j]
            if a[0] == b[0] and (a[1] == b[1] or a[0] == -np.inf):
                continue
            if not abs(a[0] - b[0]) > eps(vocab, a[0]) + eps(vocab, b[0]):
                return False
    return True


def check_near_tie(got, inputs, g, W, vocab):
    """An undecided group g, held to everything that does not depend on the order of candidates closer than the
    tolerances.  `inputs` = (logits, old scores, old finished or None, eos, pad).  The W slots hold W distinct candidates;
    a finished parent continues with the pad only; each written score is within eps of the reference's score of THAT
    candidate; no candidate of the reference's W best that was left out is better than a chosen one by more than the two
    tolerances; the slots are exactly those of the slot rule applied to the written scores ranked (score descending, w, v
    ascending), which is the order the kernel itself ranks by; the flags follow from (parent, token)."""
    parent, tokens, scores, new_fin = got
    logits, old_scores, old_fin, eos, pad = inputs
    base = g * W
    was = [old_fin is not None and old_fin[base + w] != 0 for w in range(W)]
    chosen = [(int(parent[base + t]) - base, int(tokens[base + t])) for t in range(W)]
    assert len(set(chosen)) == W, (g, chosen)
    live = {w: row_scores(logits[base + w], old_scores[base + w]) for w in {w for w, _ in chosen} if not was[w]}
    want = []
    for t, (w, v) in enumerate(chosen):
        if was[w]:
            assert v == pad, (g, t, w, v)
            ref = -np.inf if np.isnan(old_scores[base + w]) else float(old_scores[base + w])
        else:
            ref = float(live[w][v])
        want.append(ref)
        have = float(scores[base + t])
        assert (np.isinf(ref) and have == ref) or abs(have - ref) <= eps(vocab, ref), (g, t, have, ref)
        if new_fin is not None:
            assert new_fin[base + t] == int(was[w] or (eos >= 0 and v == eos)), (g, t, new_fin[base + t])
    worst = min(want)
    fin = None if old_fin is None else np.asarray(old_fin)[base:base + W]
    best = group_ranking(np.asarray(logits[base:base + W], dtype=np.float64), np.asarray(old_scores, dtype=np.float64)[base:base + W],
                         fin, W, pad)
    for sc, w, v in best:
        if (w, v) not in chosen:
            assert not sc - worst > eps(vocab, sc) + eps(vocab, worst), (g, (sc, w, v), worst)
    ranked = sorted(range(W), key=lambda t: (-float(scores[base + t]), chosen[t][0], chosen[t][1]))
    assert assign_slots([chosen[t][0] for t in ranked], W) == ranked, (g, chosen, [float(scores[base + t]) for t in range(W)])


def check(got, ref, W, vocab, check_finished=True, inputs=None):
    """(parent, tokens, scores, finished) numpy arrays of an implementation against beam_pick's dict: parent[parent] ==
    parent everywhere, parents inside their group, and in the decided groups parent / tokens / finished exactly and the
    scores within eps.  Returns the number of undecided groups; with `inputs` (see check_near_tie) those are not left out
    altogether but held to all that their near ties leave determined."""
    parent, tokens, scores, fin = got
    parent = np.asarray(parent)
    assert (parent[parent] == parent).all(), parent
    undecided = 0
    for g, ranking in enumerate(ref['ranking']):
        sl = slice(g * W, (g + 1) * W)
        assert (parent[sl] // W == g).all(), (g, parent[sl])
        if not decided(ranking, vocab):
            undecided += 1
            if inputs is not None:
                check_near_tie((parent, tokens, scores, fin if check_finished else None), inputs, g, W, vocab)
            continue
        assert (parent[sl] == ref['parent'][sl]).all(), (g, parent[sl], ref['parent'][sl])
        assert (tokens[sl] == ref['tokens'][sl]).all(), (g, tokens[sl], ref['tokens'][sl])
        if check_finished:
            assert (fin[sl] == ref['finished'][sl]).all(), (g, fin[sl], ref['finished'][sl])
        want = ref['scores'][sl]
        with np.errstate(invalid='ignore'):
            close = np.abs(scores[sl] - want) <= eps(vocab, want)
        assert ((np.isinf(want) & (scores[sl] == want)) | close).all(), (g, scores[sl], want)
    return undecided


def copy_rows(arrays, parent, lengths, first_position):
    """bp_beam_copy_rows on (rows, positions, ...) numpy arrays, returned as new arrays."""
    out = []
    for a in arrays:
        new = a.copy()
        for r in range(a.shape[0]):
            n = min(max(int(lengths[r]), 0), a.shape[1])
            if parent[r] != r and n > first_position:
                new[r, first_position:n] = a[parent[r], first_position:n]
        out.append(new)
    return out


DRAWN_VOCABS = (8, 63, 64, 65, 257, 4096)     # the draw below leaves 0-1 % of groups undecided there (26 % at 50264, W = 8)
UNDECIDED_CAP = 0.05


def draw(groups, W, vocab, seed, dtype=None, finished_share=0.0):
    """The drawn case of the beam tests: logits 3 N(0, 1) (rounded to `dtype`, a torch 16-bit type, when given), beam scores
    uniform in [-20, 0], a share of rows finished.  (logits fp32 array, scores fp32, finished int32)."""
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((groups * W, vocab))).astype(np.float32)
    if dtype is not None:
        import torch
        x = torch.from_numpy(x).to(dtype).float().numpy()
    s = rng.uniform(-20.0, 0.0, size=groups * W).astype(np.float32)
    fin = (rng.uniform(size=groups * W) < finished_share).astype(np.int32)
    return x, s, fin


def planted(W, vocab, w0, v0, seed):
    """One group whose W + 2 best candidates are planted spikes at least 0.5 apart over noise of 0.01, the best of them
    (w0, v0): row (w0 + k) % W has a spike of 24 (at v0 for k = 0) and the beam score that puts that candidate at -k; row w0
    has two more spikes, at -0.5 and -1.5.  (logits fp32 (W, vocab), beam scores fp32 (W,).)  Needs vocab >= 3."""
    rng = np.random.default_rng(seed)
    x = (0.01 * rng.uniform(-1.0, 1.0, size=(W, vocab))).astype(np.float32)
    scores = np.zeros(W, dtype=np.float32)
    others = [v for v in rng.permutation(vocab)[:3] if v != v0][:2]
    for k in range(W):
        w = (w0 + k) % W
        x[w, v0 if k == 0 else int(rng.integers(0, vocab))] = 24.0
        if k == 0:
            x[w, others[0]], x[w, others[1]] = 23.5, 22.5
        row = x[w].astype(np.float64)
        scores[w] = -k + (np.log(np.sum(np.exp(row - 24.0))))
    return x, scores


def logprob_group(W, vocab, cands):
    """Logits of one group that ARE log-probabilities: cands {(w, v): logp}; the other columns of every row share the rest
    of the row's mass evenly (far below the planted ones at the sizes used here)."""
    x = np.zeros((W, vocab), dtype=np.float64)
    for w in range(W):
        mine = {v: lp for (cw, v), lp in cands.items() if cw == w}
        x[w] = np.log((1.0 - sum(np.exp(lp) for lp in mine.values())) / (vocab - len(mine)))
        for v, lp in mine.items():
            x[w, v] = lp
    return x.astype(np.float32)
