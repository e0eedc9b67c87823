"""Host restatement of the two phrase matches of bp_pick_token_phrases (include/bp_hip.h) in plain python, on top of
pick_lim_ref -- test infrastructure shared by test_pick_phrases_host.py and test_gpu_pick_phrases.py.  Independent of
src/utils/generation.py (torch) and of the kernel: a phrase is a python list, a match is a comparison of list slices."""
import numpy as np

import pick_lim_ref as L
import pick_ref as R

MAX_PHRASE_LEN, MAX_PHRASES = 64, 1024


def unpack(ids, offsets, total=None):
    """The phrases the DEVICE sees in a packed pair, in order, None for one it ignores: offsets that leave [0, total] or a
    length outside 1..MAX_PHRASE_LEN.  Indices are kept, so a reason 1 + j still names entry j of the list."""
    ids, offsets = [int(v) for v in ids], [int(v) for v in offsets]
    total = len(ids) if total is None else total
    out = []
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        ok = 0 <= lo and hi <= total and 1 <= hi - lo <= MAX_PHRASE_LEN
        out.append(ids[lo:hi] if ok else None)
    return out


def pack(phrases):
    """(ids, offsets) int32 arrays of a list of lists."""
    offsets = np.cumsum([0] + [len(w) for w in phrases]).astype(np.int32)
    return np.array([t for w in phrases for t in w], dtype=np.int32), offsets


def banned_by_phrases(h, phrases, vocab):
    """The set of ids inside [0, vocab) that the ban phrases forbid behind the history h (a list of ints, already clamped): the
    last id of every phrase whose other ids are the end of h, raw values compared; a phrase of one id always bans it."""
    h = [int(v) for v in h]
    banned = set()
    for w in phrases:
        if w is None:
            continue
        head, last = [int(t) for t in w[:-1]], int(w[-1])
        if len(h) >= len(head) and h[len(h) - len(head):] == head and 0 <= last < vocab:
            banned.add(last)
    return banned


def stop_match(h, token, c, begin, minimum, phrases, eos):
    """What ends a row that picked `token` for column c behind the UNCLAMPED history h = row[0 : c] (None: the token has no
    column, c outside [0, seq_cols), or there is no row): None nothing, 0 the EOS id, 1 + j the lowest stop phrase j that is
    the end of h ++ [token] and begins at or behind `begin`, asked only once c >= minimum.  begin, minimum: clamped at 0."""
    if eos is not None and eos >= 0 and int(token) == eos:
        return 0
    if h is None or c < max(int(minimum), 0):
        return None
    text = [int(v) for v in h] + [int(token)]
    assert len(text) == c + 1
    for j, w in enumerate(phrases):
        if w is None:
            continue
        n = len(w)
        if c + 1 - n >= max(int(begin), 0) and text[c + 1 - n:] == [int(t) for t in w]:
            return 1 + j
    return None


def values(x, temperature, seq_row, counter, vocab, ban_phrases=(), **kw):
    """pick_lim_ref.values with the ban phrases' ids as -inf too (one more source of step 3 of the contract)."""
    z = L.values(x, temperature, seq_row, counter, vocab, **kw)
    banned = banned_by_phrases(L.clamped_history(seq_row, counter), ban_phrases, vocab)
    if banned:
        z[sorted(banned)] = -np.inf
    return z


def step(x, seq_row, counter, finished, begin, minimum, ban_phrases, stop_phrases, eos=None, pad=0, **kw):
    """One greedy pick of one row as the kernel makes it: (token, reason) with reason None when the row does not end here.  A
    row finished on entry takes the pad and ends nowhere."""
    if finished:
        return pad, None
    vocab = len(x)
    token = R.greedy(values(x, None, seq_row, counter, vocab, ban_phrases, eos_token_id=eos, min_length=max(minimum, 0),
                            penalty_begin=max(begin, 0), **kw))
    has_column = seq_row is not None and 0 <= counter < len(seq_row)
    h = [int(v) for v in seq_row[:counter]] if has_column else None
    return token, stop_match(h, token, counter, begin, minimum, stop_phrases, eos)
