"""Host restatement of the limited token pick (include/bp_hip.h: bp_pick_token_lim) in numpy, on top of pick_ctl_ref -- test
infrastructure shared by test_pick_limits_host.py and test_gpu_pick_limits.py.  Independent of
src/utils/generation.py::_eager_pick (torch) and of the kernel: the n-gram set comes from python lists and sets, the counts
from collections.Counter, the fma from a float64 product and sum that is asserted to be exact, and the hash of the kernel's
count table is restated so that the tests can plant collisions."""
from collections import Counter

import numpy as np

import pick_ctl_ref as C
import pick_ref as R

ID_BITS = 19
MAX_NGRAM, MAX_COUNTED_COLS, MAX_LIMITED_VOCAB, MAX_LDS_BYTES = 64, 8191, 2 ** 19, 160 * 1024
STATIC_LDS = 68112                      # PickShared


def clamped_history(seq_row, counter):
    """h = seq_row[0 : Lh] as a list of python ints, Lh = min(max(counter, 0), len); no row: empty."""
    if seq_row is None:
        return []
    return [int(v) for v in list(seq_row)[:min(max(int(counter), 0), len(seq_row))]]


def ngram_set(h, n, vocab):
    """The ids inside [0, vocab) that would complete an n-gram h already holds: h[i + n - 1] for 0 <= i <= len(h) - n with
    h[i : i + n - 1] == the last n - 1 entries of h.  The raw values are compared; n = 1 gives every id of h."""
    if n <= 0 or len(h) < n:
        return set()
    tail = h[len(h) - (n - 1):] if n > 1 else []
    return {h[i + n - 1] for i in range(len(h) - n + 1) if h[i:i + n - 1] == tail and 0 <= h[i + n - 1] < vocab}


def counts(h, begin, vocab):
    """Counter of the ids inside [0, vocab) at the positions [min(begin, len(h)), len(h))."""
    return Counter(v for v in h[min(max(int(begin), 0), len(h)):] if 0 <= v < vocab)


def count_penalty(frequency_penalty, presence_penalty, n):
    """float32 fma(a_f, n, a_p): the float64 product is exact (24 + 13 bits); the sum must be, for the inputs a test uses."""
    a_f, a_p = np.float32(frequency_penalty), np.float32(presence_penalty)
    total = np.float64(a_f) * n + np.float64(a_p)
    if np.isfinite(total):
        from fractions import Fraction
        assert Fraction(float(a_f)) * n + Fraction(float(a_p)) == Fraction(float(total)), 'inexact in float64: choose other penalties'
    with np.errstate(over='ignore'):
        return np.float32(total)


def limited(z, h, vocab, no_repeat_ngram_size=0, frequency_penalty=0.0, presence_penalty=0.0, penalty_begin=0,
            suppress_tokens=None):
    """Steps 2 and 3 of the contract on float32 values that already carry pen(): the count penalty, then the bans (the EOS
    mask stays with pick_ctl_ref.eos_masked)."""
    z = np.asarray(z, dtype=np.float32).copy()
    if frequency_penalty != 0.0 or presence_penalty != 0.0:
        with np.errstate(invalid='ignore', over='ignore'):
            for v, n in counts(h, penalty_begin, vocab).items():
                z[v] = np.float32(z[v] - count_penalty(frequency_penalty, presence_penalty, n))
    banned = ngram_set(h, no_repeat_ngram_size, vocab)
    banned |= {int(t) for t in (suppress_tokens if suppress_tokens is not None else []) if 0 <= int(t) < vocab}
    if banned:
        z[sorted(banned)] = -np.inf
    return z


def values(x, temperature, seq_row, counter, vocab, repetition_penalty=1.0, eos_token_id=None, min_length=0, **limits):
    """What every pass sees: pen(float32(x) [* float32(1 / T)]), the count penalty, the bans, the EOS mask.  temperature None:
    the greedy values."""
    h = clamped_history(seq_row, counter)
    base = np.asarray(x, dtype=np.float32) if temperature is None else R.scaled(x, temperature)
    z = limited(C.pen(base, C.history(seq_row, counter, vocab), repetition_penalty), h, vocab, **limits)
    return C.eos_masked(z, counter, eos_token_id, min_length)


def pick(x, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0, offset=0, row=0, counter=0, seq_row=None,
         repetition_penalty=1.0, eos_token_id=None, pad_token_id=None, min_length=0, finished=False, **limits):
    """(token, z, keep, u, finished_after) of one row, as pick_ctl_ref.pick."""
    vocab = len(x)
    u = R.uniform(seed, offset, row, counter) if do_sample else None
    if finished:
        pad = pad_token_id if pad_token_id is not None else eos_token_id
        return int(pad), None, None, u, True
    kw = dict(repetition_penalty=repetition_penalty, eos_token_id=eos_token_id, min_length=min_length, **limits)
    token = R.greedy(values(x, None, seq_row, counter, vocab, **kw))
    z, keep = None, None
    if do_sample:
        z = values(x, temperature, seq_row, counter, vocab, **kw)
        if not R.degenerate(z):
            keep = R.kept_set(z, top_k, top_p)
            c = R.cdf(z, keep)
            hit = np.nonzero(c > u)[0]
            token = int(hit[0]) if hit.size else int(np.nonzero(keep)[0][-1])
    return token, z, keep, u, bool(eos_token_id is not None and eos_token_id >= 0 and token == eos_token_id)


# ---- the count table of the kernel (csrc/pick_core.h: lim_hash, LimLayout) -------------------------------------------------------------

def table_slots(seq_cols):
    """The power of two >= 2 seq_cols, at least 2."""
    slots = 2
    while slots < 2 * seq_cols:
        slots *= 2
    return slots


def table_slot(token, seq_cols):
    """First slot the kernel probes for `token`: the top log2(slots) bits of the 32-bit product with 2654435761."""
    log2 = table_slots(seq_cols).bit_length() - 1
    return ((int(token) * 2654435761) & 0xFFFFFFFF) >> (32 - log2)


def colliding_ids(seq_cols, vocab, how_many, slot=None):
    """`how_many` ids below `vocab` that start their probe in one slot (the slot of id 1 by default)."""
    slot = table_slot(1, seq_cols) if slot is None else slot
    ids = [t for t in range(vocab) if table_slot(t, seq_cols) == slot][:how_many]
    assert len(ids) == how_many, 'the vocabulary holds too few ids of that slot'
    return ids


def lds_bytes(vocab, seq_cols, repetition_penalty=1.0, no_repeat_ngram_size=0, frequency_penalty=0.0, presence_penalty=0.0,
              n_suppress=0):
    """Static + dynamic LDS of a launch: a bitmap of (vocab + 31) // 32 + 1 words for the history (a penalty of either kind) and
    one for the bans, and the count table."""
    words = (vocab + 31) // 32 + 1
    counted = frequency_penalty != 0.0 or presence_penalty != 0.0
    total = STATIC_LDS
    total += 4 * words * (repetition_penalty != 1.0 or counted)
    total += 4 * words * (no_repeat_ngram_size > 0 or n_suppress > 0)
    total += 4 * table_slots(seq_cols) * counted
    return total
