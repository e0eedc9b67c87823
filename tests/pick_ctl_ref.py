"""Host restatement of the controlled token pick (include/bp_hip.h: bp_pick_token_ctl) in numpy, on top of pick_ref -- test
infrastructure shared by test_pick_control_host.py and test_gpu_pick_control.py.  Independent of
src/utils/generation.py::_eager_pick (torch) and of the kernel: the history is a python set, pen two float32 products picked by
np.where, the EOS mask an assignment, and everything behind them is pick_ref's."""
import numpy as np

import pick_ref as R


def history(seq_row, counter, vocab):
    """The set of ids of seq_row[0 : min(counter, len)] inside [0, vocab); seq_row None or counter <= 0: empty."""
    if seq_row is None or counter <= 0:
        return set()
    return {int(v) for v in list(seq_row)[:min(int(counter), len(seq_row))] if 0 <= int(v) < vocab}


def pen(z, hist, theta):
    """float32 z with the members of `hist` multiplied by float32(theta) when negative, else by float32(1) / float32(theta):
    one float32 multiplication either way.  theta == 1 leaves z alone."""
    z = np.asarray(z, dtype=np.float32)
    if theta == 1.0 or not hist:
        return z.copy()
    t = np.float32(theta)
    rt = np.float32(1.0) / t
    member = np.zeros(z.shape[0], dtype=bool)
    member[sorted(hist)] = True
    with np.errstate(invalid='ignore', over='ignore'):
        return np.where(member, np.where(z < 0, z * t, z * rt), z).astype(np.float32)


def eos_masked(z, counter, eos_token_id, min_length):
    z = z.copy()
    if eos_token_id is not None and eos_token_id >= 0 and counter < min_length:
        z[eos_token_id] = -np.inf
    return z


def greedy_values(x, hist, theta, counter, eos_token_id, min_length):
    """pen(float32(x)) under the EOS mask: what the greedy answer is the argmax of."""
    return eos_masked(pen(np.asarray(x, dtype=np.float32), hist, theta), counter, eos_token_id, min_length)


def scaled_values(x, temperature, hist, theta, counter, eos_token_id, min_length):
    """z = pen(float32(x) * float32(1 / T)) under the EOS mask."""
    return eos_masked(pen(R.scaled(x, temperature), hist, theta), counter, eos_token_id, min_length)


def pick(x, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0, offset=0, row=0, counter=0, seq_row=None,
         repetition_penalty=1.0, eos_token_id=None, pad_token_id=None, min_length=0, finished=False):
    """(token, z, keep, u, finished_after) of one row; keep is None for greedy / degenerate / finished rows."""
    vocab = len(x)
    u = R.uniform(seed, offset, row, counter) if do_sample else None
    if finished:
        pad = pad_token_id if pad_token_id is not None else eos_token_id
        return int(pad), None, None, u, True
    hist = history(seq_row, counter, vocab)
    g = R.greedy(greedy_values(x, hist, repetition_penalty, counter, eos_token_id, min_length))
    z, keep, token = None, None, g
    if do_sample:
        z = scaled_values(x, temperature, hist, repetition_penalty, counter, eos_token_id, min_length)
        if not R.degenerate(z):
            keep = R.kept_set(z, top_k, top_p)
            c = R.cdf(z, keep)
            hit = np.nonzero(c > u)[0]
            token = int(hit[0]) if hit.size else int(np.nonzero(keep)[0][-1])
    return token, z, keep, u, bool(eos_token_id is not None and eos_token_id >= 0 and token == eos_token_id)
