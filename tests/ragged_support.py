"""What the tests of generation from right-padded prompts of different lengths share (test_ragged_prompts_host.py,
test_gpu_ragged_prompts.py): the case of the issue, teacher forcing through the loop's own model calls, and the restated ends
of the rows.  Importing it touches no GPU."""
import torch

BATCH, S, LENGTHS, MAX_LENGTH = 4, 8, (1, 5, 8, 8), 40
N = MAX_LENGTH - 1 - S                      # tokens every row generates: width = max(S, max_length - 1) = 39


def padded(ids, lengths, pad):
    """`ids` (batch, S) with the pad behind every row's prompt: what the loop feeds its prefill."""
    cols = torch.arange(ids.shape[1], device=ids.device)[None, :]
    at = torch.as_tensor(lengths, device=ids.device)[:, None]
    return torch.where(cols < at, ids, torch.full_like(ids, pad))


def loop_logits(model, ids, lengths, sequences, new_tokens, pad=0, capacity=None):
    """(new_tokens, batch, vocab): entry [i, b] is the logits the pick of column lengths[b] + i of row b saw, recomputed by
    the loop's own calls on the tokens of `sequences` -- the padded prefill, the row gather, then one-token cached steps on
    device lengths that start at the rows' own.  Also returns the InferenceParams, whose caches (of `capacity` positions,
    default the width) then hold the first lengths[b] + new_tokens - 1 positions of every row."""
    from src.utils.generation import InferenceParams
    batch, width = ids.shape[0], ids.shape[1] + new_tokens
    at = torch.as_tensor(lengths, device=ids.device)
    ip = InferenceParams(max_sequence_len=width if capacity is None else capacity, max_batch_size=batch)
    ip.lengths_per_sample = torch.zeros((batch,), dtype=torch.int32, device=ids.device)
    rows = torch.arange(batch, device=ids.device)
    out = []
    with torch.inference_mode():
        logits = model(padded(ids, lengths, pad), inference_params=ip).logits
        out.append(logits[rows, at - 1])
        ip.sequence_len_offset = ids.shape[1]
        ip.lengths_per_sample.copy_(at)
        for i in range(new_tokens - 1):
            fed = sequences[rows, at + i].unsqueeze(1).contiguous()
            out.append(model(fed, inference_params=ip).logits[:, -1])
            ip.lengths_per_sample += 1
            ip.sequence_len_offset += 1
    return torch.stack([t.clone() for t in out]), ip


def ends(sequences, lengths, new_tokens, eos):
    """end_b by the contract, in python: 1 + the first column >= L_b (and < L_b + N) holding the EOS id, else L_b + N."""
    out = []
    for row, begin in zip(sequences.tolist(), lengths):
        hits = [c for c in range(begin, min(begin + new_tokens, len(row))) if eos is not None and row[c] == eos]
        out.append(hits[0] + 1 if hits else begin + new_tokens)
    return out
