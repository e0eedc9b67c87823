"""What the tests of the packed prefill share (test_gpu_packed_prefill.py): the case of tests/test_gpu_packed_forward.py with
N generated tokens behind every prompt, and teacher forcing through the calls the loop itself makes with packed_prefill=True.
Importing it touches no GPU."""
import torch

LENGTHS = (1, 70, 37, 130, 64, 5)          # 307 positions; 130 > 128: two flash query tiles, 64 / 70: a key tile and a bit
BATCH, S, N = len(LENGTHS), max(LENGTHS), 6
MAX_LENGTH = S + N + 1                      # width = max(S, max_length - 1) = S + N: every row generates N tokens
WIDTH = S + N


def padded_ids(vocab, device, seed=3):
    """(BATCH, S) ids in [1, vocab) with 0 behind every row's prompt."""
    ids = torch.randint(1, vocab, (BATCH, S), generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(LENGTHS):
        ids[b, n:] = 0
    return ids.to(device)


def pack(ids, lengths):
    """(packed ids (total,), cu_seqlens (B + 1,) int32, max_seqlen) of right-padded ids, from host lengths alone."""
    index = torch.cat([torch.arange(b * ids.shape[1], b * ids.shape[1] + n) for b, n in enumerate(lengths)]).to(ids.device)
    cu = torch.tensor([0] + list(lengths), dtype=torch.int64).cumsum(0).to(device=ids.device, dtype=torch.int32)
    return ids.reshape(-1).index_select(0, index), cu, max(lengths)


def packed_loop_logits(model, ids, lengths, sequences, new_tokens, capacity=None):
    """ragged_support.loop_logits for the loop with packed_prefill=True: (new_tokens, batch, vocab), entry [i, b] the logits
    the pick of column lengths[b] + i of row b saw, recomputed by the loop's own calls on the tokens of `sequences` -- the
    packed prefill of the trunk-and-head model (inference_params + cu_seqlens + max_seqlen), the LM head over the rows' last
    positions alone, then one-token cached steps on device lengths that start at the rows' own.  Also returns the
    InferenceParams, whose caches then hold the first lengths[b] + new_tokens - 1 positions of every row."""
    from src.utils.generation import InferenceParams
    batch, width = ids.shape[0], ids.shape[1] + new_tokens
    at = torch.as_tensor(lengths, device=ids.device)
    ip = InferenceParams(max_sequence_len=width if capacity is None else capacity, max_batch_size=batch)
    ip.lengths_per_sample = torch.zeros((batch,), dtype=torch.int32, device=ids.device)
    rows = torch.arange(batch, device=ids.device)
    packed, cu, longest = pack(ids, lengths)
    out = []
    with torch.inference_mode():
        hidden = model.transformer(packed, inference_params=ip, cu_seqlens=cu, max_seqlen=longest)
        out.append(model.lm_head(hidden.index_select(0, cu[1:].long() - 1)))
        ip.sequence_len_offset = ids.shape[1]
        ip.lengths_per_sample.copy_(at)
        for i in range(new_tokens - 1):
            fed = sequences[rows, at + i].unsqueeze(1).contiguous()
            out.append(model(fed, inference_params=ip).logits[:, -1])
            ip.lengths_per_sample += 1
            ip.sequence_len_offset += 1
    return torch.stack([t.clone() for t in out]), ip
