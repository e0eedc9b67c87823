"""Packed (variable-length) batches: the sequences of a batch behind one another without padding, described by
`cu_seqlens` -- the form BackpackModel.forward / GPTModel.forward take as `input_ids (total,)` + `cu_seqlens` + `max_seqlen`
and the ragged kernels read (bp_flash_fwd, bp_sense_*_varlen).

This module is the ONE place that reads lengths on the host and checks them: the kernels never validate `cu_seqlens`
(include/bp_hip.h), so what is built here is non-decreasing, starts at 0 and holds no length beyond `max_seqlen`.
"""
import torch
import torch.nn.functional as F

from flash_attn.bert_padding import index_first_axis
from flash_attn.models.gpt import packed_coordinates, packed_position_ids  # noqa: F401  (re-exported: device-side, no host read)


def _checked_lengths(lengths, longest=None):
    lengths = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
    if not lengths:
        raise ValueError('pack_sequences: an empty batch')
    if min(lengths) < 0:
        raise ValueError(f'pack_sequences: negative length {min(lengths)}')
    if longest is not None and max(lengths) > longest:
        raise ValueError(f'pack_sequences: length {max(lengths)} exceeds the padded width {longest}')
    if sum(lengths) == 0:
        raise ValueError('pack_sequences: no tokens (every length is 0)')
    if sum(lengths) >= 2 ** 31:
        raise ValueError('pack_sequences: 2^31 or more tokens (cu_seqlens is int32)')
    return lengths


def pack_sequences(sequences, lengths=None, device=None):
    """-> (ids (total,) int64, cu_seqlens (B + 1,) int32, max_seqlen int), all on one device.

    sequences: a list of id sequences (lists or 1-D tensors; an empty one is a legal zero-length sample), or, with
    `lengths` (B,), right-padded ids (B, S) whose row b holds lengths[b] tokens.  `device` defaults to the ids' own (CPU for
    lists).  Raises ValueError for an empty batch, a batch without tokens, negative lengths, lengths beyond S."""
    if lengths is not None:
        if not torch.is_tensor(sequences) or sequences.dim() != 2:
            raise ValueError('pack_sequences: with lengths, the ids must be a (B, S) tensor')
        batch, width = sequences.shape
        lens = _checked_lengths(lengths, width)
        if len(lens) != batch:
            raise ValueError(f'pack_sequences: {len(lens)} lengths for {batch} rows')
        device = sequences.device if device is None else device
        lens_t = torch.tensor(lens, dtype=torch.int64, device=sequences.device)
        keep = torch.arange(width, device=sequences.device)[None, :] < lens_t[:, None]
        ids = index_first_axis(sequences.reshape(-1), keep.reshape(-1).nonzero().squeeze(1)).to(torch.int64)
    else:
        if torch.is_tensor(sequences):
            raise ValueError('pack_sequences: padded ids need their lengths')
        rows = [s.reshape(-1).to(torch.int64) if torch.is_tensor(s) else torch.tensor(list(map(int, s)), dtype=torch.int64)
                for s in sequences]
        lens = _checked_lengths([r.numel() for r in rows])
        if device is None:
            device = next((s.device for s in sequences if torch.is_tensor(s)), torch.device('cpu'))
        ids = torch.cat([r.to(device) for r in rows])
    cu = F.pad(torch.cumsum(torch.tensor(lens, dtype=torch.int64), 0), (1, 0)).to(torch.int32)
    return ids.to(device), cu.to(device), max(lens)


def unpack_rows(values, cu_seqlens, max_seqlen, fill=0):
    """values (total, ...) of a packed batch -> (B, max_seqlen, ...): row b holds its sequence's rows, `fill` behind them.
    The inverse of pack_sequences for per-token values (hidden states, logits, scores)."""
    if cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2:
        raise ValueError('unpack_rows: cu_seqlens must be (B + 1,)')
    batch, width = cu_seqlens.numel() - 1, int(max_seqlen)
    cu = cu_seqlens.to(device=values.device, dtype=torch.int64)
    if int(cu[-1]) != values.shape[0]:
        raise ValueError(f'unpack_rows: cu_seqlens ends at {int(cu[-1])}, values hold {values.shape[0]} rows')
    if int((cu[1:] - cu[:-1]).max()) > width:
        raise ValueError(f'unpack_rows: a sequence is longer than max_seqlen = {width}')
    return pad_rows(values, cu, width, fill)


def pad_rows(values, cu_seqlens, max_seqlen, fill=0):
    """unpack_rows without its checks and without a host read: for cu_seqlens that pack_sequences built."""
    sample, position = packed_coordinates(cu_seqlens.to(values.device), values.shape[0])
    out = values.new_full((cu_seqlens.numel() - 1, int(max_seqlen)) + tuple(values.shape[1:]), fill)
    out[sample, position] = values
    return out
