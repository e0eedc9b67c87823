"""Attention modules -- API mirror of the reference's flash_attn/modules/mha.py for the serial
(non tensor-parallel) path: FlashSelfAttention / FlashCrossAttention (HIP kernel), their eager
twins SelfAttention / CrossAttention (the reference's own non-fused path, any device), and MHA.
ParallelMHA, rotary embeddings, dwconv and the Triton variants are out of scope."""
import math
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

import bp_hip
from flash_attn.flash_attn_interface import (flash_attn_unpadded_kvpacked_func,
                                             flash_attn_unpadded_qkvpacked_func)
from flash_attn.ops.fused_dense import FusedDense

_NEG = -10000.0  # additive mask value of the eager path (reference mha.py:212,219)


class FlashSelfAttention(nn.Module):
    """Fused softmax attention on packed qkv.  Reference: mha.py:34-100."""

    def __init__(self, causal=False, softmax_scale=None, attention_dropout=0.0, triton=False):
        super().__init__()
        assert not triton, 'the gfx950 build has no Triton path'
        self.causal = causal
        self.softmax_scale = softmax_scale
        self.dropout_p = attention_dropout
        self.triton = False

    def forward(self, qkv, causal=None, cu_seqlens=None, max_seqlen=None):
        """qkv (B,S,3,H,D) -> (B,S,H,D); or (total,3,H,D) + cu_seqlens int32 + max_seqlen
        -> (total,H,D)."""
        assert qkv.dtype in (torch.float16, torch.bfloat16)
        assert qkv.is_cuda
        causal = self.causal if causal is None else causal
        p_drop = self.dropout_p if self.training else 0.0
        if cu_seqlens is not None:
            assert cu_seqlens.dtype == torch.int32
            assert max_seqlen is not None and isinstance(max_seqlen, int)
            return flash_attn_unpadded_qkvpacked_func(qkv, cu_seqlens, max_seqlen, p_drop,
                                                      softmax_scale=self.softmax_scale, causal=causal)
        batch, seqlen = qkv.shape[0], qkv.shape[1]
        # fixed-length batch: cu_seqlens=None tells the C ABI that sequence b occupies rows [b*S, (b+1)*S)
        # (bp_flash_fwd / bp_flash_bwd, include/bp_hip.h) -- the reference builds an arange here on every
        # call (mha.py:91-94); no tensor means nothing a captured HIP graph could be left pointing at
        out = flash_attn_unpadded_qkvpacked_func(
            qkv.flatten(0, 1), None, seqlen, p_drop, softmax_scale=self.softmax_scale, causal=causal)
        return out.unflatten(0, (batch, seqlen))


class FlashCrossAttention(nn.Module):
    """Fused attention with separate q and packed kv.  Reference: mha.py:103-176."""

    def __init__(self, causal=False, softmax_scale=None, attention_dropout=0.0, triton=False):
        super().__init__()
        assert not triton, 'the gfx950 build has no Triton path'
        self.causal = causal
        self.softmax_scale = softmax_scale
        self.dropout_p = attention_dropout
        self.triton = False

    def forward(self, q, kv, causal=None, cu_seqlens=None, max_seqlen=None, cu_seqlens_k=None,
                max_seqlen_k=None):
        """q (B,Sq,H,D), kv (B,Sk,2,H,D); or the unpadded forms with both cu_seqlens."""
        assert q.dtype in (torch.float16, torch.bfloat16)
        assert q.is_cuda and kv.is_cuda
        causal = self.causal if causal is None else causal
        p_drop = self.dropout_p if self.training else 0.0
        if cu_seqlens is not None:
            assert cu_seqlens.dtype == torch.int32 and isinstance(max_seqlen, int)
            assert cu_seqlens_k is not None and cu_seqlens_k.dtype == torch.int32
            assert max_seqlen_k is not None
            return flash_attn_unpadded_kvpacked_func(q, kv, cu_seqlens, cu_seqlens_k, max_seqlen,
                                                     max_seqlen_k, p_drop,
                                                     softmax_scale=self.softmax_scale, causal=causal)
        batch, sq, sk = q.shape[0], q.shape[1], kv.shape[1]
        assert kv.shape[0] == batch and kv.shape[3] == q.shape[2] and kv.shape[4] == q.shape[3]
        out = flash_attn_unpadded_kvpacked_func(
            q.flatten(0, 1), kv.flatten(0, 1), None, None, sq, sk, p_drop,
            softmax_scale=self.softmax_scale, causal=causal)
        return out.unflatten(0, (batch, sq))


def _eager_attention(q, k, v, softmax_scale, causal, key_padding_mask, p_drop):
    """The reference's non-fused arithmetic, in its op order: scale K, additive -10000 masks,
    softmax in v.dtype (mha.py:206-224)."""
    scale = softmax_scale or 1.0 / math.sqrt(q.shape[-1])
    scores = torch.einsum('bthd,bshd->bhts', q, k * scale)
    if key_padding_mask is not None:
        pad = torch.full(key_padding_mask.shape, _NEG, dtype=scores.dtype, device=scores.device)
        pad.masked_fill_(key_padding_mask, 0.0)
        scores = scores + pad[:, None, None, :]
    if causal:
        sq, sk = scores.shape[-2], scores.shape[-1]
        mask = torch.triu(torch.full((sq, sk), _NEG, device=scores.device), 1)
        scores = scores + mask.to(dtype=scores.dtype)
    attn = torch.softmax(scores, dim=-1, dtype=v.dtype)
    attn = F.dropout(attn, p_drop)
    return torch.einsum('bhts,bshd->bthd', attn, v)


class SelfAttention(nn.Module):
    """Eager twin of FlashSelfAttention (any dtype, any device).  Reference: mha.py:179-224."""

    def __init__(self, causal=False, softmax_scale=None, attention_dropout=0.0):
        super().__init__()
        self.causal = causal
        self.softmax_scale = softmax_scale
        self.dropout_p = attention_dropout

    def forward(self, qkv, causal=None, key_padding_mask=None):
        causal = self.causal if causal is None else causal
        q, k, v = qkv.unbind(dim=2)
        return _eager_attention(q, k, v, self.softmax_scale, causal, key_padding_mask,
                                self.dropout_p if self.training else 0.0)


class CrossAttention(nn.Module):
    """Eager twin of FlashCrossAttention.  Reference: mha.py:227-276."""

    def __init__(self, causal=False, softmax_scale=None, attention_dropout=0.0):
        super().__init__()
        self.causal = causal
        self.softmax_scale = softmax_scale
        self.dropout_p = attention_dropout

    def forward(self, q, kv, causal=None, key_padding_mask=None):
        causal = self.causal if causal is None else causal
        assert kv.shape[0] == q.shape[0] and kv.shape[3] == q.shape[2] and kv.shape[4] == q.shape[3]
        k, v = kv.unbind(dim=2)
        return _eager_attention(q, k, v, self.softmax_scale, causal, key_padding_mask,
                                self.dropout_p if self.training else 0.0)


class LinearResidual(nn.Linear):
    """nn.Linear that also hands back its input (reference mha.py:279-284)."""

    def forward(self, input):
        return _linear_forward(self, input), input


def _linear_forward(layer, x):
    """nn.Linear.forward; without autograd through bp_hip.linear, the helper FusedDense uses as well (a pinned library
    solution for the few large shapes with one, F.linear otherwise)."""
    if torch.is_grad_enabled():
        return nn.Linear.forward(layer, x)
    return bp_hip.linear(x, layer.weight, layer.bias)


class _Linear(nn.Linear):
    """nn.Linear (same parameters and state-dict keys) whose inference forward goes through bp_hip.linear."""

    def forward(self, input):
        return _linear_forward(self, input)


class MHA(nn.Module):
    """Multi-head self attention: Wqkv -> inner attention -> out_proj.  Reference: mha.py:287-467.
    State-dict keys (`Wqkv.*`, `out_proj.*`) match the reference so its checkpoints load.
    Self-attention only; `use_flash_attn` picks the HIP kernel, otherwise the eager twin runs."""

    def __init__(self, embed_dim, num_heads, cross_attn=False, bias=True, dropout=0.0,
                 softmax_scale=None, causal=False, layer_idx=None, dwconv=False, rotary_emb_dim=0,
                 rotary_emb_scale_base=0, fused_bias_fc=False, use_flash_attn=False,
                 return_residual=False, checkpointing=False, device=None, dtype=None):
        factory_kwargs = {'device': device, 'dtype': dtype}
        super().__init__()
        if cross_attn or dwconv or rotary_emb_dim > 0:
            raise NotImplementedError('gfx950 build: MHA covers the Backpack/GPT-2 self-attention '
                                      'path only (no cross_attn / dwconv / rotary)')
        self.embed_dim = embed_dim
        self.cross_attn = False
        self.causal = causal
        self.layer_idx = layer_idx
        self.dwconv = False
        self.rotary_emb_dim = 0
        self.use_flash_attn = use_flash_attn
        self.return_residual = return_residual
        self.checkpointing = checkpointing
        self.num_heads = num_heads
        assert embed_dim % num_heads == 0, 'embed_dim must be divisible by num_heads'
        self.head_dim = embed_dim // num_heads
        # fused_bias_fc selects FusedDense, as upstream (mha.py:330-337): same parameters, bias gradient by bp_column_sum
        linear_cls = FusedDense if fused_bias_fc else _Linear
        if return_residual:
            qkv_cls = partial(FusedDense, return_residual=True) if fused_bias_fc else LinearResidual
        else:
            qkv_cls = linear_cls
        self.Wqkv = qkv_cls(embed_dim, 3 * embed_dim, bias=bias, **factory_kwargs)
        attn_cls = FlashSelfAttention if use_flash_attn else SelfAttention
        cross_cls = FlashCrossAttention if use_flash_attn else CrossAttention
        self.inner_attn = attn_cls(causal=causal, softmax_scale=softmax_scale, attention_dropout=dropout)
        self.inner_cross_attn = cross_cls(causal=causal, softmax_scale=softmax_scale,
                                          attention_dropout=dropout)
        self.out_proj = linear_cls(embed_dim, embed_dim, **factory_kwargs)

    def forward(self, x, x_kv=None, key_padding_mask=None, cu_seqlens=None, max_seqlen=None,
                inference_params=None, **kwargs):
        """x (batch, seqlen, hidden) or, with cu_seqlens/max_seqlen, (total, hidden)."""
        if inference_params is not None:
            assert key_padding_mask is None
            if cu_seqlens is not None or max_seqlen is not None:
                return self._forward_packed_prefill(x, inference_params, cu_seqlens, max_seqlen)
            return self._forward_cached(x, inference_params)
        if cu_seqlens is not None:
            assert max_seqlen is not None and key_padding_mask is None and self.use_flash_attn
        if key_padding_mask is not None:
            assert cu_seqlens is None and max_seqlen is None and not self.use_flash_attn
        if self.use_flash_attn:
            kwargs = {'cu_seqlens': cu_seqlens, 'max_seqlen': max_seqlen, **kwargs}
        else:
            kwargs = {'key_padding_mask': key_padding_mask, **kwargs}
        if self.return_residual:
            qkv, x = self.Wqkv(x)
        else:
            qkv = self.Wqkv(x)
        qkv = qkv.unflatten(-1, (3, self.num_heads, self.head_dim))
        if self.checkpointing:
            context = torch.utils.checkpoint.checkpoint(self.inner_attn, qkv, **kwargs)
        else:
            context = self.inner_attn(qkv, **kwargs)
        out = self.out_proj(context.flatten(-2))
        return out if not self.return_residual else (out, x)

    # ---- KV-cached generation: the reference's contract (mha.py:356-440, flash_attn/utils/generation.py:23-55) --------
    # key_value_memory_dict[layer_idx] is a (max_batch, max_seqlen, 2, nheads, head_dim) cache, created on first use.
    #   prefill (sequence_len_offset == 0, any length): causal attention over the prompt, its K/V written at [0, S)
    #   decode  (one new token per sample): the new K/V is written at position L_b and the token attends to [0, L_b];
    #           L_b = inference_params.lengths_per_sample[b] (device int32) when set, else sequence_len_offset for all.
    # The HIP path decodes with bp_flash_decode (append + attention in one call, no host read of the lengths); the eager
    # twin does the same bookkeeping in torch.  More than one new token at a non-zero offset is refused: the reference
    # runs that case without a causal mask among the new tokens.
    #   packed prefill (sequence_len_offset == 0, x (total, hidden) + cu_seqlens + max_seqlen; HIP path only): the ragged
    #           flash call over the packed prompts, their K/V scattered to [b, 0:len_b) by one bp_scatter_packed_rows launch
    #           that reads cu_seqlens on the device; positions at or behind len_b are not written.  A packed call at a
    #           non-zero offset is refused: cached steps stay one token per sample on (B, 1) inputs.

    def _kv_cache(self, inference_params, like):
        assert self.layer_idx is not None, 'generation requires layer_idx in the constructor'
        cache = inference_params.key_value_memory_dict.get(self.layer_idx)
        if cache is None:
            # zeros, not empty: the eager twin reads the whole (masked) cache, never garbage
            cache = torch.zeros(inference_params.max_batch_size, inference_params.max_sequence_len, 2, self.num_heads,
                                self.head_dim, dtype=like.dtype, device=like.device)
            inference_params.key_value_memory_dict[self.layer_idx] = cache
        return cache

    def _forward_cached(self, x, inference_params):
        if torch.is_grad_enabled() and (x.requires_grad or self.Wqkv.weight.requires_grad):
            raise RuntimeError('KV-cached decoding is inference-only: run it under torch.no_grad() or '
                               'torch.inference_mode()')
        if self.return_residual:
            qkv, x = self.Wqkv(x)
        else:
            qkv = self.Wqkv(x)
        qkv = qkv.unflatten(-1, (3, self.num_heads, self.head_dim))      # (B, S, 3, H, D)
        batch, seqlen = qkv.shape[:2]
        cache = self._kv_cache(inference_params, qkv)
        b0 = inference_params.batch_size_offset
        b1 = b0 + batch
        assert b1 <= cache.shape[0], 'batch_size_offset + batch exceeds max_batch_size'
        if inference_params.sequence_len_offset == 0:
            assert seqlen <= cache.shape[1], 'prompt longer than max_sequence_len'
            cache[b0:b1, :seqlen] = qkv[:, :, 1:]
            context = self.inner_attn(qkv)                                  # causal flash kernel / eager twin
        else:
            refuse_multi_token_step(seqlen, inference_params)
            lengths = cache_lengths(inference_params, batch, qkv.device)
            scale = self.inner_attn.softmax_scale or self.head_dim ** -0.5
            q, k_new, v_new = qkv[:, 0].unbind(dim=1)                       # (B, H, D) each
            if self.use_flash_attn:
                context = bp_hip.flash_decode(q, k_new, v_new, cache[b0:b1], lengths, scale).unsqueeze(1)
            else:
                context = _eager_decode(q, qkv[:, 0, 1:], cache, b0, lengths, scale).unsqueeze(1)
        out = self.out_proj(context.flatten(-2))
        return out if not self.return_residual else (out, x)

    def _forward_packed_prefill(self, x, inference_params, cu_seqlens, max_seqlen):
        """x (total, hidden): the prompts of a packed batch.  Their K/V go to [b, 0:len_b) of the cache rows of this call."""
        if torch.is_grad_enabled() and (x.requires_grad or self.Wqkv.weight.requires_grad):
            raise RuntimeError('KV-cached decoding is inference-only: run it under torch.no_grad() or '
                               'torch.inference_mode()')
        refuse_packed_step(inference_params)
        assert cu_seqlens is not None and max_seqlen is not None and x.dim() == 2 and self.use_flash_attn, \
            'a packed prefill takes x (total, hidden), cu_seqlens, max_seqlen and use_flash_attn=True'
        if self.return_residual:
            qkv, x = self.Wqkv(x)
        else:
            qkv = self.Wqkv(x)
        qkv = qkv.unflatten(-1, (3, self.num_heads, self.head_dim))      # (total, 3, H, D)
        batch = cu_seqlens.numel() - 1
        cache = self._kv_cache(inference_params, qkv)
        b0 = inference_params.batch_size_offset
        assert b0 + batch <= cache.shape[0], 'batch_size_offset + batch exceeds max_batch_size'
        assert max_seqlen <= cache.shape[1], 'prompt longer than max_sequence_len'
        bp_hip.scatter_packed_rows([(qkv[:, 1:], cache[b0:b0 + batch])], cu_seqlens, max_seqlen)
        context = self.inner_attn(qkv, cu_seqlens=cu_seqlens, max_seqlen=max_seqlen)   # the ragged causal flash call
        out = self.out_proj(context.flatten(-2))
        return out if not self.return_residual else (out, x)


def refuse_packed_step(inference_params):
    """A packed batch with `inference_params` is a PREFILL: after the prompt a cached call takes (B, 1) ids."""
    if inference_params.sequence_len_offset != 0:
        raise ValueError('a packed batch (cu_seqlens / max_seqlen) with inference_params is a prefill '
                         f'(sequence_len_offset == 0, got {inference_params.sequence_len_offset}): cached steps take one '
                         'token per sample as (B, 1) ids')


def cache_lengths(inference_params, batch, device):
    """(batch,) int32 cached positions of the samples of this call: `lengths_per_sample` (device) when the caller keeps
    per-sample lengths, else `sequence_len_offset` for every sample (the reference's contract)."""
    lengths = getattr(inference_params, 'lengths_per_sample', None)
    if lengths is not None:
        b0 = inference_params.batch_size_offset
        return lengths[b0:b0 + batch]
    return torch.full((batch,), inference_params.sequence_len_offset, dtype=torch.int32, device=device)


def refuse_multi_token_step(seqlen, inference_params):
    """After the prompt (`sequence_len_offset` > 0) a cached call takes ONE new token per sample: MHA's contract above."""
    if inference_params.sequence_len_offset != 0 and seqlen != 1:
        raise NotImplementedError(
            f'KV-cached decoding takes one new token per sample after the prompt (got {seqlen} at offset '
            f'{inference_params.sequence_len_offset}); feed multi-token continuations one token at a time')


def _eager_decode(q, kv_new, cache, b0, lengths, scale):
    """Eager twin of bp_flash_decode: append kv_new (B, 2, H, D) at row lengths[b], attend to rows [0, lengths[b]]
    (reference op order: scale K, softmax in v.dtype)."""
    batch = q.shape[0]
    rows = torch.arange(b0, b0 + batch, device=q.device)
    cache[rows, lengths.long()] = kv_new
    k, v = cache[b0:b0 + batch].unbind(dim=2)                              # (B, M, H, D)
    scores = torch.einsum('bhd,bshd->bhs', q, k * scale)
    visible = torch.arange(cache.shape[1], device=q.device)[None, :] <= lengths[:, None].long()
    scores = scores.masked_fill(~visible[:, None, :], float('-inf'))
    attn = torch.softmax(scores, dim=-1, dtype=v.dtype)
    return torch.einsum('bhs,bshd->bhd', attn, v)
