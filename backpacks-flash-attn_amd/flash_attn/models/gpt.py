"""GPT-2 trunk -- mirror of the reference's flash_attn/models/gpt.py for the serial path:
`create_mixer_cls` (:44-69, incl. the 1/(layer_idx+1) softmax scale), `create_mlp_cls` (:72-108),
`create_block` (:111-122), `GPTModel` (:175-246), `GPTLMHeadModel` (:249-282).
Linear layers / LayerNorm / embeddings are torch ops on ROCm (hipBLASLt); every layer's attention
is one launch of the HIP flash kernel when `config.use_flash_attn` is set."""
import math
from collections import namedtuple
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F
from transformers import GPT2Config

import bp_hip
from flash_attn.modules.block import Block
from flash_attn.modules.embedding import GPT2Embeddings
from flash_attn.modules.mha import MHA, cache_lengths, refuse_packed_step
from flash_attn.modules.mlp import FusedDenseGeluDense, Mlp
from flash_attn.ops.layer_norm import dropout_add_layer_norm
from flash_attn.utils.pretrained import state_dict_from_pretrained
from flash_attn.utils.hf_convert import gpt2_trunk_state_dict, remap_state_dict_gpt2


def create_mixer_cls(config, layer_idx=None, process_group=None, device=None, dtype=None):
    assert process_group is None, 'tensor parallelism is out of scope for the Backpack path'
    head_dim = getattr(config, 'head_dim', config.hidden_size // config.num_attention_heads)
    softmax_scale = 1.0 if not config.scale_attn_weights else head_dim ** (-0.5)
    if config.scale_attn_by_inverse_layer_idx:
        assert layer_idx is not None
        softmax_scale /= float(layer_idx + 1)
    return partial(MHA, num_heads=config.num_attention_heads, dropout=config.attn_pdrop,
                   softmax_scale=softmax_scale, causal=True, layer_idx=layer_idx,
                   use_flash_attn=getattr(config, 'use_flash_attn', False),
                   fused_bias_fc=getattr(config, 'fused_bias_fc', False),
                   device=device, dtype=dtype)


def _activation(config):
    assert config.activation_function in ('gelu', 'gelu_new', 'gelu_fast')
    approximate = 'tanh' if config.activation_function in ('gelu_new', 'gelu_fast') else 'none'
    return partial(F.gelu, approximate=approximate)


def create_mlp_cls(config, layer_idx=None, process_group=None, device=None, dtype=None):
    assert process_group is None
    inner_dim = config.n_inner if config.n_inner is not None else 4 * config.hidden_size
    if getattr(config, 'fused_dense_gelu_dense', False):
        assert config.activation_function in ('gelu_new', 'gelu_fast'), \
            'fused_dense_gelu_dense only supports approximate gelu'          # reference gpt.py:75-78
        return partial(FusedDenseGeluDense, hidden_features=inner_dim, device=device, dtype=dtype)
    return partial(Mlp, hidden_features=inner_dim, activation=_activation(config), device=device,
                   dtype=dtype)


def create_block(config, layer_idx=None, process_group=None, device=None, dtype=None):
    mixer_cls = create_mixer_cls(config, layer_idx, process_group=process_group, device=device, dtype=dtype)
    mlp_cls = create_mlp_cls(config, layer_idx, process_group=process_group, device=device, dtype=dtype)
    norm_cls = partial(nn.LayerNorm, eps=config.layer_norm_epsilon, device=device, dtype=dtype)
    block = Block(config.hidden_size, mixer_cls, mlp_cls, norm_cls=norm_cls, prenorm=True,
                  resid_dropout=config.resid_pdrop,
                  fused_dropout_add_ln=getattr(config, 'fused_dropout_add_ln', False))
    block.layer_idx = layer_idx
    return block


def _init_weights(module, n_layer, initializer_range=0.02, rescale_prenorm_residual=True):
    """GPT-2 initialisation (reference gpt.py:153-172): N(0, std) for Linear / Embedding weights,
    zero biases, and N(0, std / sqrt(2 * n_layer)) for the projections that write into the
    residual stream (out_proj, fc2)."""
    if isinstance(module, nn.Linear):
        nn.init.normal_(module.weight, std=initializer_range)
        if module.bias is not None:
            nn.init.zeros_(module.bias)
    elif isinstance(module, nn.Embedding):
        nn.init.normal_(module.weight, std=initializer_range)
    if rescale_prenorm_residual:
        for name, p in module.named_parameters():
            if name in ('out_proj.weight', 'fc2.weight'):
                nn.init.normal_(p, mean=0.0, std=initializer_range / math.sqrt(2 * n_layer))


def _pad_vocab(config):
    multiple = getattr(config, 'pad_vocab_size_multiple', 1)
    if not hasattr(config, 'unpadded_vocab_size'):
        config.unpadded_vocab_size = config.vocab_size   # the tokenizer's size: the embedding rows from here on are no words
    if config.vocab_size % multiple != 0:
        config.vocab_size += multiple - config.vocab_size % multiple
    return multiple


class GPTPreTrainedModel(nn.Module):

    def __init__(self, config, *inputs, **kwargs):
        super().__init__()
        if not isinstance(config, GPT2Config):
            raise ValueError('config must be a transformers.GPT2Config, got %r' % type(config))
        self.config = config

    @classmethod
    def from_pretrained(cls, model_name, config, *inputs, state_dict=None, **kwargs):
        """Build the model and load Hugging Face GPT-2 weights into it (reference gpt.py:140-151).
        `state_dict`: an already loaded HF state dict (skips the lookup of `model_name`).  A `GPTLMHeadModel`
        takes the remapped dict as it is; a bare `GPTModel` takes it without the `transformer.` prefix and
        the head (upstream's strict load only works for the former)."""
        model = cls(config, *inputs, **kwargs)
        hf = state_dict if state_dict is not None else state_dict_from_pretrained(model_name)
        if hasattr(model, 'lm_head'):
            hf = {(k[len('transformer.'):] if k.startswith('transformer.') else k): v for k, v in hf.items()
                  if k != 'lm_head.weight'}
            model.load_state_dict(remap_state_dict_gpt2(hf, config))
            model.tie_weights()
        else:
            model.load_state_dict(gpt2_trunk_state_dict(hf, config))
        return model


def packed_coordinates(cu_seqlens, total):
    """(sample, position), two (total,) int64 tensors: the sequence every row of a packed batch belongs to and its position
    inside it, computed on cu_seqlens' device without a host read.  Row t belongs to the sample b with
    cu[b] <= t < cu[b + 1], i.e. b = #{entries of cu[1:] <= t} (empty samples repeat an entry and own no row)."""
    cu = cu_seqlens.long()
    rows = torch.arange(total, device=cu.device)
    sample = torch.bucketize(rows, cu[1:], right=True).clamp_(max=cu.numel() - 2)
    return sample, rows - cu[sample]


def packed_position_ids(cu_seqlens, total):
    """Default position ids of a packed batch: they restart at 0 in every sequence."""
    return packed_coordinates(cu_seqlens, total)[1]


class GPTModel(GPTPreTrainedModel):
    """embeddings -> fp32 residual stream -> ln_0 -> n_layer pre-norm blocks.  gpt.py:175-246."""

    def __init__(self, config: GPT2Config, process_group=None, device=None, dtype=None):
        super().__init__(config)
        assert process_group is None, 'tensor parallelism is out of scope for the Backpack path'
        factory_kwargs = {'device': device, 'dtype': dtype}
        self.process_group = None
        self.pad_vocab_size_multiple = _pad_vocab(config)
        self.embeddings = GPT2Embeddings(config.hidden_size, config.vocab_size,
                                         config.max_position_embeddings, **factory_kwargs)
        self.emb_drop = nn.Dropout(config.embd_pdrop)
        self.fused_dropout_add_ln = getattr(config, 'fused_dropout_add_ln', False)
        self.ln_0 = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_epsilon, **factory_kwargs)
        self.layers = nn.ModuleList([create_block(config, layer_idx=i, **factory_kwargs)
                                     for i in range(config.num_hidden_layers)])
        self.apply(partial(_init_weights, n_layer=config.num_hidden_layers,
                           initializer_range=config.initializer_range))

    # Inference forwards take the chained add + LayerNorm launches (`_forward_chained`); False: always the launches of
    # `forward` below.  Same bits either way (tests/test_gpu_ln_chain.py compares the two in one process).
    ln_chain = True

    def _chain_applies(self, input_ids, inference_params):
        if not self.ln_chain or self.training or torch.is_grad_enabled() or inference_params is not None:
            return False
        if not self.fused_dropout_add_ln or not input_ids.is_cuda or input_ids.dtype != torch.int64 \
                or torch.is_autocast_enabled():
            return False
        word = self.embeddings.word_embeddings
        if word.weight.dtype not in (torch.float16, torch.bfloat16) or word.max_norm is not None:
            return False
        return all(type(layer) is Block and layer.chain_supported() for layer in self.layers)

    def _forward_chained(self, input_ids, position_ids):
        """The forward of eval() without an autograd graph, 16-bit activations and an fp32 residual stream: the embedding
        lookup happens inside ln_0's launch and again inside the first block's norm1 (no embedding tensor, no fp32 copy of
        it), every norm2 stores z alone and the following norm1 settles the residual in place (Block._forward_chained),
        and the last norm stores no residual at all.  Only launches are rearranged; every sum keeps its order."""
        emb = self.embeddings
        input_ids = input_ids.contiguous()
        pos_table = emb.position_embeddings.weight if emb.max_position_embeddings > 0 else None
        if pos_table is not None and position_ids is not None:
            position_ids = position_ids.expand_as(input_ids).contiguous() \
                if position_ids.shape[-1] != input_ids.shape[-1] else position_ids.contiguous()
        source = (input_ids, position_ids if pos_table is not None else None, emb.word_embeddings.weight, pos_table)
        hidden = bp_hip.add_layer_norm(None, None, self.ln_0.weight, self.ln_0.bias, self.ln_0.eps,
                                       return_residual=False, embedding=source)
        residual = pending = None
        for i, layer in enumerate(self.layers):
            hidden, residual, pending = layer._forward_chained(hidden, residual, pending,
                                                               embedding=source if i == 0 else None)
        return hidden

    def forward(self, input_ids, position_ids=None, inference_params=None, cu_seqlens=None, max_seqlen=None):
        """`inference_params` (src/utils/generation.py InferenceParams): KV-cached generation, forwarded to every mixer
        (reference gpt.py:243).  In a decode step without `position_ids` the position of sample b is its cached length,
        read on the device.
        `cu_seqlens` ((B + 1,) int32) + `max_seqlen` (int): a PACKED batch, `input_ids` (total,) -> (total, d); every mixer
        receives the two (MHA.forward's ragged form), default positions restart at 0 in every sequence."""
        if cu_seqlens is not None or max_seqlen is not None:
            return self._forward_packed(input_ids, position_ids, inference_params, cu_seqlens, max_seqlen)
        if self._chain_applies(input_ids, inference_params):
            return self._forward_chained(input_ids, position_ids)
        if inference_params is not None and position_ids is None and inference_params.sequence_len_offset > 0:
            lengths = cache_lengths(inference_params, input_ids.shape[0], input_ids.device)
            position_ids = lengths.long().unsqueeze(1) + torch.arange(input_ids.shape[1], device=input_ids.device)
        mixer_kwargs = None if inference_params is None else {'inference_params': inference_params}
        return self._embed_and_run(input_ids, position_ids, mixer_kwargs)

    def _forward_packed(self, input_ids, position_ids, inference_params, cu_seqlens, max_seqlen):
        """The packed form of `forward`: the unchained launches over (total, d) rows (every row-wise kernel takes any
        number of rows), attention through the ragged flash call.  HIP trunk only: the eager attention has no ragged form
        (BackpackModel pads such batches).
        With `inference_params` at sequence_len_offset == 0 it is the PACKED PREFILL: every mixer also scatters its K/V into
        the rows of its cache (MHA._forward_packed_prefill).  At a non-zero offset it stays refused: cached steps take one
        token per sample as (B, 1) ids."""
        if inference_params is not None:
            refuse_packed_step(inference_params)
        if cu_seqlens is None or max_seqlen is None or input_ids.dim() != 1:
            raise ValueError('a packed batch needs input_ids (total,), cu_seqlens (B + 1,) int32 and max_seqlen (int)')
        if not getattr(self.config, 'use_flash_attn', False):
            if inference_params is not None:
                raise ValueError('a packed batch with inference_params (a packed prefill) needs use_flash_attn=True: the '
                                 'eager attention has no ragged form')
            raise NotImplementedError('a packed batch needs use_flash_attn=True: the eager attention has no ragged form')
        if position_ids is None:
            position_ids = packed_position_ids(cu_seqlens, input_ids.shape[0])
        mixer_kwargs = {'cu_seqlens': cu_seqlens, 'max_seqlen': int(max_seqlen)}
        if inference_params is not None:
            mixer_kwargs['inference_params'] = inference_params
        return self._embed_and_run(input_ids, position_ids, mixer_kwargs)

    def _embed_and_run(self, input_ids, position_ids, mixer_kwargs):
        hidden = self.embeddings(input_ids, position_ids=position_ids)
        if self.fused_dropout_add_ln:
            # one HIP launch: residual (fp32) = hidden, hidden = LN(residual)   (reference gpt.py:236-240)
            hidden, residual = dropout_add_layer_norm(
                hidden, None, self.ln_0.weight, self.ln_0.bias,
                self.emb_drop.p if self.training else 0.0, self.ln_0.eps, prenorm=True,
                residual_in_fp32=True)
        else:
            residual = self.emb_drop(hidden).float()   # residual stream stays fp32 (gpt.py:231-234)
            hidden = self.ln_0(residual.to(dtype=self.ln_0.weight.dtype))
        for layer in self.layers:
            hidden, residual = layer(hidden, residual, mixer_kwargs=mixer_kwargs)
        return hidden


class GPTLMHeadModel(GPTPreTrainedModel):
    """GPTModel + tied LM head.  gpt.py:249-282."""

    def __init__(self, config: GPT2Config, process_group=None, device=None, dtype=None):
        super().__init__(config)
        self.process_group = None
        self.transformer = GPTModel(config, device=device, dtype=dtype)
        self.lm_head = nn.Linear(config.n_embd, config.vocab_size, bias=False, device=device, dtype=dtype)
        self.apply(partial(_init_weights, n_layer=config.num_hidden_layers,
                           initializer_range=config.initializer_range))
        self.tie_weights()

    def tie_weights(self):
        self.lm_head.weight = self.transformer.embeddings.word_embeddings.weight

    def forward(self, input_ids, position_ids=None, inference_params=None):
        hidden = self.transformer(input_ids, position_ids=position_ids, inference_params=inference_params)
        CausalLMOutput = namedtuple('CausalLMOutput', ['logits'])
        return CausalLMOutput(logits=self.lm_head(hidden))
