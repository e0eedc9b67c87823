"""Control experiments on a trained Backpack -- MI355X-native mirror of the reference's
training/src/models/intervened_models.py (same public names and constructor arguments:
create_content_soft_mask :9-20, get_sense_vector_of_word :23-26, mask_annealing :29-53,
WeightedBackpackLMHeadModel :58-105, NegativeWeightedBackpackLMHeadModel :108-165,
ReplacedWordLMHeadModel :168-199).

All three models change what enters the sense contraction `sum_l alpha_l @ C_l`.  The reference redoes
that contraction in eager ops on a materialised alpha (B,k,S,S) and an edited copy of the content; here,
when the wrapped network runs its HIP path (`config.use_flash_attn`), it stays ONE fused launch:
  * per-(token, sense) weights go in as `key_weight` (C ABI bp_sense_mix_weighted) -- no weighted copy of
    the 25 MB/sample content tensor, no alpha;
  * vocabulary-sized "content logits" use the same kernel with d_out = vocab;
  * the similarity term of the annealing only needs the logits of the tokens that occur in the sequence,
    so it is a (S x S) product per sense against the gathered embeddings instead of a gather out of a
    (B,k,S,vocab) tensor (identical numbers, 50264/S times less work and memory).
With `use_flash_attn=False` the reference's eager op sequence runs (any device / dtype).

KV-cached decoding (`forward(..., inference_params=ip)`, `generate` / `sample` with `kv_cache=True`): the wrappers are the
`SenseIntervention` of `BackpackModel`'s cached path.  Weighted: the per-(sense, position) weights of the cached positions
live in `ip.key_value_memory_dict` and enter the step as `key_weight` of bp_sense_decode_weighted; the annealed weights
change at every step, but the similarity sums behind them are running sums, advanced by one gathered GEMV over the cached
rows (bp_sense_rows_dot).  ReplacedWord: cache form, the listed tokens' rows are replaced as they are appended.
State, all (max_batch_size, ..., max_sequence_len), indexed on the device through the cached lengths:
  'intervened_ids'     int64 token ids of the cached positions
  'intervened_weight'  fp32 (., k, .) the key weights the contraction reads
  'intervened_sims'    fp32 (., k, .) annealed: sum_j relu(C_l(x_i) . E[x_j]) over the tokens so far
  'intervened_dots'    fp32 (., k, .) annealed: the step's dot products (bp_sense_rows_dot's output)
  'intervened_content_weights' / 'intervened_replace'   device copies of content_weights / sense_dict, made by the prefill
"""
from collections import namedtuple

import torch
from torch import nn

import bp_hip
from src.models.backpack import SenseIntervention
from src.utils.generation import GenerationMixin

CausalLMOutput = namedtuple('CausalLMOutput', ['logits'])


def create_content_soft_mask(content_weights, input_ids, scores):
    """content_weights (vocab, k), input_ids (B,S), scores (B,S,k) -> weights (B,S,k) =
    w[token] * score + (1 - score)   (reference :9-20)."""
    picked = content_weights.to(scores.device)[input_ids]
    return picked * scores + (1 - scores)


def get_sense_vector_of_word(word_id, model, sense_index):
    """Sense vector `sense_index` of token `word_id` (reference :23-26; a sense vector does not depend on
    the context, so one position is enough -- the reference fills a whole n_positions row)."""
    ids = torch.as_tensor(word_id, device=model.lm_head.weight.device).reshape(1, 1).long()
    senses = model.transformer.content_model(ids)          # (1, k, 1, d)
    return senses[0, sense_index, 0, :]


def mask_annealing(model, input_ids, target_vector, content, annealing_scale=0.1, upweight_nearby=True):
    """scores (B,k,S) = sigmoid(-scale * sum_j relu(content[b,l,i] . E[ids[b,j]]) + 6) [* (1 + i/100)]
    (reference :29-53; `target_vector` is unused there as well)."""
    seqlen = input_ids.shape[1]
    emb = model.lm_head.weight[input_ids]                                      # (B, S, d)
    sims = torch.relu(content @ emb.transpose(1, 2).unsqueeze(1)).sum(dim=3)   # (B,k,S,d)@(B,1,d,S) -> sum_j
    scores = torch.sigmoid(-annealing_scale * sims + 6)
    if upweight_nearby:
        scores = scores * (1 + torch.arange(seqlen, device=scores.device) / 100).reshape(1, 1, seqlen)
    return scores


def _anneal_weights(sims, picked, annealing_scale, upweight_nearby, first_position=0):
    """sims (B,k,n) fp32 similarity sums, picked (B,k,n) content_weights of the tokens -> (B,k,n) fp32 weights
    (mask_annealing's score + create_content_soft_mask; position i of the last axis is first_position + i)."""
    scores = torch.sigmoid(-annealing_scale * sims + 6)
    if upweight_nearby:
        scores = scores * (1 + torch.arange(first_position, first_position + sims.shape[2], device=sims.device) / 100)
    return picked * scores + (1 - scores)


def _refuse_packed(model, cu_seqlens, max_seqlen):
    """Packed batches (BackpackModel.forward's cu_seqlens / max_seqlen) stop at the wrappers: their edits -- per-position
    weights, replaced rows, key weights -- are written for (B, S) ids, and the packed mix kernels have no weighted form."""
    if cu_seqlens is not None or max_seqlen is not None:
        raise NotImplementedError(f'{type(model).__name__} takes no packed batch (cu_seqlens / max_seqlen): pad the '
                                  'sequences to (B, S), or score the wrapped network')


class _Intervened(nn.Module, GenerationMixin, SenseIntervention):
    """Shared plumbing: the three stages of the wrapped network, the contraction, and where a call goes -- with
    `inference_params` to the cached path of the wrapped BackpackModel (its hook: this wrapper), else to `_mixed`."""

    def forward(self, input_ids, position_ids=None, inference_params=None, cu_seqlens=None, max_seqlen=None):
        _refuse_packed(self, cu_seqlens, max_seqlen)
        cached = self.backpack_network.transformer._forward_cached
        mixed = self._mixed(input_ids, position_ids) if inference_params is None else \
            cached(input_ids, position_ids, inference_params, intervention=self)
        return CausalLMOutput(logits=self.backpack_network.lm_head(mixed))

    def _packed(self, packed_prefill):
        if packed_prefill:
            raise NotImplementedError(f'packed_prefill=True is not available on {type(self).__name__}: the edits of the '
                                      'sense-intervened wrappers are written for (B, S) ids (see _refuse_packed)')
        return super()._packed(packed_prefill)

    def beam_search(self, *args, **kwargs):
        # the mixin's beam search reorders the wrapped network's caches between slots, not the wrapper's own per-row
        # state (ids, sims, dots, weights)
        raise NotImplementedError('beam_search is not available on the sense-intervened wrappers: their per-row cache '
                                  'state is not reordered between beam slots')

    def _stages(self, input_ids, position_ids):
        t = self.backpack_network.transformer
        hidden = t.gpt2_model(input_ids, position_ids=position_ids, inference_params=None)
        content = t.content_model(input_ids, position_ids, None)                  # (B,k,S,d) view
        return t, hidden, content

    @staticmethod
    def _mix(t, hidden, content, key_weight=None):
        """sum_l (alpha_l * key_weight_l) @ content_l; content (B,k,S,d_out), key_weight (B,k,S) or None."""
        attn = t.contextualization_attn
        if t.fused_senses:
            return bp_hip.sense_mix(attn.project(hidden), content.transpose(1, 2), attn.scale(),
                                    key_weight=key_weight)
        alpha = attn(hidden)                                                      # (B,k,S,S)
        if key_weight is not None:
            content = content * key_weight.unsqueeze(3).to(content.dtype)
        return torch.sum(alpha @ content, dim=1)

    def _weights(self, input_ids, content):
        """(B,k,S) per-token, per-sense weights of the soft mask (reference :83-99)."""
        if self.anneal:
            scores = mask_annealing(self.backpack_network, input_ids, self.target_weight, content,
                                    self.annealing_scale, self.upweight_nearby).transpose(1, 2)
        else:
            b, k, s, _ = content.shape
            scores = torch.ones(b, s, k, device=content.device)
        return create_content_soft_mask(self.content_weights, input_ids, scores.float()).transpose(1, 2)


class WeightedBackpackLMHeadModel(_Intervened):
    """Sense vectors re-weighted per (token, sense) before the contraction (reference :58-105).
    Generation from right-padded prompts of different lengths (`prompt_lengths`) is taken without annealing, where a
    position's weight depends on its own token alone.  The annealed form raises NotImplementedError: its similarity sums
    run over every position of the prefilled width, so they would count the pad columns behind a shorter prompt."""

    def __init__(self, backpack_network, content_weights, target_weight, annealing_scale, anneal=True,
                 upweight_nearby=True):
        super().__init__()
        self.backpack_network = backpack_network
        self.content_weights = content_weights          # (vocab, k)
        self.target_weight = target_weight
        self.annealing_scale = annealing_scale
        self.anneal = anneal
        self.upweight_nearby = upweight_nearby

    def _ragged(self, prompt_lengths):
        if prompt_lengths is not None and self.anneal:
            raise NotImplementedError('prompt_lengths is not available with annealing: the similarity sums of the prefill '
                                      'would count the pad columns behind a shorter prompt')
        return super()._ragged(prompt_lengths)

    def _mixed(self, input_ids, position_ids):
        t, hidden, content = self._stages(input_ids, position_ids)
        return self._mix(t, hidden, content, self._weights(input_ids, content))

    # ---- KV-cached decoding ----
    def _cached_state(self, ip, k=None, device=None):
        """The wrapper's (ids, weight, sims, dots, content_weights) of `key_value_memory_dict`; given `k`: made by the prefill."""
        caches = ip.key_value_memory_dict
        if k is not None:
            mb, ms = ip.max_batch_size, ip.max_sequence_len
            state = {'intervened_ids': ((mb, ms), torch.long), 'intervened_weight': ((mb, k, ms), torch.float32)}
            if self.anneal:
                state.update(intervened_sims=((mb, k, ms), torch.float32), intervened_dots=((mb, k, ms), torch.float32))
            for name, (shape, dtype) in state.items():
                if name not in caches:
                    caches[name] = torch.zeros(shape, dtype=dtype, device=device)
            # one device copy of the (vocab, k) weights per prefill: the steps index it without touching the host
            caches['intervened_content_weights'] = self.content_weights.to(device=device, dtype=torch.float32)
        return tuple(caches.get('intervened_' + name) for name in ('ids', 'weight', 'sims', 'dots', 'content_weights'))

    def prefill_key_weight(self, model, input_ids, content, ip):
        batch, seqlen = input_ids.shape
        b0 = ip.batch_size_offset
        ids, weight, sims_state, _, cw = self._cached_state(ip, content.shape[1], input_ids.device)
        ids[b0:b0 + batch, :seqlen] = input_ids
        picked = cw[input_ids].transpose(1, 2)                                     # (B,k,S)
        if self.anneal:
            emb = self.backpack_network.lm_head.weight[input_ids]                  # (B,S,d)
            sims = torch.relu(content @ emb.transpose(1, 2).unsqueeze(1)).sum(dim=3, dtype=torch.float32)
            sims_state[b0:b0 + batch, :, :seqlen] = sims
            picked = _anneal_weights(sims, picked, self.annealing_scale, self.upweight_nearby)
        weight[b0:b0 + batch, :, :seqlen] = picked
        return picked.contiguous()

    def step_key_weight(self, model, input_ids, table, rows, new_row, lengths, ip):
        batch = input_ids.shape[0]
        b0, ms = ip.batch_size_offset, ip.max_sequence_len
        ids, weight, sims, dots, cw = self._cached_state(ip)
        sample = torch.arange(b0, b0 + batch, device=input_ids.device)
        at = lengths.long()
        ids[sample, at] = input_ids[:, 0]
        if not self.anneal:
            weight[sample, :, at] = cw[input_ids[:, 0]]                            # fixed once appended
            return weight[b0:b0 + batch]
        # sims[b,l,i] += relu(C_l(x_i) . E[x_L]) for the cached i < L, and the new position's own sum over all tokens; the
        # pair (L, L) comes once, out of the rows-dot (its row is new_row).  Fixed shapes over max_sequence_len masked by
        # the device lengths: a captured step is valid for every later step.
        emb_w = self.backpack_network.lm_head.weight
        sims, dots = sims[b0:b0 + batch], dots[b0:b0 + batch]
        vec = emb_w[input_ids[:, 0]]                                               # (B,d) = E[x_L]
        pos = torch.arange(ms, device=input_ids.device)
        cached, new = pos[None, :] < at[:, None], pos[None, :] == at[:, None]      # (B,ms)
        if model.fused_senses:
            if not bp_hip.sense_rows_dot_supported(table, vec):
                raise RuntimeError(f'Backpack decode: bp_sense_rows_dot does not take {table.shape[1]} senses with '
                                   f'{table.shape[2]} output columns (include/bp_hip.h)')
            bp_hip.sense_rows_dot(table, rows, new_row, lengths, vec, dots)
        else:
            dots.copy_(_eager_rows_dot(table, rows, new_row, lengths, vec))
        own = torch.einsum('bld,bjd->blj', table[new_row.long()], emb_w[ids[b0:b0 + batch]])   # (B,k,ms)
        own = torch.where(cached[:, None, :], torch.relu(own).float(), 0.0).sum(dim=2, keepdim=True)
        hit = torch.relu(dots)
        sims.copy_(torch.where(cached[:, None, :], sims + hit, torch.where(new[:, None, :], own + hit, sims)))
        picked = cw[ids[b0:b0 + batch]].transpose(1, 2)                            # (B,k,ms)
        weight[b0:b0 + batch] = _anneal_weights(sims, picked, self.annealing_scale, self.upweight_nearby)
        return weight[b0:b0 + batch]


def _eager_rows_dot(table, rows, new_row, lengths, vec):
    """Eager restatement of bp_sense_rows_dot over the whole row index: (B,k,max_seqlen) fp32 = table[row(b,j), l] . vec[b]
    in the tensors' dtype, position lengths[b] taking new_row[b]; entries past it carry no meaning."""
    pos = torch.arange(rows.shape[1], device=rows.device)
    index = torch.where(pos[None, :] == lengths[:, None].long(), new_row[:, None].long(), rows.long())
    index = index.clamp(0, table.shape[0] - 1)
    return torch.einsum('bjld,bd->blj', table[index], vec).float()


class NegativeWeightedBackpackLMHeadModel(WeightedBackpackLMHeadModel):
    """Per (sense, position) the 2 % most negative re-weighted vocabulary logits replace the plain ones,
    then the contraction runs on vocabulary-sized content (reference :108-165)."""

    def forward(self, input_ids, position_ids=None, inference_params=None, cu_seqlens=None, max_seqlen=None):
        _refuse_packed(self, cu_seqlens, max_seqlen)
        if inference_params is not None:
            raise NotImplementedError(
                'NegativeWeightedBackpackLMHeadModel has no KV-cached decoding: its content is vocabulary-sized per '
                '(position, sense) and does not fit a cache; generate without kv_cache')
        t, hidden, content = self._stages(input_ids, position_ids)
        weights = self._weights(input_ids, content)                              # (B,k,S)
        # everything in the content's storage order (B,S,k,.) -- the order the kernel reads -- so the
        # vocabulary-sized tensors are produced once and never transposed in memory
        c_st = content.transpose(1, 2)                                           # (B,S,k,d), contiguous
        w_lm_t = self.backpack_network.lm_head.weight.t()
        logits_c = c_st @ w_lm_t                                                 # (B,S,k,V)
        logits_w = (c_st * weights.transpose(1, 2).unsqueeze(3).to(c_st.dtype)) @ w_lm_t
        cut = torch.quantile(logits_w.float(), q=0.02, keepdim=True, dim=-1)
        logits_c = torch.where(logits_w < cut, logits_w, logits_c).transpose(1, 2)   # (B,k,S,V) view
        return CausalLMOutput(logits=self._mix(t, hidden, logits_c))


class ReplacedWordLMHeadModel(_Intervened):
    """Tokens listed in `sense_dict` {token id: (k, d) tensor} contribute those sense vectors instead of
    their own (reference :168-199)."""

    def __init__(self, backpack_network, sense_dict):
        super().__init__()
        self.backpack_network = backpack_network
        self.sense_dict = sense_dict

    def replace_content(self, input_ids, content):
        content = content.clone()
        for word, senses in self.sense_dict.items():           # one masked assignment per listed word
            hit = (input_ids == word)                            # (B,S)
            if bool(hit.any()):
                b_idx, s_idx = hit.nonzero(as_tuple=True)
                content[b_idx, :, s_idx, :] = senses.to(content.device, content.dtype)
        return content

    # ---- KV-cached decoding: cache form only (the rows are edited as they are appended; the whole-vocabulary table is
    # neither cloned nor edited), sense_dict as a device lookup so that a captured step asks the host nothing ----
    cache_form_only = True

    def edit_rows(self, input_ids, content, ip):
        if ip.sequence_len_offset == 0:
            self._read_sense_dict(ip, input_ids.device, self.backpack_network.lm_head.weight.dtype)
        slot, rows = ip.key_value_memory_dict['intervened_replace']
        s = slot[input_ids]                                                       # (B,S), -1 = keep the token's own rows
        picked = rows[s.clamp(min=0)]                                             # (B,S,k,d)
        return torch.where((s >= 0)[:, :, None, None], picked, content.transpose(1, 2)).transpose(1, 2)

    def _read_sense_dict(self, ip, device, dtype):
        """token id -> slot (vocab,) and the stacked replacement rows (n,k,d): once per prefill."""
        vocab = self.backpack_network.lm_head.weight.shape[0]
        t = self.backpack_network.transformer
        slot = torch.full((vocab,), -1, dtype=torch.long)
        rows = [torch.zeros(t.num_content_vectors, t.config.n_embd)]              # slot 0 when the dict is empty
        for n, (word, senses) in enumerate(self.sense_dict.items()):
            slot[int(word)] = n
            rows.append(senses.detach().cpu().float())
        rows = rows[1:] or rows
        ip.key_value_memory_dict['intervened_replace'] = (slot.to(device), torch.stack(rows).to(device, dtype))

    def _mixed(self, input_ids, position_ids):
        t, hidden, content = self._stages(input_ids, position_ids)
        content = self.replace_content(input_ids, content)
        if t.fused_senses and content.transpose(1, 2).stride(-1) != 1:
            content = content.contiguous()
        return self._mix(t, hidden, content)


class ScaledSenseLMHeadModel(_Intervened):
    """One sense of the listed words scaled by `percent` wherever they occur: the counterfactual of the reference's gender-bias
    experiment (training/src/test_genderbias.py:71-78, compute_counterfactual: `contextualization[0, sense_index, :, j] *=
    percent` for every position j whose token is one of `word_ids`).  The key weights are `percent` at (sense_index, those
    positions) and 1 elsewhere, so on the HIP path the contraction stays one bp_sense_mix_weighted launch.  percent = 1 is
    the wrapped network.  Full forward only: `inference_params` raises (read the result with src/utils/scoring.py:candidate_probs)."""

    def __init__(self, backpack_network, word_ids, sense_index, percent):
        super().__init__()
        self.backpack_network = backpack_network
        self.word_ids = [int(w) for w in (word_ids.tolist() if torch.is_tensor(word_ids) else word_ids)]
        self.sense_index = int(sense_index)
        self.percent = float(percent)
        k = backpack_network.transformer.num_content_vectors
        if not 0 <= self.sense_index < k:
            raise ValueError(f'sense_index {sense_index} outside the {k} senses of the network')

    def forward(self, input_ids, position_ids=None, inference_params=None, cu_seqlens=None, max_seqlen=None):
        _refuse_packed(self, cu_seqlens, max_seqlen)
        if inference_params is not None:
            raise NotImplementedError('ScaledSenseLMHeadModel has no KV-cached decoding: it is a full-forward readout')
        return super().forward(input_ids, position_ids, None)

    def key_weight(self, input_ids, nsenses):
        """(B,k,S) fp32: `percent` at (sense_index, positions holding one of word_ids), 1 elsewhere."""
        words = torch.as_tensor(self.word_ids, dtype=input_ids.dtype, device=input_ids.device)
        hit = (input_ids.unsqueeze(-1) == words).any(dim=-1)                       # (B,S)
        weight = torch.ones(input_ids.shape[0], nsenses, input_ids.shape[1], dtype=torch.float32, device=input_ids.device)
        weight[:, self.sense_index] = torch.where(hit, self.percent, 1.0)
        return weight

    def _mixed(self, input_ids, position_ids):
        t, hidden, content = self._stages(input_ids, position_ids)
        return self._mix(t, hidden, content, self.key_weight(input_ids, content.shape[1]))
