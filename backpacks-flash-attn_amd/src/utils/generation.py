"""Greedy decoding / sampling -- mirror of the reference's training/src/utils/generation.py:23-92.  By default, as
upstream, there is no KV cache: every step re-runs the whole forward on the grown prefix (so every step exercises the
HIP attention and sense-mix kernels); `kv_cache=True` decodes on the caches of InferenceParams instead (_decode_cached).
`temperature`, `top_k`, `top_p`, `rng_state` or `device_pick=True` move the pick to the device (bp_pick_token; _eager_pick on CPU tensors), on the cache with
cg=True inside the captured step (_decode_cached_picked); without them the loops below run as they always did.
`repetition_penalty`, `eos_token_id`, `pad_token_id` and `min_length` (kv_cache=True only) select the controlled pick
(bp_pick_token_ctl): rows stop at their EOS, the loop ends once every row has, and `lengths` reports where.
`no_repeat_ngram_size`, `frequency_penalty`, `presence_penalty` and `suppress_tokens` (kv_cache=True only) select its limited
form (bp_pick_token_lim): no n-gram twice, counted penalties on what was generated, ids that never appear.
`bad_words_ids` and `stop_sequences` (kv_cache=True only), lists of token-id lists, select its phrased form
(bp_pick_token_phrases): a banned phrase never appears, a row ends where its generated text ends with a stop sequence, and
`stop_reasons` tells what ended it.
`prompt_lengths` (kv_cache=True only) takes a batch of right-padded prompts of different lengths: every row generates the same
number of tokens behind ITS prompt (_CachedSteps; bp_pick_token_lim_rows where a limit or `min_new_tokens` needs the row's begin).
`output_logprobs` / `top_logprobs` (kv_cache=True only) record what the model thought of every token it produced: one more
launch behind each pick (bp_pick_report; _eager_report on CPU tensors), with cg=True inside the captured step (_PickRecord).
Differences kept deliberately small: the result is a plain dataclass instead of the
transformers `*DecoderOnlyOutput` classes (removed in transformers 5), and the appended token is
`unsqueeze(1)` so batch sizes > 1 work (the reference's `unsqueeze(0)` in greedy_decode, :68, only
concatenates for batch 1; identical result there).

Index contract kept bit for bit: the reference never appends the LAST token it picks (:64-72 -- `seqlen`
starts at prompt + 1 and the loop appends only while `seqlen < max_length`), so `sequences` has
max(prompt_len, max_length - 1) columns, not max_length as its docstring says; `scores` holds the first
step's logits only (:59).  Same here."""
import warnings
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch


@dataclass
class InferenceParams:
    """The reference's KV-cache state (flash_attn/utils/generation.py:11-20): `key_value_memory_dict[layer_idx]` holds a
    (max_batch_size, max_sequence_len, 2, nheads, head_dim) cache per trunk layer (a Backpack adds its sense keys and row
    index under keys of their own, see BackpackModel).  A call with `sequence_len_offset == 0` is a prefill; later calls
    take one new token per sample.  `lengths_per_sample`, optional, is a (max_batch_size,) int32 DEVICE tensor of the
    cached positions of every sample: when set, decode steps read the lengths from it (per-sample lengths, no host value
    in the step -- one captured graph serves every step) and the caller advances it, as it advances
    `sequence_len_offset`; when None the lengths are `sequence_len_offset`."""
    max_sequence_len: int
    max_batch_size: int
    sequence_len_offset: int = 0
    batch_size_offset: int = 0
    key_value_memory_dict: dict = field(default_factory=dict)
    lengths_per_sample: Optional[torch.Tensor] = None


@dataclass
class DecoderOnlyOutput:
    sequences: torch.Tensor
    scores: Optional[Tuple[torch.Tensor, ...]] = None
    lengths: Optional[torch.Tensor] = None      # (batch,) int64: 1 + the column of every row's first EOS, when an EOS id is given
    # The record of the picks (output_logprobs / top_logprobs, _PickRecord), aligned with `sequences` column for column: entry
    # [b, c] describes sequences[b, c] under the logits it was picked from.  Prompt columns and the columns at or behind a
    # row's end hold 0 (floats) and -1 (ranks, ids).
    token_logprobs: Optional[torch.Tensor] = None       # (batch, width) fp32: log-probability of the token, raw logits
    token_ranks: Optional[torch.Tensor] = None          # (batch, width) int32: its 0-based rank, ties towards the lower id
    token_entropies: Optional[torch.Tensor] = None      # (batch, width) fp32: entropy of the distribution it came from
    top_token_ids: Optional[torch.Tensor] = None        # (batch, width, n) int32: the n most likely tokens, best first
    top_token_logprobs: Optional[torch.Tensor] = None   # (batch, width, n) fp32: their log-probabilities
    # (batch,) int64, when stop sequences are given: -1 the row ran to its full length, 0 its EOS id ended it, 1 + j its stop
    # sequence j did (the lowest j where several end at the same token)
    stop_reasons: Optional[torch.Tensor] = None


def _decode(input_ids, model, max_length, pick):
    """The reference's loop, statement for statement (:56-72 / :31-44)."""
    seqlen_og = input_ids.shape[1]
    with torch.inference_mode():
        logits = model(input_ids).logits[:, -1]
        scores = [logits]                       # upstream records the first step's scores only (:59,:32)
        next_token = pick(logits)
        seqlen = seqlen_og + 1
        while seqlen < max_length:
            input_ids = torch.cat((input_ids, next_token.unsqueeze(1)), dim=1)
            logits = model(input_ids).logits[:, -1]
            next_token = pick(logits)           # the pick of the final iteration is dropped, as upstream
            seqlen += 1
    return DecoderOnlyOutput(sequences=input_ids, scores=tuple(scores))


def _decode_graphed(input_ids, model, max_length, pick):
    """The same loop on ONE captured forward (HIP graph): the prefix lives in a fixed (batch, width) buffer padded with
    token 0, width = the final sequence length.  Every layer of the model is causal or per-token, so the logits of
    position t do not depend on what is stored behind it: replaying the full-width forward and reading row t gives what
    the reference computes on the grown prefix, for ~150 kernel launches less host work per token (the decode loop of a
    small model is launch-bound: there is no KV cache upstream either).  Greedy tokens can differ from the eager loop
    only where two logits tie to within the rounding of a differently tiled GEMM."""
    batch, seqlen_og = input_ids.shape
    width = max(seqlen_og, max_length - 1)
    buf = torch.zeros((batch, width), dtype=input_ids.dtype, device=input_ids.device)
    buf[:, :seqlen_og] = input_ids
    with torch.inference_mode():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):                      # warm-up outside the capture (workspaces, library handles)
                model(buf)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_logits = model(buf).logits
        graph.replay()
        logits = static_logits[:, seqlen_og - 1].clone()
        scores = [logits]
        next_token = pick(logits)
        seqlen = seqlen_og + 1
        while seqlen < max_length:
            buf[:, seqlen - 1] = next_token
            graph.replay()
            next_token = pick(static_logits[:, seqlen - 1])
            seqlen += 1
    return DecoderOnlyOutput(sequences=buf[:, :max(seqlen_og, seqlen - 1)].clone(), scores=tuple(scores))


def _decode_cached(input_ids, model, max_length, pick, cg=False):
    """The same loop on a KV cache (InferenceParams): one prefill over the prompt, then one cached step per token -- the
    new token's logits from the trunk's K/V caches and the Backpack's sense caches, no forward over the prefix.  The
    cached lengths live on the device (`lengths_per_sample`), so with cg=True ONE decode step is captured (single
    stream) and replayed per token: position, cache appends and the length increment all happen inside the graph.
    The first step runs eagerly (it also warms up the libraries before the capture).  Same index contract as _decode."""
    batch, seqlen_og = input_ids.shape
    ip = InferenceParams(max_sequence_len=max(seqlen_og, max_length - 1), max_batch_size=batch)
    ip.lengths_per_sample = torch.zeros((batch,), dtype=torch.int32, device=input_ids.device)
    tokens = [input_ids]
    with torch.inference_mode():
        logits = model(input_ids, inference_params=ip).logits[:, -1]
        scores = [logits]
        next_token = pick(logits)
        ip.sequence_len_offset = seqlen_og
        ip.lengths_per_sample.fill_(seqlen_og)
        seqlen = seqlen_og + 1
        graph = None
        while seqlen < max_length:
            tokens.append(next_token.unsqueeze(1))
            if graph is not None:
                static_ids.copy_(tokens[-1])
                graph.replay()
                logits = static_logits
            else:
                logits = model(tokens[-1], inference_params=ip).logits[:, -1]
                ip.lengths_per_sample += 1
                if cg and input_ids.is_cuda and seqlen + 1 < max_length:
                    static_ids = tokens[-1].clone()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        static_logits = model(static_ids, inference_params=ip).logits[:, -1]
                        ip.lengths_per_sample += 1
            ip.sequence_len_offset += 1
            next_token = pick(logits)           # the pick of the final iteration is dropped, as upstream
            seqlen += 1
    return DecoderOnlyOutput(sequences=torch.cat(tokens, dim=1), scores=tuple(scores))


# ---- the device pick: temperature / top-k / top-p, one definition for the HIP kernel and its torch restatement -----------------

_M32 = 0xFFFFFFFF
_DEFAULT_STOP_CHECK_EVERY = 16      # steps between two polls of the finished flags (_StopPoll); see DESIGN.md


def _philox2x32(c0, c1, key):
    """Philox2x32-10 (csrc/bp_philox.h) on int64 tensors holding 32-bit values: the 32 x 32 -> 64 bit product is built from
    16-bit halves, so nothing leaves the signed 64-bit range."""
    for _ in range(10):
        hi16, lo16 = c0 >> 16, c0 & 0xFFFF
        ph, pl = hi16 * 0xD256D193, lo16 * 0xD256D193                 # < 2^48 each; product = (ph << 16) + pl
        low = ((ph & 0xFFFF) << 16) + (pl & _M32)
        prod_hi = ((ph >> 16) + (pl >> 32) + (low >> 32)) & _M32
        c0, c1 = prod_hi ^ key ^ c1, low & _M32
        key = (key + 0x9E3779B9) & _M32
    return c0, c1


def _pick_uniforms(rng_state, counters):
    """float64 u = ((r0 >> 8) + 0.5) 2^-24 of every row b: (r0, _) = philox2x32(counters[b], salt, key), (key, salt) =
    dropout_stream(rng_state, b) (csrc/bp_philox.h; tests/philox_ref.py restates both with numpy)."""
    seed, offset = rng_state[0], rng_state[1]
    rows = torch.arange(counters.shape[0], dtype=torch.int64, device=counters.device)
    a, b = _philox2x32(offset & _M32, (offset >> 32) & _M32, seed & _M32)
    key, salt = _philox2x32(a ^ rows, b.expand_as(rows), (seed >> 32) & _M32)
    r0, _ = _philox2x32(counters.to(torch.int64) & _M32, salt, key)
    return ((r0 >> 8).double() + 0.5) * 2.0 ** -24


def _history_mask(sequences, counters, vocab):
    """(batch, vocab) bool: the ids of sequences[b, :min(counters[b], cols)] that lie inside [0, vocab)."""
    batch, cols = sequences.shape
    seen = (torch.arange(cols, device=sequences.device)[None, :] < counters.long()[:, None])
    seen = seen & (sequences >= 0) & (sequences < vocab)
    member = torch.zeros((batch, vocab + 1), dtype=torch.bool, device=sequences.device)
    member.scatter_(1, torch.where(seen, sequences, torch.full_like(sequences, vocab)), True)   # the rest lands in a spare column
    return member[:, :vocab]


def _ngram_mask(sequences, counters, vocab, n):
    """(batch, vocab) bool: the ids that would complete an n-gram the history sequences[b, :Lh] already holds, Lh =
    min(max(counters[b], 0), cols): h[i + n - 1] for every i <= Lh - n whose n - 1 ids equal the last n - 1 of h."""
    batch, cols = sequences.shape
    banned = torch.zeros((batch, vocab), dtype=torch.bool, device=sequences.device)
    for b in range(batch):
        h = sequences[b, :min(max(int(counters[b]), 0), cols)].tolist()
        tail = h[len(h) - n + 1:] if n > 1 else []
        for i in range(len(h) - n + 1):
            if h[i:i + n - 1] == tail and 0 <= h[i + n - 1] < vocab:
                banned[b, h[i + n - 1]] = True
    return banned


def _history_counts(sequences, counters, vocab, begin):
    """(batch, vocab) int64: how often an id occurs at the positions [min(begin, Lh), Lh) of sequences[b]; begin: an int, or
    (batch,) with one value per row."""
    batch, cols = sequences.shape
    at = torch.arange(cols, device=sequences.device)[None, :]
    if isinstance(begin, torch.Tensor):
        begin = begin.to(sequences.device).long()[:, None]
    seen = (at >= begin) & (at < counters.long()[:, None]) & (sequences >= 0) & (sequences < vocab)
    counts = torch.zeros((batch, vocab + 1), dtype=torch.int64, device=sequences.device)
    counts.scatter_add_(1, torch.where(seen, sequences, torch.full_like(sequences, vocab)), seen.long())
    return counts[:, :vocab]


PICK_MAX_PHRASE_LEN = 64      # bp_pick_token_phrases: BP_PICK_MAX_PHRASE_LEN of include/bp_hip.h
PICK_MAX_PHRASES = 1024       # BP_PICK_MAX_PHRASES


def _phrase_lists(phrases, name):
    """`phrases` (a sequence of sequences or tensors of token ids) as a list of lists of ints, within the bounds of
    bp_pick_token_phrases: 1 to 64 ids a phrase, at most 1024 phrases."""
    rows = [[int(t) for t in (ph.tolist() if isinstance(ph, torch.Tensor) else ph)] for ph in phrases]
    if len(rows) > PICK_MAX_PHRASES or any(not 1 <= len(r) <= PICK_MAX_PHRASE_LEN for r in rows):
        raise ValueError(f'generation: {name} takes at most {PICK_MAX_PHRASES} phrases of 1 to {PICK_MAX_PHRASE_LEN} token ids')
    return rows


def _phrase_ban_mask(sequences, counters, vocab, phrases):
    """(batch, vocab) bool: the last id of every phrase whose other ids are the end of the history sequences[b, :Lh], Lh =
    min(max(counters[b], 0), cols) -- raw values compared, the prompt included; a last id outside [0, vocab) bans nothing."""
    batch, cols = sequences.shape
    banned = torch.zeros((batch, vocab), dtype=torch.bool, device=sequences.device)
    for b in range(batch):
        h = sequences[b, :min(max(int(counters[b]), 0), cols)].tolist()
        for w in phrases:
            if len(h) >= len(w) - 1 and h[len(h) - len(w) + 1:] == w[:-1] and 0 <= w[-1] < vocab:
                banned[b, w[-1]] = True
    return banned


def _eager_stop(picked, counters, sequences, finished, begin, minimum, stop_sequences, eos_token_id):
    """What ends a row at this pick, bp_pick_token_phrases's rule: (batch,) int64 on the CPU, -1 nothing, 0 the EOS id, 1 + j
    stop sequence j (the lowest).  `picked` is the token of column c = counters[b]; rows whose flag is set on entry end
    nowhere.  A stop sequence of L ids counts when the token has a column (0 <= c < cols), c >= minimum, c + 1 - L >= begin
    and sequences[b, c + 1 - L : c] ++ [picked] equals it; begin and minimum: an int or one value per row, negatives are 0."""
    batch = picked.shape[0]
    reasons = torch.full((batch,), -1, dtype=torch.int64)
    per_row = lambda v, b: max(int(v[b]) if isinstance(v, torch.Tensor) else int(v), 0)
    for b in range(batch):
        if finished is not None and int(finished[b]) != 0:
            continue
        token, c = int(picked[b]), int(counters[b])
        if eos_token_id is not None and eos_token_id >= 0 and token == eos_token_id:
            reasons[b] = 0
            continue
        if sequences is None or not 0 <= c < sequences.shape[1] or c < per_row(minimum, b):
            continue
        text = sequences[b, :c].tolist() + [token]
        for j, w in enumerate(stop_sequences or ()):
            if c + 1 - len(w) >= per_row(begin, b) and text[c + 1 - len(w):] == w:
                reasons[b] = 1 + j
                break
    return reasons


@dataclass(frozen=True)
class PickOptions:
    """The options of the pick, as greedy_decode / sample and GenerationMixin.generate / .sample take them by keyword.
    temperature, top_k (ties at the threshold kept), top_p: the usual filters of a draw; an argmax ignores them.
    repetition_penalty, eos_token_id, pad_token_id (default: the EOS id), min_length (absolute, prompt included): the
    controls of bp_pick_token_ctl, kv_cache=True only; any of them selects the device pick.  With an EOS id a row ends at its
    first EOS behind the prompt, holds the pad behind it, `sequences` is cut to the longest row and `lengths` (batch,) int64
    reports every row's end; the loop asks every `stop_check_every` steps whether all rows have ended (_StopPoll).
    no_repeat_ngram_size (no n-gram occurs twice, prompt included), frequency_penalty, presence_penalty (an id generated n > 0
    times loses frequency_penalty * n + presence_penalty; the prompt is not counted), suppress_tokens (a list or tensor of ids
    that are never picked): the limits of bp_pick_token_lim, under the same conditions.
    bad_words_ids, stop_sequences (each a list of lists of token ids, 1 to 64 ids a phrase, at most 1024 phrases): the phrases of
    bp_pick_token_phrases, under the same conditions.  The last id of a bad word is never picked while the row's text, prompt
    included, ends with the ids in front of it.  A row whose GENERATED text ends with a stop sequence ends there like a row at
    its EOS id (the sequence stays in the output; min_length / min_new_tokens delay it as they delay the EOS); `lengths` then
    reports every row's end and `stop_reasons` what ended it: -1 the full length, 0 the EOS id, 1 + j stop sequence j.
    min_new_tokens: the EOS id is masked while a row has generated fewer tokens than that, i.e. below the absolute length
    prompt + min_new_tokens of the row (with prompt_lengths: the row's own prompt); not together with min_length.
    do_sample and penalty_begin (the first history position the two counted penalties see) are set by the entry points: sample()
    draws, and the penalties count from the prompt length on (with prompt_lengths: from every row's own, _Picker)."""
    do_sample: bool = False
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    repetition_penalty: float = 1.0
    eos_token_id: Optional[int] = None
    pad_token_id: Optional[int] = None
    min_length: int = 0
    no_repeat_ngram_size: int = 0
    frequency_penalty: float = 0.0
    presence_penalty: float = 0.0
    penalty_begin: int = 0
    suppress_tokens: object = None
    min_new_tokens: int = 0
    bad_words_ids: object = None
    stop_sequences: object = None

    def __post_init__(self):
        if not (self.temperature > 0.0 and self.temperature < float('inf')) or not 0.0 < self.top_p <= 1.0:
            raise ValueError('generation: temperature must be finite and > 0, top_p in (0, 1]')
        if not (self.repetition_penalty > 0.0 and self.repetition_penalty < float('inf')):
            raise ValueError('generation: repetition_penalty must be finite and > 0')
        if self.min_length < 0 or (self.eos_token_id is not None and self.eos_token_id < 0) or (
                self.pad_token_id is not None and self.pad_token_id < 0):
            raise ValueError('generation: min_length, eos_token_id and pad_token_id must not be negative')
        if self.min_new_tokens < 0 or (self.min_new_tokens != 0 and self.min_length != 0):
            raise ValueError('generation: min_new_tokens must not be negative, and is not given together with min_length')
        if self.no_repeat_ngram_size < 0 or not all(abs(float(v)) < float('inf')
                                                    for v in (self.frequency_penalty, self.presence_penalty)):
            raise ValueError('generation: no_repeat_ngram_size must not be negative, frequency_penalty and presence_penalty finite')
        for name in ('bad_words_ids', 'stop_sequences'):
            if getattr(self, name) is not None:
                _phrase_lists(getattr(self, name), name)

    @property
    def limited(self):
        """Whether a limit of bp_pick_token_lim is given; penalty_begin alone is none."""
        return (self.no_repeat_ngram_size != 0 or self.frequency_penalty != 0.0 or self.presence_penalty != 0.0
                or self.suppress_tokens is not None or self.bad_words_ids is not None)

    @property
    def controlled(self):
        """Whether a control of bp_pick_token_ctl, a limit or a stop sequence is given: the options that need kv_cache=True."""
        return (self.repetition_penalty != 1.0 or self.eos_token_id is not None or self.pad_token_id is not None
                or self.min_length != 0 or self.min_new_tokens != 0 or self.limited or self.stop_sequences is not None)

    @property
    def phrased(self):
        """Whether a phrase list of bp_pick_token_phrases is given."""
        return self.bad_words_ids is not None or self.stop_sequences is not None

    @property
    def wants_device_pick(self):
        """Whether any option asks for the device pick: without one (and without rng_state / device_pick=True) the loops pick
        on the host, as the reference does."""
        return self.temperature != 1.0 or self.top_k != 0 or self.top_p != 1.0 or self.controlled

    @property
    def pad(self):
        """What a finished row holds: the pad id, else the EOS id, else 0."""
        if self.pad_token_id is not None:
            return self.pad_token_id
        return self.eos_token_id if self.eos_token_id is not None else 0


def _eager_pick(logits, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, rng_state=None, counters=None,
                repetition_penalty=1.0, eos_token_id=None, pad_token_id=None, min_length=0, finished=None, sequences=None,
                no_repeat_ngram_size=0, frequency_penalty=0.0, presence_penalty=0.0, penalty_begin=0, suppress_tokens=None,
                bad_words_ids=None, stop_sequences=None, ends=None, reasons=None):
    """The contract of bp_pick_token (include/bp_hip.h) in torch ops, for tensors the kernel does not take (CPU): tokens
    (batch,) int64 of logits (batch, vocab).  Greedy: torch.argmax (lowest index of the maximum, a NaN largest).  Sampling:
    z = float(x) / T in fp32; top-k keeps z >= the k-th largest (ties kept); top-p keeps a token iff the kept mass strictly
    above its logit is < p; the token is the lowest index whose cumulative kept probability exceeds u; rows with a NaN or
    +inf, or without a finite logit, take the greedy answer.  Masses are float64 here and 40-bit fixed point in the kernel:
    the two agree wherever u is not within rounding of a boundary of the cumulative distribution.

    The controls of bp_pick_token_ctl: ids of the history sequences[b, :counters[b]] have their value multiplied by
    repetition_penalty (negative values) or by its fp32 reciprocal (the others), in fp32, after the temperature; the EOS
    entry is -inf while counters[b] < min_length; rows whose `finished` flag is set take pad_token_id (default: the EOS
    id).  `finished` is only read here: _Picker sets the flag of a row that picked the EOS id.  min_length and penalty_begin
    each take an int or a (batch,) tensor with one value per row (bp_pick_token_lim_rows; negative entries count as 0).

    The limits of bp_pick_token_lim, applied behind the repetition penalty in this order: an id that occurs n > 0 times at
    the history positions >= penalty_begin loses fp32(frequency_penalty * n + presence_penalty) (float64 product and sum
    rounded once: the kernel's fma wherever the float64 sum is exact); the ids of `suppress_tokens` (a list or a tensor; ids
    outside the vocabulary are ignored) and the ids that would complete an n-gram (n = no_repeat_ngram_size) the history
    already holds are -inf, like the masked EOS.

    The phrases of bp_pick_token_phrases (lists of lists of ids): the last id of a phrase of `bad_words_ids` is -inf, too, while
    the history ends with the ids in front of it (_phrase_ban_mask).  With `stop_sequences` (not None) this function also does
    what the kernel does behind the pick: a row that was not finished on entry and picks the EOS id, or whose text behind
    penalty_begin now ends with a stop sequence (_eager_stop), has its flag in `finished` set, its `ends` entry set to
    counters[b] + 1 and its `reasons` entry to 0 (EOS) or 1 + the sequence's index; other rows' entries are left alone."""
    x = logits.float()
    batch, vocab = x.shape
    if counters is None:
        counters = torch.zeros((batch,), dtype=torch.int32, device=x.device)
    one = torch.ones((), dtype=torch.float32, device=x.device)
    member = None
    if repetition_penalty != 1.0 and sequences is not None:
        member = _history_mask(sequences, counters, vocab)
    masked = None
    if eos_token_id is not None and eos_token_id >= 0:
        masked = torch.zeros((batch, vocab), dtype=torch.bool, device=x.device)
        if isinstance(min_length, torch.Tensor):
            min_length = min_length.to(x.device).clamp(min=0)
        masked[:, eos_token_id] = counters < min_length
    if no_repeat_ngram_size > 0 and sequences is not None:
        banned = _ngram_mask(sequences, counters, vocab, int(no_repeat_ngram_size))
        masked = banned if masked is None else masked | banned
    if suppress_tokens is not None:
        ids = torch.as_tensor(suppress_tokens, dtype=torch.int64, device=x.device).view(-1)
        ids = ids[(ids >= 0) & (ids < vocab)]
        if masked is None:
            masked = torch.zeros((batch, vocab), dtype=torch.bool, device=x.device)
        masked[:, ids] = True
    if bad_words_ids is not None and sequences is not None:
        banned = _phrase_ban_mask(sequences, counters, vocab, _phrase_lists(bad_words_ids, 'bad_words_ids'))
        masked = banned if masked is None else masked | banned
    minus = None
    if (frequency_penalty != 0.0 or presence_penalty != 0.0) and sequences is not None:
        counts = _history_counts(sequences, counters, vocab, penalty_begin.clamp(min=0) if isinstance(penalty_begin, torch.Tensor)
                                 else int(penalty_begin))
        minus = (torch.tensor(frequency_penalty, dtype=torch.float32).double() * counts.double()
                 + torch.tensor(presence_penalty, dtype=torch.float32).double()).float().to(x.device)
        minus = torch.where(counts > 0, minus, torch.zeros_like(minus))

    def controlled(v):
        if member is not None:
            v = torch.where(member, torch.where(v < 0, v * repetition_penalty, v * (one / repetition_penalty)), v)
        if minus is not None:
            v = torch.where(minus != 0, v - minus, v)
        if masked is not None:
            v = torch.where(masked, torch.full_like(v, float('-inf')), v)
        return v

    def done(picked):
        if finished is None:
            return picked
        pad = pad_token_id if pad_token_id is not None else (eos_token_id if eos_token_id is not None else 0)
        picked = torch.where(finished != 0, torch.full_like(picked, pad), picked)
        if stop_sequences is not None:
            why = _eager_stop(picked, counters, sequences, finished, penalty_begin, min_length,
                              _phrase_lists(stop_sequences, 'stop_sequences'), eos_token_id).to(picked.device)
            ended = why >= 0
            finished[ended] = 1
            if ends is not None:
                ends[ended] = (counters[ended] + 1).to(ends.dtype)
            if reasons is not None:
                reasons[ended] = why[ended].to(reasons.dtype)
        return picked

    greedy = torch.argmax(controlled(x), dim=-1)
    if not do_sample:
        return done(greedy)
    z = controlled(x * (one / temperature))
    zmax = z.max(dim=-1, keepdim=True).values
    degenerate = (torch.isnan(z).any(dim=-1) | (z == float('inf')).any(dim=-1) | (zmax[:, 0] == float('-inf')))
    z = torch.where(degenerate[:, None], torch.zeros_like(z), z)          # any finite row: its result is discarded
    zmax = torch.where(degenerate[:, None], torch.zeros_like(zmax), zmax)
    keep = torch.ones_like(z, dtype=torch.bool)
    if 0 < top_k < vocab:
        keep = z >= torch.topk(z, top_k, dim=-1).values[:, -1:]
    w = torch.exp((z - zmax).double()) * keep
    if top_p < 1.0:
        zs, order = torch.sort(torch.where(keep, z, torch.full_like(z, float('-inf'))), dim=-1, descending=True, stable=True)
        ws = torch.gather(w, 1, order)
        before = torch.cumsum(ws, dim=-1) - ws                            # mass in front of every sorted position
        idx = torch.arange(vocab, device=x.device).expand_as(zs)
        new_run = torch.ones_like(zs, dtype=torch.bool)
        new_run[:, 1:] = zs[:, 1:] != zs[:, :-1]
        run_start = torch.cummax(torch.where(new_run, idx, torch.zeros_like(idx)), dim=-1).values
        above = torch.gather(before, 1, run_start)                        # mass of strictly larger logits: ties share it
        keep_sorted = above < top_p * ws.sum(dim=-1, keepdim=True)
        keep = keep & torch.zeros_like(keep).scatter_(1, order, keep_sorted)
        w = w * keep
    cdf = torch.cumsum(w, dim=-1)
    u = _pick_uniforms(rng_state, counters)
    hit = cdf > (u * cdf[:, -1])[:, None]
    last_kept = vocab - 1 - torch.flip(keep, dims=(-1,)).int().argmax(dim=-1)
    drawn = torch.where(hit.any(dim=-1), hit.int().argmax(dim=-1), last_kept)
    return done(torch.where(degenerate, greedy, drawn))


class _Picker:
    """The pick of the decode loops through bp_pick_token (CUDA tensors) or _eager_pick: argmax when not do_sample, else a
    draw after temperature / top-k / top-p.  `counters` (batch,) int32 on the logits' device hold the 0-based sequence
    position of the token being picked: the Philox counter, and the column of `sequences` that receives the token.
    With an EOS id or stop sequences it owns `finished` (batch,) int32 on the logits' device, allocated by the first pick: the
    flag of a row is set by the pick that returns the EOS id or completes a stop sequence, and every later pick of that row
    returns the pad.  With stop sequences it also owns `ends` and `reasons` (batch,) int32, -1 until the pick that ends the row
    writes them (bp_pick_token_phrases).  The phrase lists are packed and copied to the device once, here.
    `prompt_lengths` (batch,) int32 on that device, for prompts of different lengths: a row's counted penalties begin, and
    its min_new_tokens count, and the text a stop sequence is looked for in begins, at its own prompt length -- per-row values
    of the pick (bp_pick_token_lim_rows), passed only where an option reads them."""

    def __init__(self, options, rng_state, device, prompt_lengths=None):
        self.options, self.finished, self.ends, self.reasons = options, None, None, None
        if options.do_sample and rng_state is None:       # from torch's generator: torch.manual_seed reproduces a run
            rng_state = torch.randint(-2 ** 63, 2 ** 63 - 1, (2,), dtype=torch.int64, device=device)
        self.rng_state = rng_state.to(device) if rng_state is not None else None
        # the keywords of bp_hip.pick_token and of _eager_pick, by the entry they select (bp_hip.pick_form): the controls only
        # for a controlled pick and the limits, penalty_begin among them, only for a limited one
        o = options
        self.keywords = dict(do_sample=o.do_sample, temperature=o.temperature, top_k=o.top_k, top_p=o.top_p)
        if o.controlled:
            self.keywords.update(repetition_penalty=o.repetition_penalty, eos_token_id=o.eos_token_id, pad_token_id=o.pad,
                                 min_length=o.min_length)
            if o.min_new_tokens:      # absolute, as min_length is: behind the prompt, the row's own where they differ
                self.keywords['min_length'] = o.penalty_begin + o.min_new_tokens if prompt_lengths is None else \
                    (prompt_lengths + o.min_new_tokens).to(torch.int32)
        if o.limited:
            suppress = o.suppress_tokens
            if suppress is not None:                  # a list or a tensor: on the device once, as the kernel reads it
                suppress = torch.as_tensor(suppress).to(device=device, dtype=torch.int32).reshape(-1).contiguous()
            self.keywords.update(no_repeat_ngram_size=o.no_repeat_ngram_size, frequency_penalty=o.frequency_penalty,
                                 presence_penalty=o.presence_penalty, suppress_tokens=suppress,
                                 penalty_begin=o.penalty_begin if prompt_lengths is None else prompt_lengths)
        if o.phrased:
            phrases = {name: _phrase_lists(getattr(o, name), name) for name in ('bad_words_ids', 'stop_sequences')
                       if getattr(o, name) is not None}
            if torch.device(device).type == 'cuda':
                import bp_hip
                phrases = {name: bp_hip.pack_phrases(rows, device, name) for name, rows in phrases.items()}
            self.keywords.update(penalty_begin=o.penalty_begin if prompt_lengths is None else prompt_lengths, **phrases)

    def __call__(self, logits, counters, tokens=None, sequences=None):
        """tokens (batch,) int64; also stored into `tokens` (batch elements) and column counters[b] of `sequences`."""
        stops = self.options.stop_sequences is not None
        if (self.options.eos_token_id is not None or stops) and self.finished is None:
            self.finished = torch.zeros((logits.shape[0],), dtype=torch.int32, device=logits.device)
            if stops:
                self.ends = torch.full((logits.shape[0],), -1, dtype=torch.int32, device=logits.device)
                self.reasons = torch.full((logits.shape[0],), -1, dtype=torch.int32, device=logits.device)
        outputs = {'ends': self.ends, 'reasons': self.reasons} if stops else {}
        if logits.is_cuda:
            import bp_hip
            return bp_hip.pick_token(logits, rng_state=self.rng_state, counters=counters, tokens=tokens, sequences=sequences,
                                     finished=self.finished, **outputs, **self.keywords).view(-1)
        picked = _eager_pick(logits, rng_state=self.rng_state, counters=counters, finished=self.finished, sequences=sequences,
                             **outputs, **self.keywords)
        if self.finished is not None and not stops:       # with stop sequences _eager_pick has set the flags, as the kernel does
            self.finished[picked == self.options.eos_token_id] = 1
        if tokens is not None:
            tokens.view(-1).copy_(picked)
        if sequences is not None:
            cols = counters.long()
            ok = (cols >= 0) & (cols < sequences.shape[1])
            rows = torch.arange(sequences.shape[0], device=sequences.device)
            sequences[rows[ok], cols[ok]] = picked[ok]
        return picked

    def loop_pick(self, input_ids):
        """pick(logits) for the loops without a cache, which keep a device position of their own."""
        position = torch.full((input_ids.shape[0],), input_ids.shape[1], dtype=torch.int32, device=input_ids.device)

        def pick(logits):
            picked = self(logits, position)
            position.add_(1)
            return picked.to(input_ids.dtype)
        return pick


PICK_REPORT_MAX_TOP = 16      # bp_pick_report: BP_PICK_REPORT_MAX_TOP of include/bp_hip.h


def _eager_report(logits, tokens, counters, *, logprob=None, rank=None, entropy=None, top_idx=None, top_logprob=None):
    """The contract of bp_pick_report (include/bp_hip.h) in torch ops, for tensors the kernel does not take (CPU); the
    signature of bp_hip.pick_report.  Per row b with c = counters[b] in [0, cols) -- other rows are left alone -- column c of
    the records that are given receives: logprob, rank and entropy of tokens[b] as _eager_score_rows (src/utils/scoring.py)
    defines them, fp32; top_idx[b, c, i] the column of position i in the order (float(x) descending with -0 == +0, a NaN above
    every number, column ascending) and top_logprob[b, c, i] = float(x) - lse of that element."""
    from src.utils.scoring import _eager_score_rows
    given = {'logprob': logprob, 'rank': rank, 'entropy': entropy, 'top_idx': top_idx, 'top_logprob': top_logprob}
    if all(v is None for v in given.values()):
        raise RuntimeError('_eager_report: give at least one record')
    batch, vocab = logits.shape
    tops = [v for v in (top_idx, top_logprob) if v is not None]
    n_top = tops[0].shape[2] if tops else 0
    if any(v.shape[2] != n_top for v in tops) or (tops and not 1 <= n_top <= min(vocab, PICK_REPORT_MAX_TOP)):
        raise RuntimeError(f'_eager_report: top_idx and top_logprob hold the same 1 .. min(vocab, {PICK_REPORT_MAX_TOP}) entries')
    cols = next(v for v in given.values() if v is not None).shape[1]
    at = counters.long()
    ok = (at >= 0) & (at < cols)
    rows, at = torch.arange(batch, device=logits.device)[ok], at[ok]
    got = _eager_score_rows(logits, tokens.reshape(batch).long(), want=('logprob', 'rank', 'lse', 'entropy'))
    for name in ('logprob', 'rank', 'entropy'):
        if given[name] is not None:
            given[name][rows, at] = got[name][ok]
    if n_top:
        x = logits.float()
        # the order as one float64 key: a NaN above +inf, -0 == +0; the stable sort keeps the lower column of equals first
        key = x.double().clamp(max=torch.finfo(torch.float64).max)
        key = torch.where(torch.isnan(x), float('inf'), key)
        order = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :n_top]
        if top_idx is not None:
            top_idx[rows, at] = order[ok].to(torch.int32)
        if top_logprob is not None:
            top_logprob[rows, at] = (x.gather(1, order) - got['lse'][:, None])[ok]


class _PickRecord:
    """The record of a generation's picks (output_logprobs / top_logprobs): buffers next to the `sequences` of a _CachedSteps --
    the same rows, row stride (the cache capacity) and width; floats start at 0, ranks and ids at -1 -- and the report behind
    every pick: bp_pick_report on CUDA tensors (one launch, no host value: inside the captured step with cg=True), else
    _eager_report.  It gets the pick's logits, its counters (the column) and the token the pick just wrote."""

    def __init__(self, steps, output_logprobs, top_logprobs):
        rows, capacity = steps.sequences.shape[0], steps.sequences.stride(0)
        device, width = steps.sequences.device, steps.width
        self.n_top, self.records = int(top_logprobs), {}

        def buffer(fill, dtype, *last):
            return torch.full((rows, capacity) + last, fill, dtype=dtype, device=device)[:, :width]
        if output_logprobs:
            self.records.update(logprob=buffer(0.0, torch.float32), rank=buffer(-1, torch.int32),
                                entropy=buffer(0.0, torch.float32))
        if self.n_top:
            self.records.update(top_idx=buffer(-1, torch.int32, self.n_top), top_logprob=buffer(0.0, torch.float32, self.n_top))

    def __call__(self, logits, counters, tokens):
        if self.n_top > logits.shape[1]:
            raise ValueError(f'generation: top_logprobs = {self.n_top} exceeds the vocabulary ({logits.shape[1]})')
        if logits.is_cuda:
            import bp_hip
            bp_hip.pick_report(logits, tokens, counters, **self.records)
        else:
            _eager_report(logits, tokens, counters, **self.records)

    _FIELDS = {'logprob': 'token_logprobs', 'rank': 'token_ranks', 'entropy': 'token_entropies', 'top_idx': 'top_token_ids',
               'top_logprob': 'top_token_logprobs'}

    def fields(self, lengths, width):
        """The fields of DecoderOnlyOutput, cut to `width` columns; with `lengths` (the rows' ends, as _trim_at_eos /
        _trim_rows_at_eos return them) the columns at or behind a row's end are reset by the mask that writes the pad."""
        out = {}
        for name, rec in self.records.items():
            rec = rec[:, :width]
            if lengths is not None:
                live = torch.arange(width, device=rec.device)[None, :] < lengths[:, None]
                rec = torch.where(live if rec.dim() == 2 else live[:, :, None], rec,
                                  torch.full_like(rec, 0 if rec.dtype.is_floating_point else -1))
            out[self._FIELDS[name]] = rec.contiguous()
        return out


class _StopPoll:
    """Whether every row has finished, asked without draining the queue.  Every `every` steps the flags are copied into
    pinned host memory behind the steps queued so far, with an event behind the copy; the copy that is READ at that point is
    the previous poll's, whose event is waited for.  So the host is never more than 2 * every steps ahead of the device,
    the device has work queued while the host waits, and the loop ends at most 2 * every steps after the last row has
    finished.  CPU flags are read directly; without flags (no EOS id) the answer is always no."""

    def __init__(self, finished, every=None):
        self.finished, self.every = finished, _DEFAULT_STOP_CHECK_EVERY if every is None else every
        self.steps, self.pending = 0, None
        if finished is not None and finished.is_cuda:
            self.host = [torch.zeros(finished.shape, dtype=finished.dtype).pin_memory() for _ in range(2)]

    def all_finished(self):
        """Called once per step; True when a poll shows every flag set."""
        self.steps += 1
        if self.finished is None or self.steps % self.every:
            return False
        if not self.finished.is_cuda:
            return bool(self.finished.all())
        buf = self.host[(self.steps // self.every) & 1]
        buf.copy_(self.finished, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        previous, self.pending = self.pending, (buf, event)
        if previous is None:
            return False
        previous[1].synchronize()
        return bool(previous[0].all())


def _trim_at_eos(sequences, seqlen_og, eos_token_id, pad_token_id):
    """(sequences cut to max_b end_b columns with the pad behind every row's end_b, end_b (batch,) int64): end_b = 1 + the
    first column >= seqlen_og of row b that holds the EOS id, the full width when there is none."""
    batch, width = sequences.shape
    cols = torch.arange(width, device=sequences.device)[None, :]
    is_eos = (sequences == eos_token_id) & (cols >= seqlen_og)
    first = torch.where(is_eos, cols, torch.full_like(cols, width - 1)).min(dim=1).values
    lengths = first + 1
    sequences = torch.where(cols < lengths[:, None], sequences, torch.full_like(sequences, pad_token_id))
    return sequences[:, :int(lengths.max())].contiguous(), lengths


def _trim_rows_at_eos(sequences, prompt_lengths, new_tokens, eos_token_id, pad_token_id):
    """_trim_at_eos for rows that begin at different positions: end_b = 1 + the first column >= prompt_lengths[b] of row b
    that holds the EOS id, prompt_lengths[b] + new_tokens when there is none (or no EOS id); the pad behind every row's end.
    Cut to max_b end_b columns only when an EOS id is given."""
    batch, width = sequences.shape
    cols = torch.arange(width, device=sequences.device)[None, :]
    begin = prompt_lengths.long()[:, None]
    lengths = begin[:, 0] + new_tokens
    if eos_token_id is not None:
        is_eos = (sequences == eos_token_id) & (cols >= begin) & (cols < lengths[:, None])
        lengths = torch.where(is_eos, cols + 1, lengths[:, None]).min(dim=1).values
    sequences = torch.where(cols < lengths[:, None], sequences, torch.full_like(sequences, pad_token_id))
    if eos_token_id is not None:
        sequences = sequences[:, :int(lengths.max())]
    return sequences.contiguous(), lengths


def _trim_at_ends(sequences, full, ends, reasons, pad_token_id):
    """_trim_at_eos / _trim_rows_at_eos where the pick itself recorded the rows' ends (stop sequences; _Picker.ends / .reasons,
    -1 for a row that did not end): end_b = ends[b] when 0 <= ends[b] <= full[b], else full[b], the row's full length ((batch,)
    int64) -- the last pick of a uniform batch lands behind `sequences` and is dropped, so an end there is none.  Returns
    (sequences cut to max_b end_b columns with the pad behind every row's end, end_b, the reasons with -1 for a full row)."""
    if ends is None:            # no pick was made
        ends = reasons = torch.full_like(full, -1)
    ends, reasons = ends.long(), reasons.long()
    ended = (ends >= 0) & (ends <= full)
    lengths = torch.where(ended, ends, full)
    cols = torch.arange(sequences.shape[1], device=sequences.device)[None, :]
    sequences = torch.where(cols < lengths[:, None], sequences, torch.full_like(sequences, pad_token_id))
    return sequences[:, :int(lengths.max())].contiguous(), lengths, torch.where(ended, reasons, torch.full_like(reasons, -1))


def _check_prompt_lengths(prompt_lengths, input_ids):
    """prompt_lengths (a sequence or a tensor of `batch` integers in [1, seq_len]) as a (batch,) int32 tensor on the device of
    input_ids, and its minimum: ONE copy to the host for the checks, one to the device; no step reads a host value."""
    return _checked_prompt_lengths(prompt_lengths, input_ids)[:2]


def _checked_prompt_lengths(prompt_lengths, input_ids):
    """_check_prompt_lengths, and the host copy it checked (a list): what a packed prefill packs by."""
    host = torch.as_tensor(prompt_lengths).detach().cpu()
    batch, seqlen = input_ids.shape
    if host.dim() != 1 or host.shape[0] != batch or host.is_floating_point() or host.dtype == torch.bool:
        raise ValueError(f'generation: prompt_lengths must hold one integer per row of input_ids ({batch})')
    values = host.tolist()
    if not all(1 <= v <= seqlen for v in values):
        raise ValueError(f'generation: prompt_lengths must lie in [1, seq_len = {seqlen}]: input_ids is right-padded')
    return host.to(device=input_ids.device, dtype=torch.int32), min(values), values


class _CachedSteps:
    """What the loops with the pick on the device share: the InferenceParams with device lengths, the preallocated
    `sequences` (rows, width) holding the prompt, width = max(prompt, max_length - 1) as in _decode, the one-token input
    `static_ids` a pick writes for the next step, the prefill, and the loop over cached steps.  The cache capacity is `width`
    rounded up to a multiple of `capacity_multiple` positions; `sequences` gets the same row stride.
    With `prompt_lengths` (rows,) int32 on the device, input_ids is right-padded: the columns behind a row's prompt are
    overwritten with `pad` before anything reads them, the prefill runs over the padded width (causal: no real position sees
    a pad) and returns the logits of every row's own last position, and the cached lengths start at the rows' own.  A step
    appends at a row's length, so what the prefill cached for the pad columns is overwritten before it could be read.
    With `packed_lengths` too (the host copy of prompt_lengths, a list: `packed_prefill=True` on a model that takes it) the
    prefill runs over the prompts' own positions instead, packed behind one another (_prefill_packed): nothing is computed
    for a pad column, and nothing is cached for one."""

    def __init__(self, input_ids, model, max_length, capacity_multiple=1, prompt_lengths=None, pad=0, packed_lengths=None):
        rows, self.prompt = input_ids.shape
        self.prompt_lengths, self.packed_lengths = prompt_lengths, packed_lengths
        self.input_ids, self.model = input_ids, model
        self.width = max(self.prompt, max_length - 1)
        capacity = (self.width + capacity_multiple - 1) // capacity_multiple * capacity_multiple
        self.ip = InferenceParams(max_sequence_len=capacity, max_batch_size=rows)
        self.lengths = self.ip.lengths_per_sample = torch.zeros((rows,), dtype=torch.int32, device=input_ids.device)
        self.sequences = torch.zeros((rows, capacity), dtype=torch.int64, device=input_ids.device)[:, :self.width]
        self.sequences[:, :self.prompt] = input_ids
        self.static_ids = torch.zeros((rows, 1), dtype=torch.int64, device=input_ids.device)
        if prompt_lengths is not None:
            behind = torch.arange(self.width, device=input_ids.device)[None, :] >= prompt_lengths.long()[:, None]
            self.sequences.masked_fill_(behind, pad)
            self.input_ids = self.sequences[:, :self.prompt].to(input_ids.dtype).contiguous()

    def prefill(self):
        """The logits of the prompt's last position (every row's own, under prompt_lengths); the caches then hold the prompt."""
        if self.packed_lengths is not None:
            return self._prefill_packed()
        logits = self.model(self.input_ids, inference_params=self.ip).logits
        self.ip.sequence_len_offset = self.prompt                 # a host integer, read only as "after the prompt"
        if self.prompt_lengths is None:
            self.lengths.fill_(self.prompt)
            return logits[:, -1]
        self.lengths.copy_(self.prompt_lengths)
        last = (self.prompt_lengths.long() - 1)[:, None, None].expand(-1, 1, logits.shape[-1])
        return logits.gather(1, last)[:, 0].contiguous()

    def _prefill_packed(self):
        """`prefill` over the packed prompts: the pad-cleaned ids without their pad columns, the model's packed prefill
        (inference_params + cu_seqlens + max_seqlen: the caches take every row's own positions), and the LM head over the
        rows' last positions alone where the model is a trunk and a head.  The row index and cu_seqlens are built from the
        HOST copy of the lengths: no value is read back from the device."""
        lens, device = self.packed_lengths, self.input_ids.device
        index = torch.cat([torch.arange(b * self.prompt, b * self.prompt + n) for b, n in enumerate(lens)]).to(device)
        ids = self.input_ids.reshape(-1).index_select(0, index).to(torch.int64)
        cu = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0).to(device=device, dtype=torch.int32)
        last = cu[1:].long() - 1
        packed = dict(inference_params=self.ip, cu_seqlens=cu, max_seqlen=max(lens))
        if hasattr(self.model, 'transformer') and hasattr(self.model, 'lm_head'):
            logits = self.model.lm_head(self.model.transformer(ids, **packed).index_select(0, last))
        else:
            logits = self.model(ids, **packed).logits.index_select(0, last)
        self.ip.sequence_len_offset = self.prompt                 # a host integer, read only as "after the prompt"
        self.lengths.copy_(self.prompt_lengths)
        return logits.contiguous()

    def step_logits(self):
        """The head of every step: the model on `static_ids`, then lengths + 1 -- the counter of the step's pick."""
        logits = self.model(self.static_ids, inference_params=self.ip).logits[:, -1]
        self.lengths += 1
        return logits

    def run(self, step, steps, cg, poll):
        """`steps` times step(), until `poll` (a _StopPoll, asked once per step) shows every row finished.  With cg on CUDA
        tensors the step is captured once, after one eager step and only when a further step remains, and replayed."""
        graph = None
        for i in range(steps):
            if graph is not None:
                graph.replay()
            else:
                step()
                if cg and self.input_ids.is_cuda and i + 1 < steps:
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        step()
                    # the capture ran nothing: lengths, caches, static_ids and sequences are as the eager step left them
            self.ip.sequence_len_offset += 1
            if poll.all_finished():
                break


def _decode_cached_picked(input_ids, model, max_length, picker, cg=False, stop_check_every=None, prompt_lengths=None,
                          report=None, packed_lengths=None):
    """_decode_cached with the pick on the device: the counter of a pick is `lengths_per_sample` after the step's
    increment, the pick writes the next step's input (`static_ids`) and column `position` of the preallocated `sequences`.
    With cg=True the captured graph is model step, length increment, pick: a generated token is one replay, with no launch
    and no host read outside it.  Same index contract as _decode (the final pick lands outside `sequences` and is dropped).
    With an EOS id the loop ends once a poll (_StopPoll, every `stop_check_every` steps) shows every row finished; finished
    rows keep stepping on the pad token until then.  The result is cut at the rows' ends (_trim_at_eos), so it depends
    neither on the polling interval nor on how far the loop overran.
    With `prompt_lengths` every row generates exactly width - prompt tokens behind its own prompt: that many picks and no
    further one, which would land inside a shorter row; `lengths` is always returned (_trim_rows_at_eos).
    With `report` = (output_logprobs, top_logprobs) every pick is followed by its record (_PickRecord) -- the captured graph is
    then model step, length increment, pick, report -- and the result carries the record's fields, trimmed as `sequences` is.
    With `packed_lengths` (prompt_lengths on the host) the prefill is the packed one (_CachedSteps); nothing behind it differs.
    With stop sequences the rows' ends are the pick's own (`ends`, `reasons` of _Picker; _trim_at_ends): `lengths` is always
    returned, `stop_reasons` too, and `sequences` is cut to the longest row."""
    d = _CachedSteps(input_ids, model, max_length, prompt_lengths=prompt_lengths, pad=picker.options.pad,
                     packed_lengths=packed_lengths)
    record = _PickRecord(d, *report) if report is not None else None

    def pick(logits):
        picker(logits, d.lengths, tokens=d.static_ids, sequences=d.sequences)
        if record is not None:
            record(logits, d.lengths, d.static_ids)

    def recorded(sequences, lengths):
        return {} if record is None else record.fields(lengths, sequences.shape[1])

    with torch.inference_mode():
        logits = d.prefill()
        sequences, lengths, o = d.sequences, None, picker.options
        if prompt_lengths is not None:
            new_tokens = d.width - d.prompt
            if new_tokens > 0:
                pick(logits)
                d.run(lambda: pick(d.step_logits()), new_tokens - 1, cg, _StopPoll(picker.finished, stop_check_every))
            if o.stop_sequences is not None:
                sequences, lengths, why = _trim_at_ends(sequences, prompt_lengths.long() + new_tokens, picker.ends, picker.reasons, o.pad)
                return DecoderOnlyOutput(sequences=sequences.to(input_ids.dtype), scores=(logits,), lengths=lengths,
                                         stop_reasons=why, **recorded(sequences, lengths))
            sequences, lengths = _trim_rows_at_eos(sequences, prompt_lengths, new_tokens, o.eos_token_id, o.pad)
            return DecoderOnlyOutput(sequences=sequences.to(input_ids.dtype), scores=(logits,), lengths=lengths,
                                     **recorded(sequences, lengths))
        pick(logits)
        d.run(lambda: pick(d.step_logits()), max_length - d.prompt - 1, cg, _StopPoll(picker.finished, stop_check_every))
        if o.stop_sequences is not None:
            full = torch.full((sequences.shape[0],), d.width, dtype=torch.int64, device=sequences.device)
            sequences, lengths, why = _trim_at_ends(sequences, full, picker.ends, picker.reasons, o.pad)
            return DecoderOnlyOutput(sequences=sequences.to(input_ids.dtype), scores=(logits,), lengths=lengths,
                                     stop_reasons=why, **recorded(sequences, lengths))
        if o.eos_token_id is not None:
            sequences, lengths = _trim_at_eos(sequences, d.prompt, o.eos_token_id, o.pad)
        return DecoderOnlyOutput(sequences=sequences.to(input_ids.dtype), scores=(logits,), lengths=lengths,
                                 **recorded(sequences, lengths))


def packed_prefill_limit(model, input_ids, max_seqlen):
    """None when `model` takes a packed prefill of `input_ids`' device with `max_seqlen` as the longest prompt, else what
    stands in the way (text): BackpackModel.packed_limit's answer for a model that is a `transformer` with one."""
    limit_of = getattr(getattr(model, 'transformer', None), 'packed_limit', None)
    if limit_of is None:
        return f'{type(model).__name__} has no packed forward'
    return limit_of(input_ids, max_seqlen)


def _packed_lengths(model, input_ids, kv_cache, prompt_lengths, host_lengths):
    """packed_prefill=True: the host lengths the prefill packs by, or None -- with one warning per model that names the
    limit -- where the model takes no packed prefill and the loop runs the padded one."""
    if prompt_lengths is None or not kv_cache:
        raise ValueError('generation: packed_prefill needs prompt_lengths and kv_cache=True (it is the prefill of '
                         'right-padded prompts of different lengths into the KV caches)')
    if hasattr(model, '_packed'):
        model._packed(True)               # a model that cannot take it refuses here, before any launch
    limit = packed_prefill_limit(model, input_ids, max(host_lengths))
    if limit is None:
        return host_lengths
    if not getattr(model, '_packed_prefill_fallback_said', False):
        model._packed_prefill_fallback_said = True
        warnings.warn('generation: packed_prefill=True runs the padded prefill on this model: ' + limit)
    return None


def _run_loop(input_ids, model, max_length, pick, do_sample, cg, kv_cache, rng_state, device_pick, stop_check_every,
              pick_options, prompt_lengths=None, output_logprobs=False, top_logprobs=0, packed_prefill=False):
    """The loop greedy_decode / sample select: with the device pick (_Picker) when device_pick, an rng_state, prompt_lengths,
    a record (output_logprobs / top_logprobs) or one of `pick_options` asks for it, else with the host's `pick` exactly as the
    reference runs."""
    if stop_check_every is not None and stop_check_every < 1:
        raise ValueError('generation: stop_check_every must be >= 1')
    report = None
    if output_logprobs or top_logprobs:
        if not 0 <= int(top_logprobs) <= PICK_REPORT_MAX_TOP:
            raise ValueError(f'generation: top_logprobs must lie in [0, {PICK_REPORT_MAX_TOP}]')
        if not kv_cache:
            raise ValueError('generation: output_logprobs and top_logprobs need kv_cache=True (the loops without a cache are '
                             'the reference\'s, statement for statement)')
        report = (bool(output_logprobs), int(top_logprobs))
    # the frequency / presence penalties count from the prompt length on: generated tokens only
    options = PickOptions(do_sample=do_sample, penalty_begin=input_ids.shape[1], **pick_options)
    if prompt_lengths is not None:
        if not kv_cache:
            raise ValueError('generation: prompt_lengths needs kv_cache=True (the loops without a cache are the reference\'s, '
                             'statement for statement)')
        prompt_lengths, _, host_lengths = _checked_prompt_lengths(prompt_lengths, input_ids)
    packed = {}
    if packed_prefill:
        lens = _packed_lengths(model, input_ids, kv_cache, prompt_lengths, None if prompt_lengths is None else host_lengths)
        packed = {} if lens is None else {'packed_lengths': lens}
    if device_pick or rng_state is not None or options.wants_device_pick or prompt_lengths is not None or report is not None:
        picker = _Picker(options, rng_state, input_ids.device, prompt_lengths)
        if kv_cache:
            return _decode_cached_picked(input_ids, model, max_length, picker, cg=cg, stop_check_every=stop_check_every,
                                         prompt_lengths=prompt_lengths, report=report, **packed)
        if options.controlled:
            raise ValueError('generation: repetition_penalty, eos_token_id, pad_token_id, min_length, min_new_tokens, '
                             'no_repeat_ngram_size, frequency_penalty, presence_penalty, suppress_tokens, bad_words_ids and '
                             'stop_sequences need kv_cache=True '
                             '(the loops without a cache are the reference\'s, statement for statement)')
        pick = picker.loop_pick(input_ids)
    if kv_cache:
        return _decode_cached(input_ids, model, max_length, pick, cg=cg)
    if cg and input_ids.is_cuda:
        return _decode_graphed(input_ids, model, max_length, pick)
    return _decode(input_ids, model, max_length, pick)


def greedy_decode(input_ids, model, max_length, cg=False, kv_cache=False, rng_state=None, device_pick=False,
                  stop_check_every=None, prompt_lengths=None, output_logprobs=False, top_logprobs=0, packed_prefill=False,
                  **pick_options):
    """input_ids (batch, seq_len) -> sequences (batch, max_length - 1): argmax continuation.
    cg=True: one captured full-width forward replayed per token (CUDA tensors only), see _decode_graphed.
    kv_cache=True: prefill once, then one cached step per token (with cg=True: one captured step), see _decode_cached.
    device_pick=True: the argmax runs in bp_pick_token (on CPU tensors: _eager_pick), with kv_cache and cg inside the
    captured step (_decode_cached_picked); the sampling options are accepted for symmetry and do not change an argmax.
    prompt_lengths (kv_cache=True only; selects the device pick): a sequence or tensor of `batch` integers 1 <= L_b <= seq_len.
    input_ids is then right-padded: row b's prompt is input_ids[b, :L_b], and what lies behind it is ignored.  With N =
    max(seq_len, max_length - 1) - seq_len, every row generates exactly N tokens: `sequences` (batch, seq_len + N) holds row
    b's prompt in [0, L_b), its tokens in [L_b, L_b + N) and the pad (PickOptions.pad) behind them; `lengths` (batch,) int64,
    always returned, is 1 + the column of the row's first EOS behind its prompt, else L_b + N; `scores` holds the logits of
    position L_b - 1 of every row; with an EOS id `sequences` is cut to the longest row.  With every L_b == seq_len the
    sequences are those of the call without the argument.
    output_logprobs, top_logprobs = n <= 16 (kv_cache=True only; either selects the device pick): the record of the picks, as
    fields of the result aligned with `sequences` column for column (DecoderOnlyOutput): with output_logprobs the log-probability
    and rank of every generated token under the logits it was picked from (the model's: before temperature, penalties and
    filters) and the entropy of that distribution; with top_logprobs the n most likely tokens of every step and their
    log-probabilities.  `sequences` and `lengths` are those of the call without the two.
    packed_prefill=True (needs prompt_lengths and kv_cache=True, else ValueError): the prefill runs over the prompts' own
    positions, packed behind one another, instead of the padded width -- the model's packed prefill (BackpackModel: the ragged
    flash call, the packed sense kernels, bp_scatter_packed_rows into the caches), and the LM head over the B last rows alone.
    Everything behind the prefill is the same loop.  The logits are those of other GEMM shapes: tokens can differ from the padded
    prefill's where two logits are within rounding.  A model that takes no packed prefill (packed_prefill_limit) runs the
    padded one, with one warning per model; the sense-intervened wrappers raise NotImplementedError.
    pick_options: the keywords of PickOptions, see there."""
    return _run_loop(input_ids, model, max_length, lambda logits: torch.argmax(logits, dim=-1), False, cg, kv_cache, rng_state,
                     device_pick, stop_check_every, pick_options, prompt_lengths, output_logprobs, top_logprobs,
                     **({'packed_prefill': True} if packed_prefill else {}))


def sample(input_ids, model, max_length, cg=False, kv_cache=False, rng_state=None, device_pick=False, stop_check_every=None,
           prompt_lengths=None, output_logprobs=False, top_logprobs=0, packed_prefill=False, **pick_options):
    """Ancestral sampling from softmax(logits) (reference :23-48); cg / kv_cache as in greedy_decode.
    temperature, top_k (ties at the threshold kept, as the reference's top_k_filter, training/run_pplm.py:569-581), top_p:
    the usual filters; any of them, an `rng_state` or device_pick=True selects the device pick (bp_pick_token, contract in
    include/bp_hip.h; _eager_pick on CPU tensors).  rng_state: int64 {seed, offset} (bp_hip.new_rng_state), drawn from
    torch's generator when None; the token at sequence position t of row b is a pure function of (logits, rng_state, b, t),
    so cached, graphed and growing-prefix runs under one rng_state draw the same numbers.
    prompt_lengths: right-padded prompts of different lengths, as in greedy_decode; the position t of a draw is the row's own.
    output_logprobs, top_logprobs: the record of the picks, as in greedy_decode.
    packed_prefill: the prefill over the packed prompts, as in greedy_decode.
    pick_options: the keywords of PickOptions, see there."""
    def pick(logits):
        return torch.distributions.Categorical(logits=torch.log_softmax(logits.float(), dim=-1)).sample()
    return _run_loop(input_ids, model, max_length, pick, True, cg, kv_cache, rng_state, device_pick, stop_check_every,
                     pick_options, prompt_lengths, output_logprobs, top_logprobs,
                     **({'packed_prefill': True} if packed_prefill else {}))


# ---- beam search on the KV cache: bp_beam_pick / bp_beam_copy_rows, or their torch restatements on CPU tensors -----------------

@dataclass
class BeamSearchOutput:
    sequences: torch.Tensor            # (batch, cols): the best hypothesis of every prompt
    scores: torch.Tensor               # (batch,) fp32: its sum of log-probabilities
    lengths: torch.Tensor              # (batch,) int64: its length, prompt included (1 + the column of its EOS, if any)
    beam_sequences: torch.Tensor       # (batch, num_beams, cols): every hypothesis, in slot order
    beam_scores: torch.Tensor          # (batch, num_beams) fp32
    beam_lengths: torch.Tensor         # (batch, num_beams) int64


def _eager_beam_pick(logits, beam_scores, finished, beam_width, eos_token_id=None, pad_token_id=None):
    """The contract of bp_beam_pick (include/bp_hip.h) in torch ops, for tensors the kernel does not take (CPU):
    (parent int32, tokens int64, new beam_scores fp32, new finished int32 or None), all (groups * W,); nothing is written.
    A live row's candidates score s_w + (float(x_v) - lse) in fp32 (all -inf for a row with a NaN or +inf, or without a
    finite logit), a finished row has the one candidate (w, pad) at s_w; a NaN score counts as -inf; candidates rank by
    (score descending, w ascending, v ascending); the W winners in rank order keep their parent's slot when it is free, the
    rest take the lowest free slot, so parent[parent[r]] == parent[r].  The sum of exponentials is a plain fp32 sum here
    and 40-bit fixed point in the kernel: the two agree wherever two candidates are not within rounding of each other."""
    x = logits.float()
    rows, vocab = x.shape
    W = int(beam_width)
    if not 1 <= W <= vocab:
        raise ValueError('beam pick: beam_width must be in 1..vocab')
    groups = rows // W
    dev = x.device
    neg_inf = torch.full((), float('-inf'), dtype=torch.float32, device=dev)
    pad = pad_token_id if pad_token_id is not None else (eos_token_id if eos_token_id is not None else 0)
    fin = finished != 0 if finished is not None else torch.zeros((rows,), dtype=torch.bool, device=dev)
    m = x.max(dim=-1).values
    degenerate = torch.isnan(x).any(dim=-1) | (m == float('inf')) | (m == float('-inf'))
    safe_m = torch.where(degenerate, torch.zeros_like(m), m)
    lse = safe_m + torch.log(torch.exp(x - safe_m[:, None]).sum(dim=-1))
    cand = beam_scores.float()[:, None] + (x - lse[:, None])
    cand = torch.where(degenerate[:, None] | torch.isnan(cand), neg_inf, cand) + 0.0
    top_s, top_v = torch.sort(cand, dim=-1, descending=True, stable=True)       # ties: ascending v
    top_s, top_v = top_s[:, :W].clone(), top_v[:, :W].clone()
    valid = torch.ones((rows, W), dtype=torch.bool, device=dev)
    frozen = beam_scores.float()
    frozen = torch.where(torch.isnan(frozen), neg_inf, frozen) + 0.0
    top_s[:, 0] = torch.where(fin, frozen, top_s[:, 0])
    top_v[:, 0] = torch.where(fin, torch.full_like(top_v[:, 0], pad), top_v[:, 0])
    valid[:, 1:] = ~fin[:, None]
    # the group's candidates in (w, rank within w) order: a stable sort by score keeps (w, v) ascending among equals
    g_s, g_v, g_ok = top_s.view(groups, W * W), top_v.view(groups, W * W), valid.view(groups, W * W)
    g_w = torch.arange(W, device=dev).repeat_interleave(W).expand(groups, W * W)
    order = torch.sort(g_s, dim=-1, descending=True, stable=True).indices
    order = torch.gather(order, 1, torch.sort((~torch.gather(g_ok, 1, order)).int(), dim=-1, stable=True).indices)[:, :W]
    win_s, win_v, win_w = torch.gather(g_s, 1, order), torch.gather(g_v, 1, order), torch.gather(g_w, 1, order)
    # slots: winners that find their parent's slot free keep it, the rest take the lowest free one, both in rank order
    ar = torch.arange(groups, device=dev)
    free = torch.ones((groups, W), dtype=torch.bool, device=dev)
    slot = torch.full((groups, W), -1, dtype=torch.int64, device=dev)
    for j in range(W):
        can = free[ar, win_w[:, j]]
        slot[:, j] = torch.where(can, win_w[:, j], slot[:, j])
        free[ar[can], win_w[can, j]] = False
    for j in range(W):
        need = slot[:, j] < 0
        low = free.int().argmax(dim=1)
        slot[:, j] = torch.where(need, low, slot[:, j])
        free[ar[need], low[need]] = False
    at = (ar[:, None] * W + slot).reshape(-1)
    src = (ar[:, None] * W + win_w).reshape(-1)
    parent = torch.empty((rows,), dtype=torch.int32, device=dev)
    parent[at] = src.to(torch.int32)
    tokens = torch.empty((rows,), dtype=torch.int64, device=dev)
    tokens[at] = win_v.reshape(-1)
    scores = torch.empty((rows,), dtype=torch.float32, device=dev)
    scores[at] = win_s.reshape(-1)
    new_finished = None
    if finished is not None:
        hit = fin[src]
        if eos_token_id is not None and eos_token_id >= 0:
            hit = hit | (win_v.reshape(-1) == eos_token_id)
        new_finished = torch.empty((rows,), dtype=torch.int32, device=dev)
        new_finished[at] = hit.to(torch.int32)
    return parent, tokens, scores, new_finished


def _eager_beam_copy_rows(tensors, parent, lengths, first_position):
    """bp_beam_copy_rows in torch ops: rows r with parent[r] != r of every (rows, positions, ...) tensor take positions
    [first_position, lengths[r]) of row parent[r]."""
    rows = parent.shape[0]
    moved = parent.long() != torch.arange(rows, device=parent.device)
    if not bool(moved.any()):          # every hypothesis kept its slot, the common case late in a search
        return
    for t in tensors:
        pos = torch.arange(t.shape[1], device=t.device)
        take = moved[:, None] & (pos[None, :] >= first_position) & (pos[None, :] < lengths.long()[:, None])
        take = take.view(rows, t.shape[1], *([1] * (t.dim() - 2)))
        t.copy_(torch.where(take, t.index_select(0, parent.long()), t))


_BEAM_OWN_CACHES = ('backpack_sense_k', 'backpack_rows', 'backpack_content')


def _beam_row_sets(ip, sequences):
    """What follows a hypothesis from slot to slot, as (rows, positions, ...) tensors: every trunk layer's K/V cache, the
    sense keys, the sequence buffer, and the Backpack's content -- in table form `backpack_rows` (token ids), in content
    form `backpack_content` and NOT `backpack_rows`: there it holds b * max_seqlen + j, a pointer into the row's OWN
    content, which stays where it is while the content it points at is copied."""
    caches = ip.key_value_memory_dict
    unknown = [k for k in caches if not isinstance(k, int) and k not in _BEAM_OWN_CACHES]
    if unknown:
        raise NotImplementedError(f'beam_search: the cache entries {unknown} hold per-row state that is not reordered')
    sets = [caches[k] for k in sorted(k for k in caches if isinstance(k, int))]
    if 'backpack_sense_k' in caches:
        sets.append(caches['backpack_sense_k'])
        if 'backpack_content' in caches:
            content = caches['backpack_content']
            sets.append(content.view(ip.max_batch_size, ip.max_sequence_len, -1))
        else:
            sets.append(caches['backpack_rows'])
    sets.append(sequences)
    return sets


def beam_search(input_ids, model, max_length, num_beams, eos_token_id=None, pad_token_id=None, length_penalty=0.0, cg=False,
                stop_check_every=None, prompt_lengths=None, **sampling_options):
    """Beam search on the KV cache: input_ids (batch, seq_len), prompts of equal length, or right-padded ones with
    `prompt_lengths` (as greedy_decode's: every hypothesis holds width - seq_len tokens behind its group's own prompt, the
    pad behind them, and the lengths, prompt included, are the rows' own) -> BeamSearchOutput.  The rows are
    the prompts repeated num_beams (W, 1..8) times, prefilled once at batch B W (prefilling B rows and fanning out is a
    later optimisation).  A step is: model step on the picked tokens, lengths + 1, bp_beam_pick (the W best of
    the group's W x vocab continuations, on the device), bp_beam_copy_rows (the caches and the sequence buffer follow the
    hypotheses that changed slot; the prompt region is the same within a group and is never copied -- with prompt_lengths
    the copy starts at the shortest prompt: the columns up to a group's own prompt are equal within the group).  With cg=True the
    whole step is captured once, after one eager step.  Exactly width - seq_len picks are made, width = max(seq_len,
    max_length - 1) as in the other loops, so the scores describe the returned tokens.
    With an EOS id a hypothesis that picks it is frozen: it stays in the beam at its score and competes on it (the common
    two-heap formulation moves it to a separate list and ranks that list by a length-normalised score; here
    `length_penalty` acts on the final ranking only), its row keeps stepping on the pad, and the loop ends once a poll
    (_StopPoll) shows every hypothesis frozen.  Best = the largest score / length ** length_penalty, length = the total
    length, prompt included; ties go to the lowest slot.  With the default 0 that is the raw sum of log-probabilities, the
    order used inside the beam.  CPU tensors take _eager_beam_pick / _eager_beam_copy_rows."""
    if sampling_options:
        raise ValueError(f'beam_search takes no sampling or penalty option, got {sorted(sampling_options)}')
    W = int(num_beams)
    if not 1 <= W <= 8:
        raise ValueError('beam_search: num_beams must be in 1..8')
    vocab = getattr(getattr(model, 'config', None), 'vocab_size', None)
    if vocab is None:                                # a model without a config: its output layer tells, before any prefill
        vocab = getattr(getattr(model, 'lm_head', None), 'out_features', None)
    if vocab is not None and W > vocab:
        raise ValueError('beam_search: num_beams exceeds the vocabulary')
    if stop_check_every is not None and stop_check_every < 1:
        raise ValueError('generation: stop_check_every must be >= 1')
    if (eos_token_id is not None and eos_token_id < 0) or (pad_token_id is not None and pad_token_id < 0):
        raise ValueError('generation: eos_token_id and pad_token_id must not be negative')
    if pad_token_id is None:
        pad_token_id = eos_token_id if eos_token_id is not None else 0
    batch, seqlen_og = input_ids.shape
    rows, dev = batch * W, input_ids.device
    first_copied = seqlen_og
    if prompt_lengths is not None:
        prompt_lengths, first_copied = _check_prompt_lengths(prompt_lengths, input_ids)
        prompt_lengths = prompt_lengths.repeat_interleave(W)       # all W rows of a group share its length
    # bp_beam_copy_rows wants rows that start on 16-byte boundaries: the cache capacity is rounded up to four positions (the
    # int32 row index of the Backpack's cache is the narrowest row), the sequence buffer gets the same row stride
    d = _CachedSteps(input_ids.repeat_interleave(W, dim=0), model, max_length, capacity_multiple=4,
                     prompt_lengths=prompt_lengths, pad=pad_token_id)
    width, sequences, static_ids = d.width, d.sequences, d.static_ids
    beam_scores = torch.full((rows,), float('-inf'), dtype=torch.float32, device=dev)
    beam_scores[::W] = 0.0                          # the first pick takes all W winners from beam 0
    finished = torch.zeros((rows,), dtype=torch.int32, device=dev) if eos_token_id is not None else None
    parent = torch.arange(rows, dtype=torch.int32, device=dev)
    with torch.inference_mode():
        logits = d.prefill()
        if W > logits.shape[-1]:
            raise ValueError('beam_search: num_beams exceeds the vocabulary')
        sets = _beam_row_sets(d.ip, sequences)

        def pick(step_logits):
            if step_logits.is_cuda:
                import bp_hip
                bp_hip.beam_pick(step_logits, beam_scores, parent, W, finished=finished, tokens=static_ids,
                                 sequences=sequences, counters=d.lengths, eos_token_id=eos_token_id,
                                 pad_token_id=pad_token_id)
                bp_hip.beam_copy_rows(sets, parent, d.lengths, first_copied)
                return
            new_parent, tokens, scores, flags = _eager_beam_pick(step_logits, beam_scores, finished, W, eos_token_id,
                                                                 pad_token_id)
            parent.copy_(new_parent)
            beam_scores.copy_(scores)
            if finished is not None:
                finished.copy_(flags)
            static_ids.view(-1).copy_(tokens)
            cols = d.lengths.long()
            ok = cols < width
            at = torch.arange(rows, device=dev)
            sequences[at[ok], cols[ok]] = tokens[ok]
            _eager_beam_copy_rows(sets, parent, d.lengths, first_copied)

        poll = _StopPoll(finished, stop_check_every)
        if width > seqlen_og:                        # width - seqlen_og picks, the first on the prefill's logits: nothing to copy yet
            pick(logits)
            if not poll.all_finished():
                d.run(lambda: pick(d.step_logits()), width - seqlen_og - 1, cg, poll)
        if prompt_lengths is not None:
            sequences, lengths = _trim_rows_at_eos(sequences, prompt_lengths, width - seqlen_og, eos_token_id, pad_token_id)
        elif eos_token_id is not None:
            sequences, lengths = _trim_at_eos(sequences, seqlen_og, eos_token_id, pad_token_id)
        else:
            lengths = torch.full((rows,), width, dtype=torch.int64, device=dev)
        scores = beam_scores.view(batch, W).clone()
        lengths = lengths.view(batch, W)
        ranked = scores / lengths.float() ** float(length_penalty) if length_penalty != 0.0 else scores
        slots = torch.arange(W, device=dev).expand(batch, W)
        best = torch.where(ranked == ranked.max(dim=1, keepdim=True).values, slots, torch.full_like(slots, W - 1)).min(dim=1).values
        beams = sequences.to(input_ids.dtype).view(batch, W, -1)
        at = torch.arange(batch, device=dev)
    return BeamSearchOutput(sequences=beams[at, best], scores=scores[at, best], lengths=lengths[at, best],
                            beam_sequences=beams, beam_scores=scores, beam_lengths=lengths)


class GenerationMixin:

    def _ragged(self, prompt_lengths):
        """The keyword of a call with prompt_lengths, none without: such a call runs the statements it always ran.  A model
        whose per-token state looks across positions overrides this to refuse."""
        return {} if prompt_lengths is None else {'prompt_lengths': prompt_lengths}

    @staticmethod
    def _recorded(output_logprobs, top_logprobs):
        """The keywords of a call that asks for a record, none without: such a call runs the statements it always ran."""
        return {'output_logprobs': output_logprobs, 'top_logprobs': top_logprobs} if output_logprobs or top_logprobs else {}

    def _packed(self, packed_prefill):
        """The keyword of a call with packed_prefill=True, none without: such a call runs the statements it always ran.  A
        model whose prefill is written for (B, S) ids overrides this to refuse."""
        return {'packed_prefill': True} if packed_prefill else {}

    def _generate(self, decode, input_ids, max_length, return_dict_in_generate, output_scores, cg, kv_cache, **pick_options):
        output = decode(input_ids, self, max_length, cg=cg, kv_cache=kv_cache, **pick_options)
        if not output_scores:
            output.scores = None
        return output if return_dict_in_generate else output.sequences

    def generate(self, input_ids, max_length, return_dict_in_generate=False, output_scores=False, cg=False, kv_cache=False,
                 rng_state=None, device_pick=False, stop_check_every=None, prompt_lengths=None, output_logprobs=False,
                 top_logprobs=0, packed_prefill=False, **pick_options):
        """greedy_decode on this model; prompt_lengths: right-padded prompts of different lengths, see there; output_logprobs,
        top_logprobs: the record of the picks (with return_dict_in_generate), see there; packed_prefill: the prefill over the
        packed prompts (with prompt_lengths and kv_cache=True), see there; pick_options: the keywords of PickOptions."""
        return self._generate(greedy_decode, input_ids, max_length, return_dict_in_generate, output_scores, cg, kv_cache,
                              rng_state=rng_state, device_pick=device_pick, stop_check_every=stop_check_every,
                              **self._ragged(prompt_lengths), **self._recorded(output_logprobs, top_logprobs),
                              **self._packed(packed_prefill), **pick_options)

    def sample(self, input_ids, max_length, return_dict_in_generate=False, output_scores=False, cg=False, kv_cache=False,
               rng_state=None, device_pick=False, stop_check_every=None, prompt_lengths=None, output_logprobs=False,
               top_logprobs=0, packed_prefill=False, **pick_options):
        """sample on this model; prompt_lengths, output_logprobs, top_logprobs, packed_prefill and pick_options as generate's."""
        return self._generate(sample, input_ids, max_length, return_dict_in_generate, output_scores, cg, kv_cache,
                              rng_state=rng_state, device_pick=device_pick, stop_check_every=stop_check_every,
                              **self._ragged(prompt_lengths), **self._recorded(output_logprobs, top_logprobs),
                              **self._packed(packed_prefill), **pick_options)

    def beam_search(self, input_ids, max_length, num_beams, return_dict_in_generate=False, eos_token_id=None,
                    pad_token_id=None, length_penalty=0.0, cg=False, stop_check_every=None, prompt_lengths=None,
                    **sampling_options):
        """The best hypothesis of every prompt (batch, cols), or the BeamSearchOutput with return_dict_in_generate."""
        output = beam_search(input_ids, self, max_length, num_beams, eos_token_id=eos_token_id, pad_token_id=pad_token_id,
                             length_penalty=length_penalty, cg=cg, stop_check_every=stop_check_every,
                             **self._ragged(prompt_lengths), **sampling_options)
        return output if return_dict_in_generate else output.sequences
