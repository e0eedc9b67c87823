"""Greedy decoding latency of Backpack-Small on the HIP path: the reference's growing-prefix loop (no KV cache upstream)
against generate(..., cg=True), one captured full-width forward replayed per token, and the KV-cached decode,
generate(..., kv_cache=True) eagerly and with cg=True (one captured decode step replayed per token; src/utils/generation.py).

    python scripts/bench_generate.py [--batch 1] [--prompt 16] [--max-length 128] [--model small] [--modes off,cached]
                                     [--legs full,kv] [--intervention none|weighted|weighted-anneal|replaced]
                                     [--pick torch|device|torch,device] [--sample] [--temperature T] [--top-k K] [--top-p P]
                                     [--repetition-penalty R] [--eos ID] [--min-length L] [--stop-check-every N]
                                     [--variant NAME:option=value,...] [--repeats N] [--beams W[,W...]]
                                     [--prompt-lengths LO:HI[:SEED]]

--pick chooses how the next token is picked: `torch` is torch.argmax / torch.distributions.Categorical on the host side
of the loop, `device` the bp_pick_token kernel (device_pick=True; with kv_cache and cg inside the captured step).  With
both, the two picks alternate inside every leg, --repeats times each, in one process: the line then carries the median
and every run of each (`<leg>_<pick>_ms`, `<leg>_<pick>_ms_runs`).  --sample times sample() instead of generate();
--temperature / --top-k / --top-p go to the device pick only (the torch pick has no such options), and so do the controls
of bp_pick_token_ctl: --repetition-penalty, --eos (an id that never occurs, e.g. 50263 of the padded vocabulary, times the
polling of the finished flags alone), --min-length and --stop-check-every (kv legs only).  --variant adds a further pick
that alternates with the others: the device pick with some generation options replaced, e.g.
`--variant pen:repetition_penalty=1.2 --variant n4:eos_token_id=50263,stop_check_every=4`, or with the limits of
bp_pick_token_lim `--variant all:no_repeat_ngram_size=3,frequency_penalty=0.5,presence_penalty=0.5,suppress_tokens=11+12+13`
(a list is written a+b+c), or with the record of the picks (bp_pick_report, one more launch per token; kv legs only)
`--variant rec:output_logprobs=1 --variant rec5:output_logprobs=1,top_logprobs=5`, or with the phrases of bp_pick_token_phrases
`--variant phr:stop_sequences=1+2+3/4+5+6,bad_words_ids=7+8+9` (phrases separated by /, the ids of one by +).

--prompt-lengths LO:HI[:SEED] (kv legs only) adds two further picks that alternate with the others: `ragged`, the device pick
with prompt_lengths drawn once on the host, uniformly from LO..HI (seed SEED, default 0) with the maximum forced to --prompt,
so that the padded width and the number of new tokens are those of the other picks; and `ragged_equal`, the same call with
every length equal to --prompt, i.e. the work of the pick without the argument through the new path; and the two again with
packed_prefill=True, `ragged_packed` and `ragged_equal_packed`: the prefill over the prompts' own positions against the prefill
over the padded width (with --max-length = --prompt + 2 one token is generated behind the prefill: the time is the prefill's).

--beams W[,W...] times beam search instead (its own line per sense_table mode): for every width W, beam_search(num_beams=W,
cg=True) against the greedy device-pick leg generate(kv_cache=True, cg=True, device_pick=True) at the same number of rows
(batch x W prompts), all legs alternating in one process, --repeats times each; then the two beam kernels alone at the
final shape -- bp_beam_pick, and bp_beam_copy_rows with every row but one of each group moving -- in microseconds per call
issued from Python (the `*_host_issue_us` keys: at these sizes the host's cost of a call, an upper bound on the kernel's).

--intervention wraps the model in the control-experiment classes of src/models/intervened_models.py (seeded
content_weights in [0, 3); for the annealed form a scale of 6 / median of the similarity sums at half the final length, so
that the scores are not saturated; eight replaced tokens, four of them in the prompt) and times the same legs on the
wrapper."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'backpacks-flash-attn_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--prompt', type=int, default=16)
    ap.add_argument('--max-length', type=int, default=128)
    ap.add_argument('--model', default='small')
    ap.add_argument('--modes', default='off,cached', help='sense_table modes to run')
    ap.add_argument('--legs', default='full,kv', help='full: growing-prefix loop and its graph; kv: the KV-cached legs')
    ap.add_argument('--intervention', default='none', choices=['none', 'weighted', 'weighted-anneal', 'replaced'])
    ap.add_argument('--pick', default='torch', help='torch, device, or torch,device (alternating)')
    ap.add_argument('--sample', action='store_true', help='time sample() instead of generate()')
    ap.add_argument('--temperature', type=float, default=1.0)
    ap.add_argument('--top-k', type=int, default=0)
    ap.add_argument('--top-p', type=float, default=1.0)
    ap.add_argument('--repetition-penalty', type=float, default=1.0)
    ap.add_argument('--eos', type=int, default=None, help='eos_token_id of the device pick')
    ap.add_argument('--min-length', type=int, default=0)
    ap.add_argument('--stop-check-every', type=int, default=None)
    ap.add_argument('--variant', action='append', default=[], help='NAME:option=value,... : the device pick with these options')
    ap.add_argument('--repeats', type=int, default=1)
    ap.add_argument('--beams', default=None, help='W[,W...]: time beam search against greedy at the same number of rows')
    ap.add_argument('--prompt-lengths', default=None, help='LO:HI[:SEED]: add the picks ragged and ragged_equal (kv legs only)')
    a = ap.parse_args()
    from bench import MODELS
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    dev = torch.device('cuda', 0)
    cfg = BackpackConfig(vocab_size=50257, n_positions=max(a.max_length, 128), scale_attn_by_inverse_layer_idx=True,
                         use_flash_attn=True, fused_bias_fc=True, fused_dense_gelu_dense=True, fused_dropout_add_ln=True,
                         pad_vocab_size_multiple=8, **MODELS[a.model])
    torch.manual_seed(0)
    model = BackpackLMHeadModel(cfg, device=dev, dtype=torch.bfloat16).eval()
    ids = torch.randint(0, 50257, (a.batch, a.prompt), device=dev)
    extra = {}
    if a.intervention != 'none':
        model, extra = intervene(model, a.intervention, ids, (a.prompt + a.max_length) // 2)
    legs = []
    if 'full' in a.legs.split(','):
        legs += [('eager_loop', False, False), ('graph_replay', True, False)]
    if 'kv' in a.legs.split(','):
        legs += [('kv_cache_eager', False, True), ('kv_cache_graph', True, True)]
    for mode in a.modes.split(','):   # content network per position (the reference's order) / cached whole-vocabulary table
        getattr(model, 'backpack_network', model).transformer.sense_table_mode = mode
        if a.beams:
            print(json.dumps(beam_legs(model, ids, a, mode)), flush=True)
            continue
        res = dict(model=a.model, batch=a.batch, prompt=a.prompt, max_length=a.max_length,
                   new_tokens=a.max_length - 1 - a.prompt, sense_table=mode, **extra)
        outs = {}
        picks = a.pick.split(',')
        plain = picks == ['torch'] and not a.sample and a.repeats == 1 and not a.variant and not a.prompt_lengths   # the line of earlier revisions, key for key
        if not plain:
            res.update(sample=a.sample, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
        options = dict(torch={}, device=dict(device_pick=True, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p))
        controls = dict(repetition_penalty=a.repetition_penalty, eos_token_id=a.eos, min_length=a.min_length,
                        stop_check_every=a.stop_check_every)
        controls = {k: v for k, v in controls.items() if v != dict(repetition_penalty=1.0, min_length=0).get(k)}
        if controls:                                   # without them the call is the one of earlier revisions
            options['device'].update(controls)
            res.update(controls)
        for spec in a.variant:
            name, _, pairs = spec.partition(':')
            # suppress_tokens is a list, written a+b+c (the comma separates the options); a list of phrases is a+b+c/d+e+f
            def value(k, v):
                if k in ('bad_words_ids', 'stop_sequences'):
                    return [[int(t) for t in phrase.split('+')] for phrase in v.split('/')]
                return [int(t) for t in v.split('+')] if k == 'suppress_tokens' else json.loads(v)
            changed = {k: value(k, v) for k, v in (pair.split('=') for pair in pairs.split(',') if pair)}
            options[name] = dict(options['device'], **changed)
            res['variant_' + name] = changed
            picks = picks + [name]
        if a.prompt_lengths:
            lo, hi, *seed = (int(v) for v in a.prompt_lengths.split(':'))
            if not 1 <= lo <= hi <= a.prompt or 'full' in a.legs.split(','):
                raise SystemExit('--prompt-lengths LO:HI needs 1 <= LO <= HI <= --prompt and --legs kv')
            drawn = torch.randint(lo, hi + 1, (a.batch,), generator=torch.Generator().manual_seed(seed[0] if seed else 0))
            drawn[int(drawn.argmax())] = a.prompt          # the longest row fills the padded width
            options['ragged_equal'] = dict(options['device'], prompt_lengths=[a.prompt] * a.batch)
            options['ragged'] = dict(options['device'], prompt_lengths=drawn.tolist())
            res['prompt_lengths'] = dict(lo=lo, hi=hi, seed=seed[0] if seed else 0, min=int(drawn.min()),
                                         mean=round(drawn.float().mean().item(), 2))
            options['ragged_equal_packed'] = dict(options['ragged_equal'], packed_prefill=True)
            options['ragged_packed'] = dict(options['ragged'], packed_prefill=True)
            res['prompt_lengths']['sum'] = int(drawn.sum())
            picks = picks + ['ragged_equal', 'ragged', 'ragged_equal_packed', 'ragged_packed']
        decode = model.sample if a.sample else model.generate
        for key, cg, kv in legs:
            runs = {pick: [] for pick in picks}
            for pick in picks:                                               # warm-up (allocator, library handles)
                decode(ids, max_length=a.max_length, cg=cg, kv_cache=kv, **options[pick])
            for _ in range(a.repeats):
                for pick in picks:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = decode(ids, max_length=a.max_length, cg=cg, kv_cache=kv, **options[pick])
                    torch.cuda.synchronize()
                    runs[pick].append((time.perf_counter() - t0) * 1e3)
                    outs[key if pick == picks[0] else key + '_' + pick] = out
            for pick in picks:
                name = key if plain else key + '_' + pick
                dt = sorted(runs[pick])[len(runs[pick]) // 2]
                res[name + '_ms'] = round(dt, 1)
                res[name + '_ms_per_token'] = round(dt / res['new_tokens'], 3)
                if not plain:
                    res[name + '_ms_runs'] = [round(r, 1) for r in runs[pick]]
        # random weights: near-uniform logits, ties flip easily
        if 'eager_loop' in outs:
            res['tokens_equal_fraction'] = round((outs['eager_loop'] == outs['graph_replay']).float().mean().item(), 4)
        if 'kv_cache_eager' in outs and not (a.sample and picks[0] == 'torch'):   # the torch sampler draws anew per call
            res['kv_tokens_equal_graph'] = bool(torch.equal(outs['kv_cache_eager'], outs['kv_cache_graph']))
            if 'eager_loop' in outs:
                res['kv_tokens_equal_fraction'] = round(
                    (outs['kv_cache_eager'] == outs['eager_loop']).float().mean().item(), 4)
        print(json.dumps(res), flush=True)

def _spread(runs):
    runs = sorted(runs)
    return dict(median=round(runs[len(runs) // 2], 2), min=round(runs[0], 2), max=round(runs[-1], 2))


def beam_legs(model, ids, a, mode):
    """The --beams line: beam search against greedy at the same number of rows, then the two beam kernels alone."""
    import bp_hip
    from src.utils.generation import _beam_row_sets, _CachedSteps
    widths = [int(w) for w in a.beams.split(',')]
    new_tokens = a.max_length - 1 - a.prompt
    res = dict(model=a.model, batch=a.batch, prompt=a.prompt, max_length=a.max_length, new_tokens=new_tokens,
               sense_table=mode, beams=widths, repeats=a.repeats)
    calls = {}
    for W in widths:
        wide = ids.repeat_interleave(W, dim=0)
        calls['beam%d' % W] = lambda W=W: model.beam_search(ids, a.max_length, W, cg=True)
        calls['greedy_rows%d' % wide.shape[0]] = lambda wide=wide: model.generate(wide, a.max_length, cg=True, kv_cache=True,
                                                                                device_pick=True)
    runs = {name: [] for name in calls}
    for call in calls.values():                                             # warm-up (allocator, library handles)
        call()
    for _ in range(a.repeats):
        for name, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0) * 1e3)
    for name in calls:
        res[name + '_ms'] = _spread(runs[name])
        res[name + '_ms_per_token'] = round(res[name + '_ms']['median'] / new_tokens, 3)
        res[name + '_ms_runs'] = [round(r, 1) for r in runs[name]]

    def per_call_us(fn, n=50):
        # back-to-back calls from Python: at these sizes this is the host's cost of issuing a call, not the kernel's time
        fn()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            fn()
        end.record()
        torch.cuda.synchronize()
        return round(start.elapsed_time(end) * 1e3 / n, 1)

    dev = ids.device
    for W in widths:
        d = _CachedSteps(ids.repeat_interleave(W, dim=0), model, a.max_length, capacity_multiple=4)   # as beam_search sets up
        rows, width = a.batch * W, d.width
        with torch.inference_mode():
            logits = d.prefill()
        sets = _beam_row_sets(d.ip, d.sequences)
        scores = torch.zeros((rows,), dtype=torch.float32, device=dev)
        parent = torch.empty((rows,), dtype=torch.int32, device=dev)
        res['beam%d_pick_host_issue_us' % W] = per_call_us(lambda: bp_hip.beam_pick(logits, scores, parent, W))
        first = (torch.arange(rows, device=dev) // W * W).to(torch.int32)   # every row continues slot 0 of its group
        full = torch.full((rows,), width, dtype=torch.int32, device=dev)
        res['beam%d_copy_host_issue_us_full_length' % W] = per_call_us(lambda: bp_hip.beam_copy_rows(sets, first, full, a.prompt))
        moved = (rows - a.batch) * (width - a.prompt)
        res['beam%d_copy_bytes_per_row_position' % W] = sum(t[0, 0].numel() * t.element_size() for t in sets)
        res['beam%d_copy_positions_moved' % W] = moved
    return res


def intervene(model, kind, ids, middle):
    """The wrapper of `kind` around `model`, and what to report about it."""
    from src.models.intervened_models import ReplacedWordLMHeadModel, WeightedBackpackLMHeadModel
    g = torch.Generator().manual_seed(11)
    k, d, vocab = model.config.num_content_vectors, model.config.n_embd, model.lm_head.weight.shape[0]
    if kind == 'replaced':
        words = ids[0, :4].tolist() + torch.randint(0, 50257, (4,), generator=g).tolist()
        senses = {w: (torch.randn(k, d, generator=g) * 0.02).to(ids.device, torch.bfloat16) for w in words}
        return ReplacedWordLMHeadModel(model, senses).eval(), dict(intervention=kind)
    cw = (torch.rand(vocab, k, generator=g) * 3).to(ids.device)
    if kind == 'weighted':
        return WeightedBackpackLMHeadModel(model, cw, None, 0.1, anneal=False).eval(), dict(intervention=kind)
    with torch.no_grad():   # random tokens stand in for the continuation of a randomly initialised model
        probe = torch.randint(0, 50257, (ids.shape[0], middle), device=ids.device)
        content = model.transformer.content_model(probe).float()
        sims = torch.relu(content @ model.lm_head.weight[probe].float().transpose(1, 2).unsqueeze(1)).sum(dim=3)
    scale = 6.0 / sims.median().item()
    scores = torch.sigmoid(-scale * sims + 6)
    band = ((scores >= 0.1) & (scores <= 0.9)).float().mean().item()
    return (WeightedBackpackLMHeadModel(model, cw, None, scale, anneal=True).eval(),
            dict(intervention=kind, annealing_scale=round(scale, 3), scores_in_band=round(band, 3)))


if __name__ == '__main__':
    main()
