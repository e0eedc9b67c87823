"""score_tokens on rows of different lengths: the padded batch against the packed one (packed=True).

    python scripts/bench_packed_eval.py [--rows 64] [--lo 32] [--hi 1024] [--runs 5] [--seed 0]
                                        [--out profiles/packed_eval_small.jsonl]

Backpack-Small, bf16.  Two legs, one JSON line each (stdout and appended to --out):
  ragged   --rows rows whose lengths are drawn uniformly from lo .. hi (seeded), right-padded to the longest
  equal    every length = hi: nothing to save, what the packed launch costs against the padded one
In each leg `padded` (score_tokens(..., lengths=)) and `packed` (..., packed=True) alternate in one process, --runs times
each after one untimed call each; wall-clock milliseconds around a device synchronisation (packing reads the lengths on the
host, which belongs to the packed leg's cost).  Reported: every run, median, min, max; the ratio of the medians next to
B * max_len / sum(len), the ratio it should approach; for `equal` how far the packed median is from the padded one, in
units of the padded leg's own min .. max spread.  Nothing here is a threshold."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'backpacks-flash-attn_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (time.perf_counter() - t0) * 1e3


def alternate(legs, runs):
    for fn in legs.values():
        fn()
    ms = {n: [] for n in legs}
    for _ in range(runs):
        for name, fn in legs.items():
            ms[name].append(round(timed(fn), 3))
    return ms


def emit(line, path):
    text = json.dumps(line)
    print(text, flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'a') as f:
            f.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=64)
    ap.add_argument('--lo', type=int, default=32)
    ap.add_argument('--hi', type=int, default=1024)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'packed_eval_small.jsonl'))
    a = ap.parse_args()
    from bench import MODELS
    from src.models.backpack import BackpackConfig, BackpackLMHeadModel
    from src.utils.scoring import score_tokens
    dev = torch.device('cuda', 0)
    cfg = BackpackConfig(vocab_size=50257, n_positions=a.hi, scale_attn_by_inverse_layer_idx=True, use_flash_attn=True,
                         fused_bias_fc=True, fused_dense_gelu_dense=True, fused_dropout_add_ln=True, pad_vocab_size_multiple=8,
                         **MODELS['small'])
    torch.manual_seed(0)
    model = BackpackLMHeadModel(cfg, device=dev, dtype=torch.bfloat16).eval()
    g = torch.Generator().manual_seed(a.seed)
    drawn = torch.randint(a.lo, a.hi + 1, (a.rows,), generator=g)
    for leg, lengths in (('ragged', drawn), ('equal', torch.full((a.rows,), a.hi))):
        width = int(lengths.max())
        ids = torch.randint(0, 50257, (a.rows, width), generator=g)
        ids[torch.arange(width)[None, :] >= lengths[:, None]] = 0
        ids, lens = ids.to(dev), lengths.to(dev)
        want = ('logprob', 'rank')
        ms = alternate({'padded': lambda: score_tokens(model, ids, lengths=lens, want=want),
                        'packed': lambda: score_tokens(model, ids, lengths=lens, want=want, packed=True)}, a.runs)
        pad, pack = score_tokens(model, ids, lengths=lens, want=want), score_tokens(model, ids, lengths=lens, want=want, packed=True)
        line = {'bench': 'packed_eval', 'model': 'small', 'dtype': 'bf16', 'leg': leg, 'rows': a.rows, 'lo': a.lo, 'hi': a.hi,
                'seed': a.seed, 'runs': a.runs, 'max_len': width, 'tokens': int(lengths.sum()),
                'padded_positions_over_tokens': round(a.rows * width / int(lengths.sum()), 3)}
        for name in ms:
            line[f'{name}_ms_runs'] = ms[name]
            line[f'{name}_ms_median'] = round(statistics.median(ms[name]), 3)
            line[f'{name}_ms_min'], line[f'{name}_ms_max'] = min(ms[name]), max(ms[name])
        line['padded_over_packed'] = round(line['padded_ms_median'] / line['packed_ms_median'], 3)
        spread = line['padded_ms_max'] - line['padded_ms_min']
        line['packed_minus_padded_ms'] = round(line['packed_ms_median'] - line['padded_ms_median'], 3)
        line['packed_minus_padded_in_padded_spreads'] = round(line['packed_minus_padded_ms'] / spread, 2) if spread > 0 else None
        line['max_logprob_difference'] = round((pad.logprobs - pack.logprobs).abs().max().item(), 5)
        line['ranks_equal_share'] = round(((pad.ranks == pack.ranks) | ~pad.mask).float().mean().item(), 5)
        emit(line, a.out)
        del ids, lens
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
