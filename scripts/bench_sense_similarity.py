"""bp_sense_similarity against the straightforward torch formulation at Backpack-Small dimensions: 50 257 candidate words,
k = 16 senses, d = 768, bf16, on a randomly initialised one-layer model's sense table.

    python scripts/bench_sense_similarity.py [--out profiles/sense_similarity_bench_small.jsonl] [--iters 10]

Legs, alternating in one process, medians of five rounds with min .. max (device events around `iters` calls):
  kernel   bp_hip.sense_similarity, nq = 1 and 4, `MinPair` only and all six outputs
  torch    einsum for G, fp32 norms, the cosine matrix, its reductions -- the same outputs
  neighbors   sense_neighbors(count=100) end to end for one word and for four
Every line carries the algorithmic bytes (ncand * k * d * 2 + outputs) and the rate they give.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (puts the package on sys.path)

import bp_hip  # noqa: E402
from src.models.backpack import BackpackConfig, BackpackLMHeadModel  # noqa: E402
from src.utils import sense_similarity as SS  # noqa: E402

VOCAB, K, D = 50257, 16, 768


def torch_similarity(table, query, want):
    """The torch formulation a user would write: G by einsum, norms from an fp32 copy, five reductions."""
    t, q = table.float(), query.float()
    g = torch.einsum('nie,cje->ncij', q, t)
    cos = g / (q.norm(dim=-1)[:, None, :, None] * t.norm(dim=-1)[None, :, None, :])
    diag = torch.diagonal(cos, dim1=2, dim2=3)
    res = {}
    if 'min_pair' in want:
        res['min_pair'] = diag.min(-1).values
    if 'max_pair' in want:
        res['max_pair'] = diag.max(-1).values
    if 'min_all' in want:
        res['min_all'] = cos.flatten(2).min(-1).values
    if 'max_all' in want:
        res['max_all'] = cos.flatten(2).max(-1).values
    if 'per_sense' in want:
        res['per_sense'] = diag.transpose(1, 2).contiguous()
    if 'flat' in want:
        res['flat'] = torch.diagonal(g, dim1=2, dim2=3).sum(-1) / (q.flatten(1).norm(dim=-1)[:, None] * t.flatten(1).norm(dim=-1)[None, :])
    return res


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sense_similarity_bench_small.jsonl'))
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sense_similarity: no GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    cfg = BackpackConfig(n_embd=D, n_head=12, n_layer=1, num_content_vectors=K, vocab_size=VOCAB, n_positions=64,
                         scale_attn_by_inverse_layer_idx=True, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
                         use_flash_attn=True, pad_vocab_size_multiple=8)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = BackpackLMHeadModel(cfg).to(dev, torch.bfloat16).eval()
    table = model.transformer.sense_table()[:VOCAB]
    lines = []
    for nq in (1, 4):
        words = [1000 * (i + 1) for i in range(nq)]
        query = SS.sense_vectors(model, words)
        for label, want in (('MinPair', ('min_pair',)), ('all six', bp_hip.SIMILARITY_OUTPUTS)):
            out_bytes = sum(4 * nq * VOCAB * (K if w == 'per_sense' else 1) for w in want)
            algo_bytes = VOCAB * K * D * 2 + out_bytes
            legs = {'kernel': lambda: bp_hip.sense_similarity(table, query, want=want),
                    'torch': lambda: torch_similarity(table, query, want)}
            got, ref = legs['kernel'](), legs['torch']()                 # warm-up, and the two legs agree
            for w in want:
                torch.testing.assert_close(got[w], ref[w], rtol=1e-4, atol=1e-5)
            times = {name: [] for name in legs}
            for _ in range(args.rounds):
                for name, fn in legs.items():
                    times[name].append(timed(fn, args.iters))
            for name, ts in times.items():
                med = statistics.median(ts)
                lines.append({'bench': 'sense_similarity', 'leg': name, 'outputs': label, 'nq': nq, 'ncand': VOCAB, 'k': K, 'd': D,
                              'dtype': 'bf16', 'ms_median': round(med, 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4),
                              'algorithmic_bytes': algo_bytes, 'tb_per_s': round(algo_bytes / med / 1e9, 3),
                              'iters': args.iters, 'rounds': args.rounds})
                print(json.dumps(lines[-1]), flush=True)
        fn = lambda: SS.sense_neighbors(model, words, count=100)         # noqa: E731
        fn()
        ts = [timed(fn, args.iters) for _ in range(args.rounds)]
        lines.append({'bench': 'sense_neighbors', 'count': 100, 'measure': 'MinPair', 'nq': nq, 'ncand': VOCAB, 'k': K, 'd': D,
                      'dtype': 'bf16', 'ms_median': round(statistics.median(ts), 4), 'ms_min': round(min(ts), 4),
                      'ms_max': round(max(ts), 4), 'iters': args.iters, 'rounds': args.rounds})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
