"""Whole-vocabulary sense projections at Backpack-Small (src/utils/sense_vocab.py): `non_contextual_localize` and
`sense_extremes(count=20)` on the HIP path (one GEMM and one bp_row_extremes launch per chunk) against a torch-only leg in
the same process that walks the same chunks with `block.max(-1)`, and with `torch.topk` at both ends.  The legs alternate;
every figure is the median of `--runs` timed calls with min .. max beside it.

    python scripts/bench_sense_vocab.py [--model small] [--runs 5] [--chunk-rows 8192] [--out FILE.jsonl]"""
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


def torch_row_extremes(block, n, largest, smallest, out=None):
    """The torch-only stand-in for `_row_extremes`: max / topk on the same block (their tie order is torch's own)."""
    res = [None] * 4
    if largest:
        res[0], res[1] = block.max(-1, keepdim=True) if n == 1 else torch.topk(block, n, dim=-1, largest=True)
    if smallest:
        res[2], res[3] = block.min(-1, keepdim=True) if n == 1 else torch.topk(block, n, dim=-1, largest=False)
    for o, v in zip(out, res):
        if v is not None:
            o.copy_(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='small')
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--chunk-rows', type=int, default=8192)
    ap.add_argument('--count', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from bench import build_model
    from src.utils import sense_vocab as SV
    dev = torch.device('cuda', 0)
    cfg, model = build_model(a.model, 1024, torch.bfloat16, dev)
    vocab_rows = model.lm_head.weight.shape[0]
    target = torch.zeros(vocab_rows, device=dev)
    target[[1000, 2000, 3000, 40000]] = 1.0
    model.transformer.sense_table()
    hip_row_extremes = SV._row_extremes
    workloads = {
        'non_contextual_localize': lambda: SV.non_contextual_localize(target, model, chunk_rows=a.chunk_rows),
        'sense_extremes': lambda: SV.sense_extremes(model, count=a.count, chunk_rows=a.chunk_rows),
    }
    lines = []
    for name, fn in workloads.items():
        times = {'hip': [], 'torch': []}
        for run in range(a.runs + 1):                      # run 0 warms both legs up and is not counted
            for leg in ('hip', 'torch'):
                SV._row_extremes = hip_row_extremes if leg == 'hip' else torch_row_extremes
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if run:
                    times[leg].append((time.perf_counter() - t0) * 1e3)
        SV._row_extremes = hip_row_extremes
        for leg, ms in times.items():
            lines.append(dict(workload=name, leg=leg, model=a.model, dtype='bf16', rows=vocab_rows * cfg.num_content_vectors,
                              cols=vocab_rows, chunk_rows=a.chunk_rows, count=a.count if name == 'sense_extremes' else 1,
                              runs=a.runs, median_ms=round(statistics.median(ms), 2), min_ms=round(min(ms), 2),
                              max_ms=round(max(ms), 2)))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(''.join(json.dumps(line) + '\n' for line in lines))


if __name__ == '__main__':
    main()
