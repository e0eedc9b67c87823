"""bp_segment_sum_rows alone (csrc/segment_sum_rows.hip): GB/s of the row stream at the shape of a Backpack-Small training
chunk, for the segment-length patterns that matter -- one row per segment (uniform ids barely repeat), a Zipf draw with
exponent 1 over the vocabulary (text), one segment that holds every row (the worst case of the split).

    python scripts/bench_segment_sum.py [--rows 32768] [--cols 12288] [--repeats 5] [--out FILE.jsonl]
One JSON line per pattern: the median of `repeats` timings of 10 launches each, and their spread.  Bytes = the 16-bit rows
read once + the fp32 sums written once."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'backpacks-flash-attn_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402

import bp_hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=32768)
    ap.add_argument('--cols', type=int, default=12288)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = torch.randn(a.rows, a.cols, device=dev, generator=gen).bfloat16()
    weights = 1.0 / torch.arange(1, 50257 + 1, device=dev, dtype=torch.float64)
    patterns = {
        'ones': torch.randperm(a.rows, device=dev, generator=gen),
        'zipf': torch.unique(torch.multinomial(weights, a.rows, replacement=True, generator=gen), return_inverse=True)[1],
        'one': torch.zeros(a.rows, dtype=torch.int64, device=dev),
    }
    lines = []
    for name, index in patterns.items():
        n_segments = int(index.max()) + 1
        order, seg_begin = bp_hip.row_segments(index, n_segments)
        acc = torch.empty(n_segments, a.cols, device=dev)
        longest = int((seg_begin[1:] - seg_begin[:-1]).max())
        for _ in range(3):
            bp_hip.segment_sum_rows(rows, order, seg_begin, acc)
        times = []
        for _ in range(a.repeats):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(10):
                bp_hip.segment_sum_rows(rows, order, seg_begin, acc)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) / 10)
        times.sort()
        moved = rows.numel() * 2 + acc.numel() * 4
        line = {'kernel': 'bp_segment_sum_rows', 'pattern': name, 'n_rows': a.rows, 'cols': a.cols, 'n_segments': n_segments,
                'longest_segment': longest, 'us_median': round(times[len(times) // 2] * 1e3, 1),
                'us_min': round(times[0] * 1e3, 1), 'us_max': round(times[-1] * 1e3, 1),
                'gb_per_s': round(moved / (times[len(times) // 2] * 1e-3) / 1e9, 1), 'bytes': moved}
        print(json.dumps(line))
        lines.append(line)
    if a.out:
        with open(a.out, 'a') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
