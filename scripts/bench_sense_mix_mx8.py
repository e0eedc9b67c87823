"""Time bp_sense_mix_gather_mx8 against bp_sense_mix_gather on the same table values (the 16-bit table is the dequantised
pair), LSE given: the two legs alternate in one process, one JSON line per shape with medians and quartiles in ms.

    python scripts/bench_sense_mix_mx8.py [--rounds 15] [--iters 10]
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'backpacks-flash-attn_amd'))
import bp_hip  # noqa: E402

SHAPES = [(64, 1024), (64, 4096), (16, 1024), (16, 4096)]     # (B, S) at k = 16, d_k = 48, d_out = 768, 50264 rows


def _time(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main(argv):
    rounds = int(argv[argv.index('--rounds') + 1]) if '--rounds' in argv else 15
    iters = int(argv[argv.index('--iters') + 1]) if '--iters' in argv else 10
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(0)
    k, dk, dout, rows = 16, 48, 768, 50264
    q8, s8 = bp_hip.sense_table_quantize(torch.randn(rows, k, dout, device=dev, generator=g).bfloat16())
    table = bp_hip.sense_table_dequantize(q8, s8, torch.bfloat16)
    for b, s in SHAPES:
        qk = torch.randn(b, s, 2, k, dk, device=dev, generator=g).bfloat16()
        index = torch.randint(0, rows, (b, s), device=dev, generator=g, dtype=torch.int32)
        lse, out = bp_hip.sense_lse(qk), torch.empty(b, s, dout, device=dev, dtype=torch.bfloat16)
        legs = {'gather16': lambda: bp_hip.sense_mix_gather(qk, table, index, out=out, lse=lse),
                'gather_mx8': lambda: bp_hip.sense_mix_gather_mx8(qk, q8, s8, index, out=out, lse=lse)}
        times = {name: [] for name in legs}
        for fn in legs.values():
            _time(fn, 3)
        for _ in range(rounds):
            for name, fn in legs.items():
                times[name].append(_time(fn, iters))
        line = {'B': b, 'S': s, 'k': k, 'd_k': dk, 'd_out': dout, 'rows': rows, 'rounds': rounds, 'iters': iters}
        for name, ts in times.items():
            q = statistics.quantiles(ts, n=4)
            line[name] = {'median_ms': round(statistics.median(ts), 4), 'q1_ms': round(q[0], 4), 'q3_ms': round(q[2], 4)}
        line['mx8_over_16'] = round(line['gather_mx8']['median_ms'] / line['gather16']['median_ms'], 3)
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main(sys.argv[1:])
