"""bp_sense_attribute at Backpack-Small dimensions (k = 16, d = 768, d_k = 48, S = 1024, bf16, two vectors per query, every
query at the last position of its own sample) against the torch formulation on the same operands: the query's row of
`bp_hip.sense_alpha`'s (B, k, S, S) output, `table[index]` and an einsum.  The legs alternate in one process; every figure is
the median of `--runs` timed runs (`--iters` back-to-back calls each) with min .. max beside it.  Algorithmic bytes per
query: k (i + 1) (d + d_k) 2 read, 4 nvec k S written.

    python scripts/bench_sense_attribution.py [--nq 1 64] [--runs 5] [--iters 10] [--out FILE.jsonl]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nq', type=int, nargs='+', default=[1, 64])
    ap.add_argument('--seqlen', type=int, default=1024)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import bp_hip
    dev = torch.device('cuda', 0)
    k, d, s, nvec, vocab = 16, 768, a.seqlen, 2, 50264
    dk = d // k
    scale = dk ** -0.5
    g = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(vocab, k, d, device=dev, generator=g).bfloat16()
    lines = []
    for nq in a.nq:
        qk = torch.randn(nq, s, 2, k, dk, device=dev, generator=g).bfloat16()
        index = torch.randint(0, vocab, (nq, s), device=dev, generator=g, dtype=torch.int32)
        qs = torch.arange(nq, dtype=torch.int32, device=dev)
        qp = torch.full((nq,), s - 1, dtype=torch.int32, device=dev)
        vec = torch.randn(nq, nvec, d, device=dev, generator=g)

        def hip():
            return bp_hip.sense_attribute(qk, table, index, qs, qp, vec, scale)[0]

        def torch_leg():
            p = bp_hip.sense_alpha(qk, scale)[qs.long(), :, qp.long(), :].float()             # (nq, k, S)
            content = table[index.long()]                                                    # (nq, S, k, d)
            return p[:, None] * torch.einsum('nslc,nvc->nvls', content.float(), vec)

        diff = (hip() - torch_leg()).abs().max().item()       # the torch leg rounds alpha to bf16: agreement to its rounding only
        times = {'hip': [], 'torch': []}
        for run in range(a.runs + 1):                          # run 0 warms both legs up and is not counted
            for leg, fn in (('hip', hip), ('torch', torch_leg)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    fn()
                torch.cuda.synchronize()
                if run:
                    times[leg].append((time.perf_counter() - t0) * 1e3 / a.iters)
        moved = nq * (k * s * (d + dk) * 2 + 4 * nvec * k * s)
        for leg, ms in times.items():
            med = statistics.median(ms)
            lines.append(dict(workload='sense_attribute', leg=leg, dtype='bf16', nq=nq, nvec=nvec, seqlen=s, nsenses=k, d=d,
                              d_k=dk, query_pos=s - 1, runs=a.runs, iters=a.iters, median_ms=round(med, 4),
                              min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), algorithmic_bytes=moved,
                              algorithmic_gb_per_s=round(moved / med / 1e6, 1), max_abs_diff_between_legs=diff))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(''.join(json.dumps(line) + '\n' for line in lines))


if __name__ == '__main__':
    main()
