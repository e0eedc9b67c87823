"""Measure, per large GEMM shape of the Backpack-Small forward, whether a hipBLASLt solution other than the heuristic's first
pick is worth pinning, and write the table bp_hip.linear reads (backpacks-flash-attn_amd/bp_hip/gemm_solutions.json).

    python scripts/tune_gemm.py --jsonl profiles/gemm_pin_tune.jsonl
    python scripts/tune_gemm.py --report            # heuristic against pinned, ms and TF/s, for every row of the shipped table

Per shape: the heuristic's first 256 candidates (bp_gemm_heuristic) plus the call torch makes for that layer; a short
screening pass on the first 262 144 rows keeps the fastest few; those, the first pick and torch's call are then timed INTERLEAVED -- one launch of
each per round, each between its own pair of events, on one stream, random operands, warm clocks.  A candidate enters
the table only if its median beats the first pick's median by more than the first pick's own min-max spread over the
same rounds (and torch's call by more than torch's spread: the model would otherwise lose what torch's pick has over the
first candidate).  The bound is computed per shape and written next to the entry; nothing here is a percentage.

Rows apply from 131 072 rows up (the LM head's chunked forms from their own row count): nothing smaller is rerouted.
Configuration measured once, not tuning at run time: the model only ever reads the table."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'backpacks-flash-attn_amd')]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bp_hip  # noqa: E402
from bp_hip import gemm  # noqa: E402

VOCAB = 50264        # GPT-2's 50257 padded to a multiple of 8
# name, epilogue, N, K, row counts (None: --m), m_min of the row written (None: the measured row count)
SHAPES = [('trunk Wqkv', 'bias', 2304, 768, None, gemm.M_BUCKET_MIN),
          ('trunk out_proj', 'bias', 768, 768, None, gemm.M_BUCKET_MIN),
          ('trunk fc1 + GELU', 'bias_gelu', 3072, 768, None, gemm.M_BUCKET_MIN),
          ('trunk fc2', 'bias', 768, 3072, None, gemm.M_BUCKET_MIN),
          ('sense Wqkv', 'bias', 1536, 768, None, gemm.M_BUCKET_MIN),
          ('lm_head', 'none', VOCAB, 768, (262144, 524288, None), None)]


def say(f, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if f is not None:
        f.write(line + '\n')
        f.flush()


def one_row_table(version, arch, dtype, epilogue, n, k, solution):
    return bp_hip.GemmTable({'library_version': version, 'arch': arch, 'entries': [
        dict(dtype=dtype, epilogue=epilogue, n=n, k=k, m_min=1, solution=solution)]})


def torch_call(epilogue, x, w, b, out):
    """The call the model makes for this layer without a table row."""
    if epilogue == 'bias_gelu':
        return lambda: torch._addmm_activation(b, x, w.t(), use_gelu=True)
    if epilogue == 'bias':
        return lambda: F.linear(x, w, b)
    return lambda: torch.mm(x, w.t(), out=out)


def rounds(calls, n):
    """n interleaved rounds over `calls` (name -> fn): ms per call, per name."""
    times = {name: [] for name in calls}
    for _ in range(n):
        evs = []
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs.append((name, e0, e1))
        torch.cuda.synchronize()
        for name, e0, e1 in evs:
            times[name].append(e0.elapsed_time(e1))
    return times


def measure(f, a, name, epilogue, n, k, m, big, version, arch, dev):
    """Time one shape; returns the summary dict of the first pick, torch's call and the best candidate."""
    dtype = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(1234)
    x = torch.randn(m, k, device=dev, dtype=dtype, generator=g)
    w = torch.randn(n, k, device=dev, dtype=dtype, generator=g) * 0.02
    b = torch.randn(n, device=dev, dtype=dtype, generator=g) if epilogue != 'none' else None
    out = big[:m * n].view(m, n)
    ref_call = torch_call(epilogue, x, w, b, out)
    check_rows = min(m, 512)
    ref = ref_call()[:check_rows].float().clone()
    cands = []
    for s in gemm.heuristic(dtype, epilogue, m, n, k, count=a.candidates):
        if s >= 0 and s not in cands:
            cands.append(s)
    gelu = epilogue == 'bias_gelu'

    def admit(s, rows):
        """A call of solution s on the first `rows` rows, or None with the reason in `skipped`."""
        t = one_row_table(version, arch, 'bf16', epilogue, n, k, s)
        xs, outs = x[:rows], out[:rows]
        outs[:check_rows].zero_()
        status = gemm.pinned(xs, w, b, gelu, outs, t)
        diff = (outs[:check_rows].float() - ref).abs().max().item() if status == 'ran' else None
        if status != 'ran' or not diff <= 0.02 * ref.abs().max().item() + 1e-3:
            skipped.append(dict(solution=s, rows=rows, status=status, max_abs_diff_vs_torch=diff))
            return None
        return lambda: gemm.pinned(xs, w, b, gelu, outs, t)

    # screening on the first --screen-m rows (every candidate, a few launches each), the final comparison on all rows
    screen_m = min(m, a.screen_m)
    calls, skipped = {}, []
    for s in cands:
        fn = admit(s, screen_m)
        if fn is not None:
            calls[s] = fn
    if not cands or cands[0] not in calls:
        say(f, what='shape skipped', gemm=name, m=m, n=n, k=k, reason='the first pick did not run', skipped=skipped)
        return None
    first = cands[0]
    rounds(calls, 1)                                   # warm every candidate's code object
    screen = rounds(calls, a.screen_reps)
    order = sorted(calls, key=lambda s: statistics.median(screen[s]))
    final_calls = {'torch': ref_call}
    for s in [first] + [s for s in order if s != first][:a.finalists]:
        fn = admit(s, m)
        if fn is not None:
            final_calls[s] = fn
    keep = [s for s in final_calls if s != 'torch']
    if first not in keep:
        say(f, what='shape skipped', gemm=name, m=m, n=n, k=k, reason='the first pick did not run on all rows', skipped=skipped)
        return None
    rounds(final_calls, 2)
    times = rounds(final_calls, a.reps)
    med = {s: statistics.median(v) for s, v in times.items()}
    spread = {s: max(v) - min(v) for s, v in times.items()}
    flops = 2.0 * m * n * k
    best = min((s for s in keep if s != first), key=lambda s: med[s], default=None)
    wins = (best is not None and med[first] - med[best] > spread[first] and med['torch'] - med[best] > spread['torch'])
    res = dict(what='shape', gemm=name, dtype='bf16', epilogue=epilogue, m=m, n=n, k=k, n_per_candidate=a.reps,
               candidates=len(cands), screened=len(calls), screen_m=screen_m, first_pick=first, first_pick_ms=round(med[first], 4),
               first_pick_spread_ms=round(spread[first], 4), first_pick_tflops=round(flops / med[first] / 1e9, 1),
               torch_ms=round(med['torch'], 4), torch_spread_ms=round(spread['torch'], 4),
               best_other=best, best_other_ms=round(med[best], 4) if best is not None else None,
               best_other_tflops=round(flops / med[best] / 1e9, 1) if best is not None else None,
               gain_ms=round(med[first] - med[best], 4) if best is not None else None,
               decision='pin' if wins else 'keep the heuristic',
               finalists={str(s): dict(median_ms=round(med[s], 4), min_ms=round(min(times[s]), 4), max_ms=round(max(times[s]), 4))
                          for s in final_calls},
               screening={str(s): round(statistics.median(screen[s]), 4) for s in order[:48]}, skipped=skipped[:16])
    say(f, **res)
    del x, w, b, out, ref
    return res


def tune(a):
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    version, arch = gemm.library()
    os.makedirs(os.path.dirname(os.path.abspath(a.jsonl)), exist_ok=True)
    f = open(a.jsonl, 'w')
    say(f, what='library', hipblaslt_version=version, arch=arch, torch=torch.__version__, hip=torch.version.hip,
        device=torch.cuda.get_device_name(0), m=a.m, reps=a.reps, screen_reps=a.screen_reps, candidates=a.candidates)
    only = set(a.only.split(',')) if a.only else None
    shapes = [s for s in SHAPES if only is None or s[0] in only]
    biggest = max(n * (mm or a.m) for _, _, n, _, ms, _ in shapes for mm in (ms or (None,)))
    big = torch.empty(biggest, device=dev, dtype=torch.bfloat16)
    # warm clocks: a second of GEMMs before the first timed launch
    xw, ww = torch.randn(65536, 768, device=dev, dtype=torch.bfloat16), torch.randn(3072, 768, device=dev, dtype=torch.bfloat16)
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(3000):
        xw @ ww.t()
    t1.record()
    torch.cuda.synchronize()
    say(f, what='warm-up', ms=round(t0.elapsed_time(t1), 1))
    del xw, ww
    entries, results = [], {}
    for name, epilogue, n, k, ms, m_min in shapes:
        for mm in (ms or (None,)):
            m = mm or a.m
            res = measure(f, a, name, epilogue, n, k, m, big, version, arch, dev)
            if res is None:
                continue
            results[(name, m)] = res
            pin = res['decision'] == 'pin'
            entries.append(dict(name=name, dtype='bf16', epilogue=epilogue, n=n, k=k, m_min=m_min or m, measured_m=m,
                                solution=res['best_other'] if pin else None, decision=res['decision'],
                                library_version=version, arch=arch, heuristic_solution=res['first_pick'],
                                heuristic_ms=res['first_pick_ms'], spread_ms=res['first_pick_spread_ms'],
                                torch_ms=res['torch_ms'], torch_spread_ms=res['torch_spread_ms'],
                                pinned_ms=res['best_other_ms'] if pin else None, gain_ms=res['gain_ms'] if pin else 0.0,
                                n_per_candidate=a.reps))
    # the LM head at --m rows: one GEMM against row chunks, each at its best admitted form
    chunk_rows = {}
    single = results.get(('lm_head', a.m))
    if single is not None:
        def admitted_ms(r):
            return r['best_other_ms'] if r['decision'] == 'pin' else min(r['first_pick_ms'], r['torch_ms'])
        best_rows, best_ms = 0, admitted_ms(single)
        for (name, m), r in results.items():
            if name != 'lm_head' or m == a.m or a.m % m:
                continue
            total = admitted_ms(r) * (a.m // m)
            say(f, what='lm_head chunking', rows=m, chunks=a.m // m, chunked_ms=round(total, 3), single_ms=round(admitted_ms(single), 3),
                single_first_pick_spread_ms=single['first_pick_spread_ms'])
            if admitted_ms(single) - total > single['first_pick_spread_ms'] and total < best_ms:
                best_rows, best_ms = m, total
        chunk_rows[str(a.m)] = best_rows
    table = dict(comment='written by scripts/tune_gemm.py: hipBLASLt solutions measured to beat the heuristic\'s first pick by more '
                         'than that pick\'s own spread (spread_ms, same run); solution null = keep the heuristic',
                 library_version=version, arch=arch, m_bucket_min=gemm.M_BUCKET_MIN, lm_head_chunk_rows=chunk_rows, entries=entries)
    os.makedirs(os.path.dirname(os.path.abspath(a.table)), exist_ok=True)
    with open(a.table, 'w') as t:
        json.dump(table, t, indent=1)
        t.write('\n')
    say(f, what='table written', path=a.table, pinned=[e['name'] + ' m>=' + str(e['m_min']) for e in entries if e['solution'] is not None],
        lm_head_chunk_rows=chunk_rows)
    f.close()


def report(a):
    """Heuristic (the torch call) against the pinned solution for every row of the shipped table, interleaved."""
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    table = gemm.shipped_table()
    for e in table.spec.get('entries', ()):
        if e.get('solution') is None:
            print(json.dumps(dict(gemm=e['name'], m=e['measured_m'], n=e['n'], k=e['k'], decision='keep the heuristic',
                                  heuristic_ms=e['heuristic_ms'], spread_ms=e['spread_ms'])), flush=True)
            continue
        m, n, k = int(e['measured_m']), int(e['n']), int(e['k'])
        x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
        w = torch.randn(n, k, device=dev, dtype=torch.bfloat16) * 0.02
        b = torch.randn(n, device=dev, dtype=torch.bfloat16) if e['epilogue'] != 'none' else None
        out = torch.empty(m, n, device=dev, dtype=torch.bfloat16)
        one = bp_hip.GemmTable(dict(table.spec, entries=[dict(e, m_min=1)]))
        calls = {'heuristic': torch_call(e['epilogue'], x, w, b, out),
                 'pinned': lambda: gemm.pinned(x, w, b, e['epilogue'] == 'bias_gelu', out, one)}
        status = calls['pinned']()
        if status != 'ran':
            print(json.dumps(dict(gemm=e['name'], m=m, status=status)), flush=True)
            continue
        rounds(calls, 3)
        t = rounds(calls, a.reps)
        fl = 2.0 * m * n * k
        print(json.dumps(dict(gemm=e['name'], m=m, n=n, k=k, **{
            key + '_ms': round(statistics.median(v), 4) for key, v in t.items()}, **{
            key + '_tflops': round(fl / statistics.median(v) / 1e9, 1) for key, v in t.items()})), flush=True)
        del x, w, b, out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--m', type=int, default=2097152, help='rows of the activations (batch x sequence of the headline run)')
    ap.add_argument('--candidates', type=int, default=256, help='heuristic candidates asked for per shape')
    ap.add_argument('--screen-reps', type=int, default=3)
    ap.add_argument('--screen-m', type=int, default=262144, help='rows of the screening pass')
    ap.add_argument('--finalists', type=int, default=8)
    ap.add_argument('--reps', type=int, default=12, help='interleaved rounds of the final comparison (n per candidate)')
    ap.add_argument('--only', default=None, help='comma-separated shape names')
    ap.add_argument('--jsonl', default='profiles/gemm_pin_tune.jsonl')
    ap.add_argument('--table', default=gemm.TABLE_PATH)
    ap.add_argument('--report', action='store_true')
    args = ap.parse_args()
    report(args) if args.report else tune(args)
