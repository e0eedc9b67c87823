"""Per-step kernel time of a `rocprofv3 --kernel-trace --output-format csv -- python bench.py` run, by kernel family:

    python scripts/rocprof_per_step.py <trace directory> [--steps 10] [out.txt]

The trace is cut into steps at the sense-mix launch (one per forward); the last `--steps` whole steps are the timed ones.
Per family: median, min, max and min-max spread of the per-step sum of kernel durations -- the figure two builds are
compared by (a family's time changed if the medians differ by more than the spread)."""
import csv
import glob
import os
import statistics
import sys

FAMILIES = (('library GEMM', ('Cijk_',)), ('add+LayerNorm', ('add_layer_norm',)), ('flash forward', ('flash_fwd',)),
            ('sense mix', ('sense_mix',)))


def family(name):
    for fam, keys in FAMILIES:
        if any(k in name for k in keys):
            return fam
    return 'other'


def main(root, steps, out=None):
    rows = []
    for path in glob.glob(os.path.join(root, '**', '*_kernel_trace.csv'), recursive=True):
        for r in csv.DictReader(open(path)):
            rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp']), r['Kernel_Name']))
    if not rows:
        raise SystemExit('no *_kernel_trace.csv under ' + root)
    rows.sort()
    cuts = [i for i, r in enumerate(rows) if 'sense_mix' in r[2]]
    spans = [rows[a:b] for a, b in zip(cuts[:-1], cuts[1:])][-steps:]
    fams = [f for f, _ in FAMILIES] + ['other', 'all kernels']
    per = {f: [] for f in fams}
    launches = {f: set() for f in fams}
    for span in spans:
        sums = dict.fromkeys(fams, 0)
        count = dict.fromkeys(fams, 0)
        for _, dur, name in span:
            for f in (family(name), 'all kernels'):
                sums[f] += dur
                count[f] += 1
        for f in fams:
            per[f].append(sums[f] / 1e6)
            launches[f].add(count[f])
    lines = [f'# per-step kernel time over the last {len(spans)} whole steps of {root} (ms; a step = one sense-mix launch to the next)',
             f'{"family":<16} {"launches":>9} {"median":>10} {"min":>10} {"max":>10} {"spread":>8}']
    for f in fams:
        v = per[f]
        lines.append(f'{f:<16} {"/".join(str(c) for c in sorted(launches[f])):>9} {statistics.median(v):10.3f} {min(v):10.3f} '
                     f'{max(v):10.3f} {max(v) - min(v):8.3f}')
    text = '\n'.join(lines)
    print(text)
    if out:
        open(out, 'w').write(text + '\n')


if __name__ == '__main__':
    args = sys.argv[1:]
    n = 10
    if '--steps' in args:
        i = args.index('--steps')
        n = int(args[i + 1])
        del args[i:i + 2]
    main(args[0], n, args[1] if len(args) > 1 else None)
