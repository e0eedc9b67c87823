"""Did a change of the sources change the generated gfx950 code?  Compares two builds kernel by kernel.

    python scripts/isa_diff.py BUILD_A BUILD_B [OBJECT.o ...]

BUILD_A / BUILD_B are two `csrc/build` directories (say, of a worktree of the parent commit and of this tree); without a
list of objects, every `*.o` that either holds.  Per kernel it prints `same` or `differs`, with the first instruction of
each side that does not match; the exit status is 1 when anything differs or is missing on one side.

The device code is reached as scripts/kernel_resources.py reaches it (llvm-objcopy the `.hip_fatbin` section,
clang-offload-bundler --unbundle), then `llvm-objdump -d --mcpu=gfx950`.  What is compared is the instruction text per
function symbol of `.text`: the address and encoding that objdump prints behind `//` are dropped, and with them the
absolute form of a branch target -- the operand of a branch is already its distance in words, so a kernel compares
equal to itself wherever it lands in the code object.  The tool looks for no instruction in particular; it compares.
"""
import glob
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr   # noqa: E402


def tools_available():
    return kr.tools_available() and os.path.exists(os.path.join(kr.LLVM, 'llvm-objdump'))


def disassemble(obj):
    """{mangled symbol: [instruction text, ...]} of the gfx950 code object embedded in `obj` ({} for a host-only object)."""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, 'fat.bin'), os.path.join(tmp, 'dev.co')
        if '.hip_fatbin' not in kr._run(os.path.join(kr.LLVM, 'llvm-readelf'), '-S', obj):
            return {}
        kr._run(os.path.join(kr.LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, obj)
        kr._run(os.path.join(kr.LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=' + kr.TARGET,
                '--input=' + fat, '--output=' + co)
        text = kr._run(os.path.join(kr.LLVM, 'llvm-objdump'), '-d', '--mcpu=gfx950', co)
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith('\t'):
            inst, _, tail = line.partition('//')
            cur.append((' '.join(inst.split()), tail.split(':')[-1].split('<')[0].split()))
    for name, insts in out.items():
        # what fills the gap up to the next function belongs to neither: s_nop 0, s_code_end, zero words (which objdump
        # prints as `...` or decodes as an instruction of its own)
        while insts and all(w in ('00000000', 'BF800000', 'BF9F0000') for w in insts[-1][1]):
            insts.pop()
        out[name] = [text for text, _ in insts]
    return out


def diff_object(obj_a, obj_b):
    """[{name, object, same, a, b}] per function symbol of the two objects; a / b: (index, text) of the first instruction
    that differs (None where a side ends first, or lacks the symbol)."""
    da, db = disassemble(obj_a), disassemble(obj_b)
    rows = []
    for name in sorted(set(da) | set(db)):
        ia, ib = da.get(name), db.get(name)
        row = {'name': name, 'object': os.path.basename(obj_a), 'same': ia == ib, 'a': None, 'b': None}
        if not row['same'] and ia is not None and ib is not None:
            at = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            row['a'] = (at, ia[at]) if at < len(ia) else None
            row['b'] = (at, ib[at]) if at < len(ib) else None
        row['missing'] = 'a' if ia is None else 'b' if ib is None else None
        rows.append(row)
    return rows


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    build_a, build_b, objects = argv[0], argv[1], argv[2:]
    if not objects:
        objects = sorted({os.path.basename(f) for d in (build_a, build_b) for f in glob.glob(os.path.join(d, '*.o'))})
    bad = 0
    for obj in objects:
        a, b = os.path.join(build_a, obj), os.path.join(build_b, obj)
        if not (os.path.exists(a) and os.path.exists(b)):
            print('%-20s only in %s' % (obj, build_a if os.path.exists(a) else build_b))
            bad += 1
            continue
        for r in diff_object(a, b):
            print('%-20s %-8s %s' % (obj, 'same' if r['same'] else 'differs', r['name']))
            if r['same']:
                continue
            bad += 1
            if r['missing']:
                print('    not in build %s' % r['missing'].upper())
                continue
            for side in ('a', 'b'):
                print('    %s: %s' % (side.upper(), '[%d] %s' % r[side] if r[side] else 'ends first'))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main(sys.argv[1:])
