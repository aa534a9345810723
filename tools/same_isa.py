#!/usr/bin/env python3
"""Is the device code of one source under csrc/ the same as at <rev>?  The check behind a refactor of its kernels.

    python tools/same_isa.py <rev> [source]          (source: a file name under csrc/, default conv.hip)

Compiles the source to device assembly (-S --cuda-device-only) from the working tree and from `git show <rev>:` copies
of csrc/ and include/, with the source's own flags of evreal_amd.build and once per variant where it has several, and
compares the text line for line after normalising the per-file __hip_cuid_<hash> symbol.  Prints `identical` per variant,
or the functions whose bodies differ and, apart, the functions only one side has (a renamed kernel or a changed argument
type is one symbol on each side); exits non-zero on any difference.  A textual comparison only.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from evreal_amd.build import COMMON, HIPCC, PER_FILE, VARIANTS  # noqa: E402

DIRS = ('evreal_amd/csrc', 'include')


def checkout(rev, dst):
    """the files of DIRS at `rev`, under dst"""
    names = subprocess.check_output(['git', 'ls-tree', '-r', '--name-only', rev, '--'] + list(DIRS), cwd=ROOT, text=True).split()
    for n in names:
        os.makedirs(os.path.dirname(os.path.join(dst, n)), exist_ok=True)
        with open(os.path.join(dst, n), 'wb') as f:
            f.write(subprocess.check_output(['git', 'show', f'{rev}:{n}'], cwd=ROOT))


def assemble(tree, src, vflags, out):
    flags = [f for f in COMMON if not f.startswith('-I')] + ['-I' + os.path.join(tree, d) for d in reversed(DIRS)]
    subprocess.check_call([HIPCC, '-S', '--cuda-device-only'] + flags + PER_FILE.get(src, []) + vflags +
                          ['-x', 'hip', os.path.join(tree, DIRS[0], src), '-o', out])
    with open(out) as f:
        return re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_', f.read())


def functions(asm):
    """{symbol: body} of the text split at `.type <sym>,@function`; what precedes the first one is ''"""
    parts = re.split(r'^\s*\.type\s+(\S+),@function.*$', asm, flags=re.M)
    return {'': parts[0], **dict(zip(parts[1::2], parts[2::2]))}


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    src = sys.argv[2] if len(sys.argv) == 3 else 'conv.hip'
    variants = VARIANTS.get(src, [('', [])])
    with tempfile.TemporaryDirectory() as tmp:
        checkout(sys.argv[1], os.path.join(tmp, 'old'))
        trees = {'old': os.path.join(tmp, 'old'), 'new': ROOT}
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            jobs = {(tag, side): pool.submit(assemble, tree, src, vflags, os.path.join(tmp, f'{side}{tag}.s'))
                    for tag, vflags in variants for side, tree in trees.items()}
        differs = False
        for tag, vflags in variants:
            old, new = jobs[tag, 'old'].result(), jobs[tag, 'new'].result()
            label = ' '.join([src] + vflags)
            if old == new:
                print(f'{label}: identical ({old.count(chr(10))} lines)')
                continue
            differs = True
            fo, fn = functions(old), functions(new)
            names = sorted(k or '(outside any function)' for k in fo.keys() & fn.keys() if fo[k] != fn[k])
            same = sum(1 for k in fo.keys() & fn.keys() if k and fo[k] == fn[k])
            print(f'{label}: {same} functions identical, {len(names)} differ' + ''.join('\n  ' + n for n in names))
            one_sided = ((f'only at {sys.argv[1]}', fo.keys() - fn.keys()), ('only in the working tree', fn.keys() - fo.keys()))
            for side, only in one_sided:
                if only:
                    print(f'{label}: {len(only)} functions {side}:' + ''.join('\n  ' + n for n in sorted(only)))
    sys.exit(1 if differs else 0)


if __name__ == '__main__':
    main()
