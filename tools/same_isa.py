#!/usr/bin/env python3
"""Is the device code of csrc/conv.hip the same as at <rev>?  The check behind a refactor of the conv kernels.

    python tools/same_isa.py <rev>

Compiles conv.hip to device assembly (-S --cuda-device-only) from the working tree and from `git show <rev>:` copies
of csrc/ and include/, once per arithmetic variant and with the flags of evreal_amd.build, and compares the text line
for line after normalising the per-file __hip_cuid_<hash> symbol.  Prints `identical` per variant, or the functions
whose bodies differ; exits non-zero on any difference.  A textual comparison only.
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

SRC = 'conv.hip'
DIRS = ('evreal_amd/csrc', 'include')


def checkout(rev, dst):
    """the files of DIRS at `rev`, under dst"""
    names = subprocess.check_output(['git', 'ls-tree', '-r', '--name-only', rev, '--'] + list(DIRS), cwd=ROOT, text=True).split()
    for n in names:
        os.makedirs(os.path.dirname(os.path.join(dst, n)), exist_ok=True)
        with open(os.path.join(dst, n), 'wb') as f:
            f.write(subprocess.check_output(['git', 'show', f'{rev}:{n}'], cwd=ROOT))


def assemble(tree, vflags, out):
    flags = [f for f in COMMON if not f.startswith('-I')] + ['-I' + os.path.join(tree, d) for d in reversed(DIRS)]
    subprocess.check_call([HIPCC, '-S', '--cuda-device-only'] + flags + PER_FILE.get(SRC, []) + vflags +
                          ['-x', 'hip', os.path.join(tree, DIRS[0], SRC), '-o', out])
    with open(out) as f:
        return re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_', f.read())


def functions(asm):
    """{symbol: body} of the text split at `.type <sym>,@function`; what precedes the first one is ''"""
    parts = re.split(r'^\s*\.type\s+(\S+),@function.*$', asm, flags=re.M)
    return {'': parts[0], **dict(zip(parts[1::2], parts[2::2]))}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        checkout(sys.argv[1], os.path.join(tmp, 'old'))
        trees = {'old': os.path.join(tmp, 'old'), 'new': ROOT}
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            jobs = {(tag, side): pool.submit(assemble, tree, vflags, os.path.join(tmp, f'{side}{tag}.s'))
                    for tag, vflags in VARIANTS[SRC] for side, tree in trees.items()}
        differs = False
        for tag, vflags in VARIANTS[SRC]:
            old, new = jobs[tag, 'old'].result(), jobs[tag, 'new'].result()
            if old == new:
                print(f'{" ".join(vflags)}: identical ({old.count(chr(10))} lines)')
                continue
            differs = True
            fo, fn = functions(old), functions(new)
            names = sorted(k or '(outside any function)' for k in fo.keys() | fn.keys() if fo.get(k) != fn.get(k))
            print(f'{" ".join(vflags)}: {len(names)} functions differ:\n  ' + '\n  '.join(names))
    sys.exit(1 if differs else 0)


if __name__ == '__main__':
    main()
