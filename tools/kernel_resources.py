"""Per-kernel resource table of csrc/kernels/*.hip, without a GPU.

Compiles every kernel file of a tree for the device only, with the build's
flags (zkmi/ops/_srchash.py HIP_FLAGS), and prints one line per kernel:
the compiler's resource-usage remarks (registers, spills, scratch, static
LDS, occupancy) and the kernel's code size from the device ELF's symbol
table.  Numbers only.

    python tools/kernel_resources.py [--root TREE] [--diff OTHER_TREE]

``--diff`` prints the kernels whose numbers differ between the two trees,
or that only one of them has (whichever file they are in; ``-`` the other
tree's line, ``+`` this one's), and exits 1 if there are any: a change that
leaves every kernel's code alone prints nothing.
"""

import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zkmi.ops._srchash import HIP_FLAGS  # noqa: E402

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
READELF = os.environ.get('READELF', '/opt/rocm/llvm/bin/llvm-readelf')
REMARK = re.compile(r'remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis')
COLS = [('VGPRs', 'VGPRs'), ('AGPRs', 'AGPRs'), ('SGPRs', 'TotalSGPRs'),
        ('vspill', 'VGPRs Spill'), ('sspill', 'SGPRs Spill'),
        ('scratch', 'ScratchSize [bytes/lane]'),
        ('LDS', 'LDS Size [bytes/block]'), ('occ', 'Occupancy [waves/SIMD]')]


def one_file(src, tmp):
    """{mangled kernel name: [file, remark values ..., code bytes]}"""
    elf = os.path.join(tmp, os.path.basename(src) + '.elf')
    r = subprocess.run(
        [HIPCC] + HIP_FLAGS + ['--cuda-device-only', '--no-gpu-bundle-output',
                               '-Rpass-analysis=kernel-resource-usage', '-c',
                               src, '-o', elf],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.exit(src + ': compile failed\n' + r.stdout)
    rem, name = {}, None
    for key, val in REMARK.findall(r.stdout):
        if key == 'Function Name':
            name = val
        rem.setdefault(name, {})[key] = val
    size = {}
    syms = subprocess.run([READELF, '-s', '-W', elf], check=True, text=True,
                          stdout=subprocess.PIPE).stdout
    for f in (ln.split() for ln in syms.splitlines()):
        if len(f) == 8 and f[3] == 'FUNC':
            size[f[7]] = f[2]
    return {k: [os.path.basename(src)] + [v[c] for _, c in COLS] + [size[k]]
            for k, v in rem.items()}


def table(root):
    kdir = os.path.join(root, 'csrc', 'kernels')
    srcs = sorted(os.path.join(kdir, f) for f in os.listdir(kdir)
                  if f.endswith('.hip'))
    out = {}
    with tempfile.TemporaryDirectory() as tmp, \
            cf.ThreadPoolExecutor(max_workers=16) as ex:
        for part in ex.map(lambda s: one_file(s, tmp), srcs):
            dup = set(part) & set(out)
            if dup:
                sys.exit('kernel defined twice: ' + ', '.join(sorted(dup)))
            out.update(part)
    return out


def show(rows):
    """rows: (mangled name, prefix, values); demangled for display"""
    names = subprocess.run(['c++filt'], input='\n'.join(r[0] for r in rows),
                           stdout=subprocess.PIPE, text=True).stdout
    names = names.split('\n')
    print(' '.join(['kernel', 'file'] + [h for h, _ in COLS] + ['code']))
    for (_, pre, vals), n in zip(rows, names):
        n = re.sub(r'^void ', '', n.split('(')[0])
        print(pre + ' '.join(['`%s`' % n] + vals))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--diff', metavar='OTHER_ROOT')
    a = ap.parse_args()
    mine = table(a.root)
    if a.diff is None:
        show([(k, '', v) for k, v in
              sorted(mine.items(), key=lambda kv: (kv[1][0], kv[0]))])
        return 0
    other = table(a.diff)
    rows = []
    for k in sorted(set(mine) | set(other)):
        m, o = mine.get(k), other.get(k)
        if m is None or o is None or m[1:] != o[1:]:
            rows += [(k, s, v) for s, v in (('- ', o), ('+ ', m)) if v]
    if rows:
        show(rows)
    return 1 if rows else 0


if __name__ == '__main__':
    sys.exit(main())
