"""The session batches' segment rule on the host: csrc/kernels/zk_sess.h
(sess_seg, sess_torn, sess_first — the text the kernels of
csrc/kernels/tree_sess.hip run) compiled by g++ into tools/sess_host.cpp with
ASan + UBSan, a stand-alone program.  Every table sits in a heap block of
exactly its length; the output is compared with numpy's searchsorted — on a
machine without a GPU."""

import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _have_asan():
    if shutil.which('gcc') is None or shutil.which('g++') is None:
        return False
    lib = subprocess.run(['gcc', '-print-file-name=libasan.so'],
                         capture_output=True, text=True).stdout.strip()
    return os.path.isabs(lib) and os.path.exists(lib)


pytestmark = [
    pytest.mark.slow,
    pytest.mark.skipif(not _have_asan(), reason='no g++ ASan runtime'),
    pytest.mark.skipif(torch.cuda.is_available(),
                       reason='sanitizer runs belong on the CPU box'),
]


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('sess') / 'sess_host')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'sess_host.cpp'), '-o', exe],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(prog, cases, tmp_path):
    """cases: (starts, off, len) -> [(f_seg, first, bad, first_bad)]"""
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as f:
        for starts, off, ln in cases:
            f.write(struct.pack('<qq', len(starts) - 1, len(off)))
            f.write(np.asarray(starts, np.int64).tobytes())
            f.write(np.asarray(off, np.int64).tobytes())
            f.write(np.asarray(ln, np.int32).tobytes())
    env = {k: v for k, v in os.environ.items() if k != 'LD_PRELOAD'}
    r = subprocess.run([prog, path], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.split('\n')
    assert len(lines) >= 3 * len(cases)
    out = []
    for k in range(len(cases)):
        seg = [int(x) for x in lines[3 * k].split()]
        first = [int(x) for x in lines[3 * k + 1].split()]
        bad, fb = (int(x) for x in lines[3 * k + 2].split())
        out.append((seg, first, bad, fb))
    return out


def _frames(sizes, at=0):
    """Frame table of back-to-back frames of `sizes` body bytes from `at`."""
    off, o = [], at
    for n in sizes:
        off.append(o + 4)
        o += 4 + n
    return off, list(sizes), o


def _bisect_seg(starts, S, h):
    """The rule's own search (for a table that is not sorted, where
    searchsorted promises nothing)."""
    lo, hi = 0, S
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if starts[mid] <= h:
            lo = mid + 1
        else:
            hi = mid
    return lo - 1


def want(starts, off, ln):
    """The issue's rule with numpy: f_seg, first, bad."""
    starts = np.asarray(starts, np.int64)
    S = len(starts) - 1
    h = np.asarray(off, np.int64) - 4
    e = np.asarray(off, np.int64) + np.asarray(ln, np.int64)
    if np.all(np.diff(starts) >= 0):
        seg = np.minimum(np.searchsorted(starts, h, 'right') - 1, S - 1)
    else:
        seg = np.array([_bisect_seg(starts, S, int(x)) for x in h], np.int64)
    first = np.searchsorted(h, starts, 'left')
    torn = [int(s) < 0 or int(x) > int(starts[int(s) + 1])
            for s, x in zip(seg, e)]
    bad = sum(torn) + int(np.sum(starts[:-1] > starts[1:])) + \
        int(starts[0] != 0)
    return [int(x) for x in seg], [int(x) for x in first], bad


def _check(prog, cases, tmp_path):
    got = _run(prog, cases, tmp_path)
    for k, (c, g) in enumerate(zip(cases, got)):
        seg, first, bad = want(*c)
        assert g[0] == seg, (k, c[0][:8], g[0][:16], seg[:16])
        assert g[1] == first, (k, c[0][:8], g[1][:16], first[:16])
        assert g[2] == bad, (k, g[2], bad)
        assert (g[3] >= 0) == (bad > 0), (k, g)
    return got


def test_named_cases(prog, tmp_path):
    off, ln, end = _frames([8, 12, 30, 9, 8, 100, 8])
    b = [o - 4 for o in off] + [end]       # the frame boundaries
    cases = [
        # S = 1
        ([0, end], off, ln),
        # S larger than the frame count (most segments empty)
        ([0] + [b[min(k // 3, 7)] for k in range(1, 24)] + [end], off, ln),
        # empty segments first, last, and three in a row
        ([0, 0, b[2], end], off, ln),
        ([0, b[2], end, end], off, ln),
        ([0, b[1], b[1], b[1], b[1], b[4], end], off, ln),
        # no frames at all
        ([0, 0], [], []),
        ([0, 0, 0, 0], [], []),
        ([0, 10, 20], [], []),
        # a boundary inside a frame's length word, and one inside its body
        ([0, b[2] + 2, end], off, ln),
        ([0, b[2] + 11, end], off, ln),
        ([0, b[5] + 4, end], off, ln),
        # frames past starts[S]
        ([0, b[2], b[4]], off, ln),
        ([0, b[3] + 1], off, ln),
        # starts[0] = 4
        ([4, b[2], end], off, ln),
        # a descending pair
        ([0, b[4], b[2], end], off, ln),
        ([0, end, 0], off, ln),
    ]
    got = _check(prog, cases, tmp_path)
    # the sound ones are sound, the others are not
    for k in range(0, 8):
        assert got[k][2] == 0 and got[k][3] == -1, (k, got[k])
        assert got[k][1][-1] == len(cases[k][1])
    for k in range(8, len(cases)):
        assert got[k][2] > 0, (k, got[k])
    # a boundary in frame 2 tears that frame alone; it is segment 0's
    assert got[8][2] == 1 and got[8][3] == 0 and got[8][0][2] == 0
    assert got[9][2] == 1 and got[10][2] == 1
    # frames 4.. lie past starts[S]: each is torn, in the last segment
    assert got[11][2] == 3 and got[11][0][4:] == [1, 1, 1]
    # starts[0] = 4: frame 0 has no segment
    assert got[13][0][0] == -1 and got[13][2] == 2
    # among equal starts the last segment owns the frames
    assert got[4][0][1] == 4 and got[4][1][1:5] == [1, 1, 1, 1]


def test_random_sound_tables(prog, tmp_path):
    rng = np.random.RandomState(7)
    cases = []
    for k in range(1000):
        nf = int(rng.randint(0, 40))
        off, ln, end = _frames([int(x) for x in rng.randint(0, 60, nf)])
        b = [o - 4 for o in off] + [end]
        S = int(rng.randint(1, 60))
        cut = np.sort(rng.randint(0, len(b), S - 1))
        starts = [0] + [b[int(c)] for c in cut] + [end]
        cases.append((starts, off, ln))
    got = _check(prog, cases, tmp_path)
    for c, g in zip(cases, got):
        assert g[2] == 0 and g[3] == -1
        assert g[1][-1] == len(c[1])
        # every frame lies inside its segment
        for j, s in enumerate(g[0]):
            assert c[0][s] <= c[1][j] - 4
            assert c[1][j] + c[2][j] <= c[0][s + 1]
