"""The rules of a session batch of any op mix on the host:
csrc/kernels/zk_sess.h (sess_refusal, sess_split_at, sess_xid — the text the
session instances of the list and GET_ACL engines and sess_split_seg_k run)
compiled by g++ into tools/sess_mix_host.cpp with ASan + UBSan, a stand-alone
program.  Every table sits in a heap block of exactly its length, so a read
of seg_state or a write of a class table outside it is a sanitizer report;
the output is compared with a Python mirror — on a machine without a GPU."""

import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, SYSTEM, EXPIRED = 0, -1, -112
INT32_MAX = 2 ** 31 - 1
INT32_MIN = -2 ** 31


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
    exe = str(tmp_path_factory.mktemp('sessmix') / 'sess_mix_host')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'sess_mix_host.cpp'), '-o', exe],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _case(S, ncap, bad, seg_state, f_seg, cls, sub, bodies=None):
    n = len(f_seg)
    assert len(seg_state) == S and len(cls) == n and len(sub) == n
    if bodies is None:
        bodies = [struct.pack('>ii', 100 + i, 8) for i in range(n)]
    return dict(S=S, ncap=ncap, bad=bad, seg_state=list(seg_state),
                f_seg=list(f_seg), cls=list(cls), sub=list(sub),
                bodies=list(bodies))


def _run(prog, cases, tmp_path):
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as f:
        for c in cases:
            f.write(struct.pack('<qqqq', c['S'], len(c['f_seg']), c['ncap'],
                                c['bad']))
            for k in ('seg_state', 'f_seg', 'cls', 'sub'):
                f.write(np.asarray(c[k], np.int32).tobytes())
            for b in c['bodies']:
                assert len(b) <= 8
                f.write(struct.pack('<i', len(b)) + b.ljust(8, b'\xee'))
    env = {k: v for k, v in os.environ.items() if k != 'LD_PRELOAD'}
    r = subprocess.run([prog, path], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.split('\n')
    assert len(lines) >= 3 * len(cases)
    return [tuple([int(x) for x in lines[3 * k + j].split()]
                  for j in range(3)) for k in range(len(cases))]


# ---- the Python mirror ------------------------------------------------------

def want_refusal(c):
    out = []
    for sg in c['f_seg']:
        if c['bad'] != 0 or not 0 <= sg < c['S']:
            out.append(SYSTEM)
        else:
            out.append(EXPIRED if c['seg_state'][sg] == 1 else OK)
    return out


def want_xid(c):
    return [struct.unpack('>i', b[:4])[0] if len(b) >= 8 else 0
            for b in c['bodies']]


def want_tables(c):
    ncap = c['ncap']
    tab = [-7] * (3 * ncap)
    for i in range(min(len(c['f_seg']), ncap)):
        k, j = c['cls'][i], c['sub'][i]
        if 0 <= k <= 2 and 0 <= j < ncap:
            tab[k * ncap + j] = c['f_seg'][i]
    return tab


def _check(prog, cases, tmp_path):
    got = _run(prog, cases, tmp_path)
    for k, (c, g) in enumerate(zip(cases, got)):
        assert g[0] == want_refusal(c), (k, g[0][:16])
        assert g[1] == want_xid(c), (k, g[1][:16])
        assert g[2] == want_tables(c), (k, g[2][:32])
    return got


def test_named_cases(prog, tmp_path):
    S, ncap = 4, 8
    state = [0, 1, 0, 2]
    seg = [0, 1, 2, 3, 3, 0]
    cls = [0, 2, 1, 2, 0, 1]
    sub = [0, 0, 0, 1, 1, 1]
    cases = [
        # 0: a sound table: segment 1 is expired, state 2 is no refusal
        _case(S, ncap, 0, state, seg, cls, sub),
        # 1: an unsound table refuses every frame, the tables are written
        _case(S, ncap, 3, state, seg, cls, sub),
        _case(S, ncap, -1, state, seg, cls, sub),
        # 3: hostile segments: none is read from seg_state
        _case(S, ncap, 0, state, [-1, S, INT32_MAX, INT32_MIN, S - 1, 0],
              cls, sub),
        # 4: hostile classes: nothing is written for them
        _case(S, ncap, 0, state, seg, [3, -1, INT32_MAX, INT32_MIN, 2, 0],
              sub),
        # 5: hostile indices
        _case(S, ncap, 0, state, seg, cls,
              [ncap, -1, INT32_MAX, INT32_MIN, ncap - 1, 0]),
        # 6: the last place of the last table, and one past it
        _case(S, ncap, 0, state, [1, 2], [2, 2], [ncap - 1, ncap]),
        # 7: more frames than the tables hold: the rest is not walked
        _case(1, 2, 0, [0], [0, 0, 0, 0], [0, 1, 2, 2], [0, 0, 0, 1]),
        # 8: no frames, no room
        _case(1, 0, 0, [1], [], [], []),
        _case(2, 0, 0, [0, 0], [0, 1], [0, 0], [0, 0]),
        # 10: S = 1
        _case(1, 4, 0, [1], [0, 1, -1], [0, 1, 2], [0, 0, 0]),
        # 11: bodies without an xid word (0..7 bytes) and with one
        _case(1, 8, 0, [0], [0] * 9, [0] * 9, list(range(8)) + [8],
              [b'\x7f' * k for k in range(8)] +
              [struct.pack('>ii', -8, 101)]),
    ]
    got = _check(prog, cases, tmp_path)
    assert got[0][0] == [OK, EXPIRED, OK, OK, OK, OK]
    assert got[1][0] == [SYSTEM] * 6 and got[2][0] == [SYSTEM] * 6
    assert got[1][2] == got[0][2]
    assert got[3][0] == [SYSTEM] * 4 + [OK, OK]
    # classes 3, -1, ...: four frames have no place
    assert sum(x != -7 for x in got[4][2]) == 2
    assert sum(x != -7 for x in got[5][2]) == 2
    assert got[6][2] == [-7] * (3 * ncap - 1) + [1]
    assert got[7][2] == [0, -7, 0, -7, -7, -7]
    assert got[8][2] == [] and got[9][2] == []
    assert got[11][1] == [0] * 8 + [-8]


def test_random_tables(prog, tmp_path):
    """Sound tables (a stable split of random classes) and tables with
    hostile values mixed in."""
    rng = np.random.RandomState(23)
    edge = [-1, INT32_MAX, INT32_MIN, 3]
    cases = []
    for k in range(600):
        S = int(rng.randint(1, 70))
        n = int(rng.randint(0, 80))
        ncap = int(rng.randint(max(n - 3, 0), n + 4))
        state = [int(x) for x in rng.randint(0, 2, S)]
        seg = [int(x) for x in rng.randint(0, S, n)]
        cls = [int(x) for x in rng.randint(0, 3, n)]
        cnt = [0, 0, 0]
        sub = []
        for c in cls:
            sub.append(cnt[c])
            cnt[c] += 1
        if k % 3 == 1:
            for _ in range(1 + n // 8):
                if n == 0:
                    break
                i = int(rng.randint(0, n))
                which = int(rng.randint(0, 3))
                v = [edge + [S, S + 1], edge, edge + [ncap, ncap + 1]][which]
                (seg, cls, sub)[which][i] = int(v[int(rng.randint(len(v)))])
        cases.append(_case(S, ncap, int(k % 5 == 4), state, seg, cls, sub))
    got = _check(prog, cases, tmp_path)
    for k, (c, g) in enumerate(zip(cases, got)):
        if k % 3 != 1 and len(c['f_seg']) <= c['ncap']:
            # sound: every frame has a place of its own, class by class in
            # request order
            for cl in range(3):
                mine = [s for s, x in zip(c['f_seg'], c['cls']) if x == cl]
                lo = cl * c['ncap']
                assert g[2][lo:lo + len(mine)] == mine
                assert set(g[2][lo + len(mine):lo + c['ncap']]) <= {-7}
