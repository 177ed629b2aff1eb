"""The rules of closing many sessions in one pass on the host:
csrc/kernels/zk_close.h (close_frame, the set of closing session ids,
close_drop_mask — the text tree_close.hip runs) compiled by g++ into
tools/close_host.cpp with ASan + UBSan, a stand-alone program run as a child
process with nothing preloaded.  Every table — the set's key and rank arrays
included — and every frame sits in a heap block of exactly its length, so a
read past one is a sanitizer report; the output is compared with a Python
mirror, on a machine without a GPU."""

import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOSE_SESSION = -11
INT32_MAX = 2 ** 31 - 1
INT32_MIN = -2 ** 31
M64 = (1 << 64) - 1


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
    exe = str(tmp_path_factory.mktemp('close') / 'close_host')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'close_host.cpp'), '-o', exe],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def body(op=CLOSE_SESSION, xid=77, tail=b''):
    return struct.pack('>ii', xid, op) + tail


def _case(frame=None, S=2, seg=0, bad=0, seg_state=(0, 0), ids=(), cap=0,
          query=(), wslots=()):
    assert len(seg_state) == S
    return dict(frame=body() if frame is None else frame, S=S, seg=seg,
                bad=bad, seg_state=list(seg_state), ids=list(ids), cap=cap,
                query=list(query), wslots=list(wslots))


def _run(prog, cases, tmp_path):
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as f:
        for c in cases:
            f.write(struct.pack('<8q', c['S'], c['seg'], c['bad'],
                                len(c['frame']), len(c['ids']), c['cap'],
                                len(c['query']), len(c['wslots'])))
            f.write(np.asarray(c['seg_state'], np.int32).tobytes())
            f.write(c['frame'])
            f.write(np.asarray(c['ids'], np.int64).tobytes())
            f.write(np.asarray(c['query'], np.int64).tobytes())
            f.write(np.asarray(c['wslots'], np.int32).tobytes())
    env = {k: v for k, v in os.environ.items() if k != 'LD_PRELOAD'}
    r = subprocess.run([prog, path], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.split('\n')
    assert len(lines) >= 5 * len(cases)
    out = []
    for k in range(len(cases)):
        ln = lines[5 * k:5 * k + 5]
        ins = [int(x) for x in ln[1].split()]
        out.append(dict(frame=int(ln[0]), cap=ins[0], inserted=ins[1:],
                        listed=[int(x) for x in ln[2].split()],
                        found=[int(x) for x in ln[3].split()],
                        mask=int(ln[4], 16)))
    return out


# ---- the Python mirror ------------------------------------------------------

def home(i, cap):
    x = i & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x & (cap - 1)


def set_cap(K):
    c = 2
    while c < 2 * K:
        c <<= 1
    return c


class Mirror(object):
    """Open addressing, linear probing, at most cap probes."""

    def __init__(self, cap):
        self.cap = cap
        self.key = [0] * cap
        self.rank = [None] * cap

    def insert(self, i, pos):
        if i == 0:
            return 0
        s = home(i, self.cap)
        for _ in range(self.cap):
            if self.key[s] in (0, i):
                self.key[s] = i
                if self.rank[s] is None or pos < self.rank[s]:
                    self.rank[s] = pos
                return 1
            s = (s + 1) & (self.cap - 1)
        return 0

    def find(self, i):
        if i == 0:
            return -1
        s = home(i, self.cap)
        for _ in range(self.cap):
            if self.key[s] == 0:
                return -1
            if self.key[s] == i:
                return self.rank[s]
            s = (s + 1) & (self.cap - 1)
        return -1


def want_frame(c):
    b = c['frame']
    if c['bad'] != 0 or not 0 <= c['seg'] < c['S']:
        return 0
    if c['seg_state'][c['seg']] == 1:
        return 0
    if len(b) < 8:
        return 0
    return int(struct.unpack_from('>i', b, 4)[0] == CLOSE_SESSION)


def _check(prog, cases, tmp_path):
    got = _run(prog, cases, tmp_path)
    for k, (c, g) in enumerate(zip(cases, got)):
        assert g['frame'] == want_frame(c), (k, g['frame'])
        cap = c['cap'] or set_cap(len(c['ids']))
        assert g['cap'] == cap, k
        m = Mirror(cap)
        assert g['inserted'] == [m.insert(i, p)
                                 for p, i in enumerate(c['ids'])], k
        assert g['listed'] == [m.find(i) for i in c['ids']], k
        assert g['found'] == [m.find(i) for i in c['query']], k
        mask = 0
        for w in c['wslots']:
            if 0 <= w < 64:
                mask |= 1 << w
        assert g['mask'] == mask, (k, hex(g['mask']))
    return got


def same_home(cap, n, start=1):
    """n ids with one home slot in a table of cap entries: one probe run."""
    out, want, i = [], None, start
    while len(out) < n:
        h = home(i, cap)
        if want is None:
            want = h
        if h == want:
            out.append(i)
        i += 1
    return out


# ---- the cases --------------------------------------------------------------

def test_close_frame(prog, tmp_path):
    S = 3
    live = (0, 0, 0)
    cases = []
    for bad in (0, 1, -1):
        for seg in (-1, 0, S - 1, S, INT32_MAX):
            cases.append(_case(S=S, seg=seg, bad=bad, seg_state=live))
    # dead segments (state 1), and states that are not "dead"
    cases += [_case(S=S, seg=1, seg_state=(0, 1, 0)),
              _case(S=S, seg=0, seg_state=(0, 1, 0)),
              _case(S=S, seg=2, seg_state=(1, 1, 0)),
              _case(S=S, seg=2, seg_state=(0, 0, 2)),
              _case(S=1, seg=0, seg_state=(1,)),
              _case(S=1, seg=0, seg_state=(0,))]
    # bodies of 0, 7 and 8 bytes, and longer
    full = body()
    cases += [_case(frame=b''), _case(frame=full[:7]), _case(frame=full),
              _case(frame=body(tail=b'\x00' * 9))]
    # other opcodes
    for op in (11, 1, 2, 4, 101, -10, -1, 0, INT32_MIN, INT32_MAX, 0xF5):
        cases.append(_case(frame=body(op=op)))
    got = _check(prog, cases, tmp_path)
    # sound table, seg 0 and S - 1 close; nothing else of the first block
    assert [g['frame'] for g in got[:5]] == [0, 1, 1, 0, 0]
    assert all(g['frame'] == 0 for g in got[5:15])
    assert [g['frame'] for g in got[15:21]] == [0, 1, 1, 1, 0, 1]
    assert [g['frame'] for g in got[21:25]] == [0, 0, 1, 1]
    assert all(g['frame'] == 0 for g in got[25:])


def test_set(prog, tmp_path):
    sid = lambda srv, k: (srv << 56) | (k + 1)
    cases = []
    for K in (0, 1, 2, 63, 64, 65):
        ids = [sid(1, 7 * k) for k in range(K)]
        cases.append(_case(ids=ids, query=[0, sid(1, 1), sid(2, 0), -1]))
    # duplicates: the smallest position wins, wherever the copies are
    a, b, c = sid(1, 0), sid(1, 1), sid(3, 9)
    cases.append(_case(ids=[a, b, a, c, b, b, a], query=[a, b, c]))
    cases.append(_case(ids=[c, c], query=[c, a]))
    # id 0: never inserted, never found; a list of zeros
    cases.append(_case(ids=[0, a, 0, b], query=[0]))
    cases.append(_case(ids=[0, 0, 0], query=[0, a]))
    # ids equal in their low bits (one index, many servers), negative ids
    low = [sid(s, 41) for s in range(1, 40)]
    cases.append(_case(ids=low, query=[sid(40, 41), 42]))
    cases.append(_case(ids=[-1, -2, INT32_MIN, -(1 << 63)],
                       query=[-3, (1 << 63) - 1]))
    # one probe run: ids of one home slot, with a duplicate inside the run
    run = same_home(64, 9)
    cases.append(_case(ids=run + [run[3]], cap=64,
                       query=same_home(64, 12)[9:] + [run[0]]))
    # a run that wraps the table's end
    wrap = [i for i in range(1, 4000) if home(i, 8) == 7][:4]
    cases.append(_case(ids=wrap, cap=8, query=wrap + [5]))
    # a full-minus-one table and a full one: lookups of absent ids end, an
    # insert without room is refused
    seven = list(range(101, 108))
    cases.append(_case(ids=seven, cap=8, query=list(range(90, 120))))
    nine = list(range(101, 110))
    cases.append(_case(ids=nine, cap=8, query=list(range(90, 120))))
    cases.append(_case(ids=[5, 6, 5], cap=1, query=[5, 6, 7]))
    got = _check(prog, cases, tmp_path)
    assert [g['cap'] for g in got[:6]] == [2, 2, 4, 128, 128, 256]
    assert got[5]['listed'] == list(range(65))
    assert got[6]['listed'] == [0, 1, 0, 3, 1, 1, 0]
    assert got[6]['found'] == [0, 1, 3]
    assert got[8]['inserted'] == [0, 1, 0, 1] and got[8]['found'] == [-1]
    assert got[9]['inserted'] == [0, 0, 0] and got[9]['found'] == [-1, -1]
    assert got[12]['listed'] == list(range(9)) + [3]
    assert got[14]['inserted'] == [1] * 7
    assert got[15]['inserted'] == [1] * 8 + [0]
    assert got[15]['listed'][-1] == -1
    assert got[16]['inserted'] == [1, 0, 1] and got[16]['found'] == [0, -1,
                                                                    -1]


def test_random_sets(prog, tmp_path):
    rng = np.random.RandomState(7)
    cases = []
    for k in range(200):
        K = int(rng.choice([0, 1, 2, 3, 9, 33, 64, 100]))
        pool = [int(x) for x in rng.randint(0, max(2, K), size=K)]
        ids = [((1 + (p & 3)) << 56) | p if p else 0 for p in pool]
        cap = 0 if k % 2 else int(rng.choice([1, 2, 8, 64, 256]))
        q = [int(x) for x in rng.randint(0, 2 * max(2, K), size=16)]
        cases.append(_case(ids=ids, cap=cap, query=q + ids[:4]))
    _check(prog, cases, tmp_path)


def test_drop_mask(prog, tmp_path):
    cases = [_case(wslots=[w]) for w in (-1, 0, 63, 64, INT32_MIN, INT32_MAX)]
    cases.append(_case(wslots=[-1, 0, 63, 64, INT32_MIN]))
    cases.append(_case(wslots=[5, 5, 9]))
    cases.append(_case(wslots=[]))
    got = _check(prog, cases, tmp_path)
    assert [g['mask'] for g in got] == [0, 1, 1 << 63, 0, 0, 0,
                                        1 | (1 << 63), (1 << 5) | (1 << 9), 0]
