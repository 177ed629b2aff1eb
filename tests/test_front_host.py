"""The rules of the front end's I/O staging on the host:
csrc/kernels/zk_front.h (front_walk, front_is_write, the table fault,
front_piece_at, the owner table and front_piece — the text front.hip runs)
compiled by g++ into tools/front_host.cpp with ASan + UBSan, a stand-alone
program run as a child process with nothing preloaded.  Every segment and
every table sits in a heap block of exactly its length, so a read past one is
a sanitizer report; the output is compared with a Python mirror
(tests/frontmodel.py), on a machine without a GPU."""

import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import frontmodel as M

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
    exe = str(tmp_path_factory.mktemp('front') / 'front_host')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'front_host.cpp'), '-o', exe],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _i64(v):
    return np.asarray(v, np.int64).tobytes()


def walk_case(seg, quota, max_packet=M.MAX_PACKET):
    return struct.pack('<8q', 0, len(seg), quota, max_packet, 0, 0, 0,
                       0) + seg


def cut_case(raw, starts, quota, max_packet=M.MAX_PACKET):
    return struct.pack('<8q', 1, len(starts) - 1, len(raw), quota,
                       max_packet, 0, 0, 0) + _i64(starts) + raw


def piece_case(wslots, rep_off=None, slot_offs=(None, None, None), err=None,
               caps=(0, 0, 0, 0)):
    have = (rep_off is not None) | (16 if err is not None else 0)
    for k, so in enumerate(slot_offs):
        if so is not None:
            have |= 2 << k
    b = struct.pack('<8q', 2, len(wslots), have, err or 0, *caps)
    if rep_off is not None:
        b += _i64(rep_off)
    b += np.asarray(wslots, np.int32).tobytes()
    for so in slot_offs:
        if so is not None:
            b += _i64(so)
    return b


def at_case(off, queries):
    return struct.pack('<8q', 3, len(off), len(queries), 0, 0, 0, 0,
                       0) + _i64(off) + _i64(queries)


def _run(prog, blobs, tmp_path):
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as f:
        for b in blobs:
            f.write(b)
    env = {k: v for k, v in os.environ.items() if k != 'LD_PRELOAD'}
    r = subprocess.run([prog, path], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.split('\n')
    assert len(lines) >= len(blobs)
    return [[int(x) for x in ln.split()] for ln in lines[:len(blobs)]]


def _flat(rows):
    return [x for r in rows for x in r]


# ---- the walk ----------------------------------------------------------------

def test_walk_cases(prog, tmp_path):
    cases = M.walk_cases()
    got = _run(prog, [walk_case(seg, q) for _, seg, q, _ in cases], tmp_path)
    for (name, seg, q, want), g in zip(cases, got):
        assert tuple(g) == M.walk(seg, q), name
        if want is not None:
            assert tuple(g) == want, name


def test_is_write_by_opcode(prog, tmp_path):
    ops = list(range(-12, 16)) + [100, 101, 102, M.INT32_MIN, 2 ** 31 - 1]
    g = M.frame(M.OPS['GET_DATA'], b'\x00' * 9)
    blobs = [walk_case(g + M.frame(op, b'\x00' * 4) + g, 8) for op in ops]
    got = _run(prog, blobs, tmp_path)
    for op, r in zip(ops, got):
        f = M.frame(op, b'\x00' * 4)
        want = (len(g), 1, 0) if M.is_write(op) else \
            (2 * len(g) + len(f), 3, 0)
        assert tuple(r) == want, op
    assert sorted(op for op in ops if M.is_write(op)) == [-11, 1, 2, 5]


def test_max_packet_is_the_launch_scalar(prog, tmp_path):
    body = b'\x00' * 40
    seg = M.raw_frame(40, body) + M.raw_frame(41, body + b'\x00')
    got = _run(prog, [walk_case(seg, 8, 40), walk_case(seg, 8, 41),
                      walk_case(seg, 8, 39), walk_case(seg, 8, 0)], tmp_path)
    assert [tuple(g) for g in got] == [(44, 1, 1), (89, 2, 0), (0, 0, 1),
                                       (0, 0, 1)]


# ---- the table ---------------------------------------------------------------

def test_table_faults(prog, tmp_path):
    g = M.frame(M.OPS['GET_DATA'], b'\x00' * 9)
    raw = g * 4
    n = len(raw)
    L = len(g)
    tables = [
        [0, L, 2 * L, n],              # sound
        [0, 0, n, n],                  # sound, empty segments
        [1, L, 2 * L, n],              # does not start at 0
        [0, 2 * L, L, n],              # descends
        [0, L, 2 * L, n + 1],          # passes n
        [0, n + 5, n + 5, n + 5],      # passes n, all of it
        [-1, L, 2 * L, n],             # negative
        [0, L, n, 2 * L],              # the last boundary descends
    ]
    got = _run(prog, [cut_case(raw, t, 8) for t in tables], tmp_path)
    for t, r in zip(tables, got):
        fault, segs = M.cut(raw, t, 8)
        assert r == [fault] + _flat(segs), t
    assert [r[0] for r in got] == [0, 0, 1, 1, 1, 1, 1, 1]
    assert got[0][1:] == [L, 1, 0, L, 1, 0, 2 * L, 2, 0]
    assert all(x == 0 for r in got[2:] for x in r[1:])


def test_random_tables(prog, tmp_path):
    rng = np.random.RandomState(11)
    ops = list(M.OPS.values()) + [7, 13, 14, 0, -1]
    blobs, want = [], []
    for k in range(200):
        S = int(rng.choice([1, 2, 3, 7, 16]))
        segs = []
        for s in range(S):
            b = b''
            for _ in range(int(rng.randint(0, 6))):
                op = int(rng.choice(ops))
                body = bytes(rng.randint(0, 256, size=int(rng.randint(0, 30)),
                                         dtype=np.uint8))
                b += M.frame(op, body)
            r = rng.randint(0, 10)
            if r == 0:
                b += M.raw_frame(int(rng.choice([-1, M.INT32_MIN,
                                                 M.MAX_PACKET + 1])))
            elif r == 1:
                b += M.raw_frame(3)[:int(rng.randint(1, 4))]
            elif r == 2 and b:
                b = b[:len(b) - int(rng.randint(1, min(len(b), 9) + 1))]
            elif r == 3:
                b = b''
            segs.append(b)
        raw = b''.join(segs)
        starts = [0]
        for b in segs:
            starts.append(starts[-1] + len(b))
        if k % 10 == 9 and len(raw) > 0:        # a faulted table
            j = int(rng.randint(0, S + 1))
            starts[j] = int(rng.choice([-1, len(raw) + 1, starts[j] + 1
                                        if j == 0 else starts[j - 1] - 1]))
        quota = int(rng.choice([0, 1, 2, 3, 64]))
        blobs.append(cut_case(raw, starts, quota))
        fault, cuts = M.cut(raw, starts, quota)
        want.append([fault] + _flat(cuts))
    got = _run(prog, blobs, tmp_path)
    assert got == want
    assert sum(w[0] for w in want) >= 10
    assert sum(1 for w in want if w[0] == 0 and 1 in w[3::3]) >= 10


# ---- the gather's search -----------------------------------------------------

def test_piece_at(prog, tmp_path):
    tables = [[0], [0, 0, 0, 5], [0, 3, 3, 3, 9, 20], [0, 16, 32, 48],
              list(range(0, 1025 * 7, 7))]
    blobs, want = [], []
    for off in tables:
        q = sorted(set([0, 1, 2, 3, 4, 8, 15, 16, 17, 19, 47, 48, 100,
                        off[-1], off[-1] + 1, off[-1] + 1000]))
        blobs.append(at_case(off, q))
        want.append([M.piece_at(off, d) for d in q])
    assert _run(prog, blobs, tmp_path) == want
    assert want[1][:5] == [2, 2, 2, 2, 2] and want[1][5] == 3
    assert want[2][3] == 3 and want[2][2] == 0


# ---- the pieces --------------------------------------------------------------

def _offs(rng, total):
    cuts = sorted(int(x) for x in rng.randint(0, total + 1, size=63))
    return [0] + cuts + [total]


def test_pieces(prog, tmp_path):
    rng = np.random.RandomState(3)
    caps = (1000, 700, 800, 900)
    so = [_offs(rng, caps[k + 1]) for k in range(3)]
    rep5 = [0, 100, 100, 400, 990, 1000]
    cases = [
        dict(wslots=[-1, 0, 63, 64, 5], rep_off=rep5, slot_offs=so),
        dict(wslots=[M.INT32_MIN, 2 ** 31 - 1, 1, 1, 1], rep_off=rep5,
             slot_offs=so),
        # two segments on one slot, the owner second in the table's order
        dict(wslots=[7, 3, 7, 3, -1], rep_off=rep5, slot_offs=so),
        # each stream absent in turn, and all of them
        dict(wslots=[0, 1, 2, 3, 4], rep_off=None, slot_offs=so),
        dict(wslots=[0, 1, 2, 3, 4], rep_off=rep5,
             slot_offs=[None, so[1], so[2]]),
        dict(wslots=[0, 1, 2, 3, 4], rep_off=rep5,
             slot_offs=[so[0], None, so[2]]),
        dict(wslots=[0, 1, 2, 3, 4], rep_off=rep5,
             slot_offs=[so[0], so[1], None]),
        dict(wslots=[0, 1, 2, 3, 4], rep_off=None,
             slot_offs=[None, None, None]),
        # the batch's err
        dict(wslots=[0, 1, 2, 3, 4], rep_off=rep5, slot_offs=so, err=2),
        dict(wslots=[0, 1, 2, 3, 4], rep_off=rep5, slot_offs=so, err=-1),
        dict(wslots=[0, 1, 2, 3, 4], rep_off=rep5, slot_offs=so, err=0),
        # slices the streams do not hold
        dict(wslots=[0, 63], rep_off=[0, 1000, 1001],
             slot_offs=[[0] + [701] * 64, [5] + [4] * 64, [-1] + [9] * 64]),
        dict(wslots=[0], rep_off=[0, 1000], slot_offs=so),
    ]
    for c in cases:
        c.setdefault('caps', caps)
    got = _run(prog, [piece_case(**c) for c in cases], tmp_path)
    for k, (c, g) in enumerate(zip(cases, got)):
        dup, ps = M.pieces(**c)
        assert g == [dup] + _flat(ps), k
    P = lambda g, s, k: tuple(g[1 + 3 * (4 * s + k):4 + 3 * (4 * s + k)])
    g = got[0]
    assert g[0] == 0
    assert P(g, 0, 0) == (0, 0, 100) and P(g, 0, 1) == (1, 0, 0)
    assert P(g, 1, 1) == (1, so[0][0], so[0][1] - so[0][0])
    assert P(g, 2, 3) == (3, so[2][63], so[2][64] - so[2][63])
    assert P(g, 3, 0) == (0, 400, 590) and P(g, 3, 2) == (2, 0, 0)
    assert got[1][0] == 2
    g = got[2]
    assert g[0] == 2
    assert P(g, 0, 2)[2] == so[1][8] - so[1][7] and P(g, 2, 2)[2] == 0
    assert P(g, 1, 2)[2] == so[1][4] - so[1][3] and P(g, 3, 2)[2] == 0
    assert all(P(got[3], s, 0) == (0, 0, 0) for s in range(5))
    assert all(P(got[4 + j], s, 1 + j)[2] == 0
               for j in range(3) for s in range(5))
    assert all(x == 0 for x in got[8][1:][2::3])
    assert all(x == 0 for x in got[9][1:][2::3])
    assert got[10] == [0] + _flat(M.pieces(**dict(cases[10], err=None))[1])
    assert [P(got[11], s, k)[2] for s in range(2) for k in range(4)] == \
        [1000, 0, 0, 0, 0, 0, 0, 0]


def test_random_pieces(prog, tmp_path):
    rng = np.random.RandomState(5)
    blobs, want = [], []
    for k in range(100):
        S = int(rng.choice([1, 2, 5, 64, 65, 130]))
        wslots = [int(x) for x in rng.randint(-2, 66, size=S)]
        caps = tuple(int(x) for x in rng.randint(0, 5000, size=4))
        rep = sorted(int(x) for x in rng.randint(0, caps[0] + 1, size=S + 1))
        so = [_offs(rng, caps[j + 1]) if rng.randint(0, 4) else None
              for j in range(3)]
        c = dict(wslots=wslots, rep_off=rep if rng.randint(0, 4) else None,
                 slot_offs=so, caps=caps,
                 err=None if rng.randint(0, 3) else int(rng.randint(0, 2)))
        blobs.append(piece_case(**c))
        dup, ps = M.pieces(**c)
        want.append([dup] + _flat(ps))
    assert _run(prog, blobs, tmp_path) == want
