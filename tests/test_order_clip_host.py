"""The rules of the ordered front end on the host: csrc/kernels/zk_front.h
front_walk_ordered and csrc/kernels/zk_order_clip.h (clip_overflow,
clip_deferred, clip_range — the text front.hip and tree_order.hip run)
compiled by g++ into tools/order_clip_host.cpp with ASan + UBSan, a
stand-alone program run as a child process with nothing preloaded.  Every
segment and every table sits in a heap block of exactly its length, so a read
past one is a sanitizer report; the output is compared with a Python mirror
(tests/ordermodel.py), on a machine without a GPU."""

import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import frontmodel as F
import ordermodel as M

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
    exe = str(tmp_path_factory.mktemp('oclip') / 'order_clip_host')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'order_clip_host.cpp'), '-o', exe],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _i64(v):
    return np.asarray(v, np.int64).tobytes()


def _i32(v):
    return np.asarray(v, np.int32).tobytes()


def walk_case(seg, quota, has_acl=True, max_packet=M.MAX_PACKET):
    return struct.pack('<8q', 0, len(seg), quota, max_packet, int(has_acl),
                       0, 0, 0) + seg


def clip_case(rank, cls, sub, f_seg, S, passes, nfr=None):
    ncap = len(cls)
    return struct.pack('<8q', 1, ncap, S, passes,
                       ncap if nfr is None else nfr, 0, 0, 0) + \
        np.asarray(rank, np.uint8).tobytes() + _i32(cls) + _i32(sub) + \
        _i32(f_seg)


def range_case(clipf, rep_off, rec_off, off, starts, nfr):
    return struct.pack('<8q', 2, len(clipf), len(rec_off), nfr, 0, 0, 0,
                       0) + _i64(clipf) + _i64(rep_off) + _i64(rec_off) + \
        _i64(off) + _i64(starts)


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


# ---- the ordered walk ----------------------------------------------------------

def test_walk_cases(prog, tmp_path):
    cases = M.walk_cases()
    got = _run(prog, [walk_case(seg, q, acl) for _, seg, q, acl, _ in cases],
               tmp_path)
    for (name, seg, q, acl, want), g in zip(cases, got):
        assert tuple(g) == M.walk_ordered(seg, q, acl), name
        if want is not None:
            assert tuple(g) == want, name


def test_walk_by_opcode(prog, tmp_path):
    """One frame of every opcode in phase 0 and behind a list."""
    ops = list(range(-12, 16)) + [100, 101, 102, F.INT32_MIN, 2 ** 31 - 1]
    g = F.frame(F.OPS['GET_DATA'], b'\x00' * 9)
    ls = F.frame(F.OPS['GET_CHILDREN'], b'\x00' * 9)
    blobs, want = [], []
    for acl in (True, False):
        for op in ops:
            f = F.frame(op, b'\x00' * 4)
            for seg in (g + f + g, ls + f + g, f + F.frame(1, b'\x00' * 4)):
                blobs.append(walk_case(seg, 8, acl))
                want.append(list(M.walk_ordered(seg, 8, acl)))
    assert _run(prog, blobs, tmp_path) == want
    # the stops the rule names, outright
    f = lambda op: F.frame(op, b'\x00' * 4)
    L = len(f(1))
    for op in (1, 2, 5):
        assert M.walk_ordered(ls + f(op) + g, 8) == (len(ls), 1, 0, 0)
        assert M.walk_ordered(g + f(op) + g, 8) == (2 * len(g) + L, 3, 0, 1)
    assert M.walk_ordered(g + f(-11) + g, 8) == (len(g) + L, 2, 0, 1)
    for op in (8, 12, 101):
        assert M.walk_ordered(f(op) + f(1), 8, False) == (L, 1, 0, 0)
    assert M.walk_ordered(f(6) + f(1), 8, True) == (L, 1, 0, 0)
    assert M.walk_ordered(f(6) + f(1), 8, False) == (2 * L, 2, 0, 1)


def test_random_walks(prog, tmp_path):
    rng = np.random.RandomState(17)
    # (weighted towards the writes and the reads: runs of several writes)
    ops = list(F.OPS.values()) + [7, 13, 14, 0, -1] + [1, 2, 5, 4, 3] * 4
    blobs, want = [], []
    for k in range(400):
        b = b''
        for _ in range(int(rng.randint(0, 9))):
            op = int(rng.choice(ops))
            body = bytes(rng.randint(0, 256, size=int(rng.randint(0, 30)),
                                     dtype=np.uint8))
            b += F.frame(op, body)
        r = rng.randint(0, 8)
        if r in (0, 3, 4):
            b += F.raw_frame(int(rng.choice([-1, F.INT32_MIN,
                                             F.MAX_PACKET + 1])))
        elif r == 1:
            b += F.raw_frame(3)[:int(rng.randint(1, 4))]
        elif r == 2 and b:
            b = b[:len(b) - int(rng.randint(1, min(len(b), 9) + 1))]
        quota = int(rng.choice([0, 1, 2, 3, 64]))
        acl = bool(rng.randint(0, 2))
        blobs.append(walk_case(b, quota, acl))
        want.append(list(M.walk_ordered(b, quota, acl)))
    assert _run(prog, blobs, tmp_path) == want
    assert sum(1 for w in want if w[2] == 1) >= 10
    assert sum(1 for w in want if w[3] >= 2) >= 20


# ---- the clip ----------------------------------------------------------------

def _batch(segs_of, classes):
    """cls / sub of a batch whose frame i has class classes[i]."""
    n = [0, 0, 0]
    sub = []
    for c in classes:
        sub.append(n[c])
        n[c] += 1
    return list(classes), sub, list(segs_of)


def test_clip_cases(prog, tmp_path):
    P = 4
    cases = []
    # no clip: every rank below passes
    cls, sub, seg = _batch([0, 0, 1, 1, 2, 2], [0] * 6)
    cases.append((dict(rank=[0, 1, 2, 3, 3, 0], cls=cls, sub=sub, f_seg=seg,
                       S=3, passes=P), [6, 6, 6], [0] * 6))
    # clipf at a segment's first frame, and at another's last; an empty
    # segment (1) between them
    cls, sub, seg = _batch([0, 0, 0, 2, 2, 2], [0] * 6)
    cases.append((dict(rank=[4, 0, 0, 0, 1, 0x7f], cls=cls, sub=sub,
                       f_seg=seg, S=3, passes=P), [0, 6, 5],
                  [1, 1, 1, 0, 0, 1]))
    # the snapshot bit is no rank; a rank of exactly passes is an overflow
    cls, sub, seg = _batch([0, 0, 1, 1], [0] * 4)
    cases.append((dict(rank=[0x83, 0x80, 0x84, 0], cls=cls, sub=sub,
                       f_seg=seg, S=2, passes=P), [4, 2], [0, 0, 1, 1]))
    # an overflow in class 0 only: the other classes' frames have no rank
    # (their sub indexes another table) but are deferred behind one
    cls, sub, seg = _batch([0, 0, 0, 0, 1, 1, 1], [2, 0, 1, 2, 2, 0, 1])
    cases.append((dict(rank=[0, 9, 9, 9, 9, 9, 9], cls=cls, sub=sub,
                       f_seg=seg, S=2, passes=P), [7, 5], [0] * 5 + [1, 1]))
    # f_seg already -1 (a frame of no segment) and outside the table
    cls, sub, seg = _batch([0, -1, 0, 5, 0], [0] * 5)
    cases.append((dict(rank=[0, 9, 0, 9, 9], cls=cls, sub=sub, f_seg=seg,
                       S=1, passes=P), [4], [0, 0, 0, 0, 1]))
    # frames past the batch's count are not looked at
    cls, sub, seg = _batch([0, 0, 0, 0], [0] * 4)
    cases.append((dict(rank=[0, 0, 9, 9], cls=cls, sub=sub, f_seg=seg, S=1,
                       passes=P, nfr=2), [4], [0, 0]))
    # a sub outside the table is no overflow
    cases.append((dict(rank=[9, 9], cls=[0, 0], sub=[-1, 2], f_seg=[0, 0],
                       S=1, passes=P), [2], [0, 0]))
    got = _run(prog, [clip_case(**c) for c, _, _ in cases], tmp_path)
    for k, ((c, clipf, df), g) in enumerate(zip(cases, got)):
        mc, md = M.clip(**c)
        assert g == mc + md, k
        assert mc == clipf and md == df, k


def test_random_clips(prog, tmp_path):
    rng = np.random.RandomState(23)
    blobs, want = [], []
    for k in range(200):
        ncap = int(rng.choice([1, 5, 63, 64, 65, 130, 300]))
        S = int(rng.choice([1, 2, 7, 40]))
        nfr = int(rng.randint(0, ncap + 1))
        seg = np.sort(rng.randint(0, S, size=ncap)).tolist()
        for j in rng.randint(0, ncap, size=ncap // 8):
            seg[j] = int(rng.choice([-1, S, S + 3]))
        classes = rng.choice([0, 0, 0, 1, 2], size=ncap).tolist()
        cls, sub, seg = _batch(seg, classes)
        if k % 5 == 0:
            sub[int(rng.randint(0, ncap))] = int(rng.choice([-1, ncap]))
            cls[int(rng.randint(0, ncap))] = int(rng.choice([-1, 3]))
        rank = (rng.randint(0, 7, size=ncap) |
                (rng.randint(0, 2, size=ncap) << 7)).tolist()
        passes = int(rng.choice([1, 4, 6, 8]))
        c = dict(rank=rank, cls=cls, sub=sub, f_seg=seg, S=S, passes=passes,
                 nfr=nfr)
        blobs.append(clip_case(**c))
        mc, md = M.clip(**c)
        want.append(mc + md)
    assert _run(prog, blobs, tmp_path) == want


# ---- the ranges --------------------------------------------------------------

def test_range_cases(prog, tmp_path):
    # three segments of 2, 0 and 3 frames of 24 request bytes and 20 reply
    # bytes each
    off = [4, 28, 52, 76, 100, 0, 0, 0]
    rec = [0, 20, 40, 60, 80, 0, 0, 0]
    starts = [0, 48, 48, 120]
    rep = [0, 40, 40, 100]
    nfr = 5
    cases = [
        ([8, 8, 8], [(40, 48), (40, 0), (100, 72)]),       # no clip
        ([0, 8, 4], [(0, 0), (40, 0), (80, 48)]),          # first / last frame
        ([1, 8, 2], [(20, 24), (40, 0), (40, 0)]),
        ([8, 8, 3], [(40, 48), (40, 0), (60, 24)]),
        # a clipf the table cannot hold is no clip; one of another segment's
        # frames stays inside the segment's own slices
        ([-1, 5, 7], [(40, 48), (40, 0), (100, 72)]),
        ([4, 8, 0], [(40, 48), (40, 0), (40, 0)]),
    ]
    got = _run(prog, [range_case(c, rep, rec, off, starts, nfr)
                      for c, _ in cases], tmp_path)
    for (c, want), g in zip(cases, got):
        m = M.ranges(c, rep, rec, off, starts, nfr)
        assert g == [x for r in m for x in r], c
        assert m == want, c
    # an encode that overflowed: rep_off is all zero, every end is 0
    z = _run(prog, [range_case([1, 8, 3], [0, 0, 0, 0], rec, off, starts,
                               nfr)], tmp_path)[0]
    assert z[0::2] == [0, 0, 0] and z[1::2] == [24, 0, 24]


def test_random_ranges(prog, tmp_path):
    rng = np.random.RandomState(29)
    blobs, want = [], []
    for k in range(200):
        S = int(rng.choice([1, 3, 65]))
        ncap = int(rng.choice([1, 7, 64, 200]))
        nfr = int(rng.randint(0, ncap + 1))
        starts = np.sort(rng.randint(0, 5000, size=S + 1)).tolist()
        rep = np.sort(rng.randint(0, 5000, size=S + 1)).tolist()
        rec = rng.randint(-10, 5100, size=ncap).tolist()
        off = rng.randint(-10, 5100, size=ncap).tolist()
        clipf = rng.randint(-2, ncap + 2, size=S).tolist()
        blobs.append(range_case(clipf, rep, rec, off, starts, nfr))
        want.append([x for r in M.ranges(clipf, rep, rec, off, starts, nfr)
                     for x in r])
    assert _run(prog, blobs, tmp_path) == want
