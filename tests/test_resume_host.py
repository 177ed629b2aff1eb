"""The rules of a session batch's SET_WATCHES catch-up on the host:
csrc/kernels/zk_resume.h (resume_frame, resume_walk, resume_decide,
resume_entry_frame — the text tree_resume.hip runs) compiled by g++ into
tools/resume_host.cpp with ASan + UBSan, a stand-alone program run as a child
process with nothing preloaded.  Every frame and every table sits in a heap
block of exactly its length, so a read past one is a sanitizer report; the
output is compared with a Python mirror written from wt_resume_k's walk
(csrc/kernels/tree_watch.hip) and the session rule's table — on a machine
without a GPU."""

import bisect
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET_WATCHES = 101
NONE, NO_SLOT = -1, -2
CREATED, DELETED, DATA_CHANGED, CHILDREN_CHANGED = 1, 2, 3, 4
ARM_DATA, ARM_CHILD = -1, -2
INT32_MAX = 2 ** 31 - 1
INT32_MIN = -2 ** 31
PIECES = (1, 2, 3, 4, 5, 7, 16, 61, 64, 1024)


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
    exe = str(tmp_path_factory.mktemp('resume') / 'resume_host')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'resume_host.cpp'), '-o', exe],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


# ---- frames -----------------------------------------------------------------

def lists(data=(), exist=(), child=()):
    out = b''
    for paths in (data, exist, child):
        out += struct.pack('>i', len(paths))
        for p in paths:
            out += struct.pack('>i', len(p)) + p
    return out


def body(tail, rel=7, op=SET_WATCHES, xid=-8):
    return struct.pack('>iiq', xid, op, rel) + tail


def _case(frame, piece=64, S=2, seg=0, bad=0, seg_state=(0, 0),
          wslots=(5, 63), decide=(), base=(), query=()):
    assert len(seg_state) == S and len(wslots) == S
    return dict(frame=frame, piece=piece, S=S, seg=seg, bad=bad,
                seg_state=list(seg_state), wslots=list(wslots),
                decide=list(decide), base=list(base), query=list(query))


def _run(prog, cases, tmp_path):
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as f:
        for c in cases:
            f.write(struct.pack('<8q', c['S'], c['seg'], c['bad'],
                                len(c['frame']), c['piece'], len(c['decide']),
                                len(c['base']), len(c['query'])))
            f.write(np.asarray(c['seg_state'], np.int32).tobytes())
            f.write(np.asarray(c['wslots'], np.int32).tobytes())
            f.write(c['frame'])
            for d in c['decide']:
                f.write(struct.pack('<5q', *d))
            f.write(np.asarray(c['base'], np.int64).tobytes())
            f.write(np.asarray(c['query'], np.int64).tobytes())
    env = {k: v for k, v in os.environ.items() if k != 'LD_PRELOAD'}
    r = subprocess.run([prog, path], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.split('\n')
    assert len(lines) >= 6 * len(cases)
    out = []
    for k in range(len(cases)):
        ln = lines[6 * k:6 * k + 6]
        walks = []
        for w in ln[1:3]:
            t = w.split()
            walks.append((int(t[0]), int(t[1]),
                          [tuple(int(x) for x in e.split(':'))
                           for e in t[2:]]))
        out.append(dict(frame=int(ln[0]), whole=walks[0], pieces=walks[1],
                        parse=tuple(int(x) for x in ln[3].split()),
                        decide=[int(x) for x in ln[4].split()],
                        entry=[int(x) for x in ln[5].split()]))
    return out


# ---- the Python mirror ------------------------------------------------------

def be32(b, k):
    return struct.unpack_from('>i', b, k)[0]


def want_walk(b):
    """wt_resume_k's listing of a frame body, and whether the three lists
    were whole (parse_request's verdict on a SET_WATCHES)."""
    end, k, out = len(b), 16, []
    for g in range(3):
        if k + 4 > end:
            return False, out
        c = max(be32(b, k), 0)
        k += 4
        for _ in range(c):
            if k + 4 > end:
                return False, out
            ln = max(be32(b, k), 0)
            if k + 4 + ln > end:
                return False, out
            out.append((g, k + 4, ln))
            k += 4 + ln
    return True, out


def want_frame(c):
    b = c['frame']
    if c['bad'] != 0 or not 0 <= c['seg'] < c['S']:
        return NONE
    if c['seg_state'][c['seg']] == 1:
        return NONE
    if len(b) < 20 or be32(b, 4) != SET_WATCHES:
        return NONE
    w = c['wslots'][c['seg']]
    return w if 0 <= w < 64 else NO_SLOT


def want_decide(kind, there, mzxid, pzxid, rel):
    if kind == 0:
        if not there:
            return DELETED
        return DATA_CHANGED if mzxid > rel else ARM_DATA
    if kind == 1:
        return CREATED if there else ARM_DATA
    if not there:
        return DELETED
    return CHILDREN_CHANGED if pzxid > rel else ARM_CHILD


def _check(prog, cases, tmp_path):
    got = _run(prog, cases, tmp_path)
    for k, (c, g) in enumerate(zip(cases, got)):
        ok, want = want_walk(c['frame'])
        assert g['frame'] == want_frame(c), (k, g['frame'])
        assert g['whole'] == (int(ok), len(want), want), (k, g['whole'][:2])
        assert g['pieces'] == g['whole'], (k, c['piece'])
        st, op, vc = g['parse']
        if op == SET_WATCHES and len(c['frame']) >= 8:
            # the walk's verdict is parse_request's
            assert (st == 0) == ok, (k, st, ok)
            if ok:
                assert vc == len(want)
        assert g['decide'] == [want_decide(*d) for d in c['decide']], k
        assert g['entry'] == [bisect.bisect_right(c['base'], e) - 1
                              for e in c['query']], k
    return got


# ---- the cases --------------------------------------------------------------

def malformed():
    """The malformed corpus of the GPU tests, as frame bodies."""
    a, b, c = b'/a/bb', b'/ccc', b'/d'
    good = lists([a, b], [c], [a])
    return {
        'count past the frame': body(
            struct.pack('>i', 5) + struct.pack('>i', len(a)) + a),
        'negative count': body(
            struct.pack('>i', -3) + lists([a], [b])[:-4]),
        'negative length': body(
            struct.pack('>i', 2) + struct.pack('>i', -9) +
            struct.pack('>i', len(b)) + b + lists()[4:]),
        'length past the frame': body(
            struct.pack('>i', 2) + struct.pack('>i', len(a)) + a +
            struct.pack('>i', 400) + b),
        'cut inside a length word': body(good[:4 + 4 + len(a) + 2]),
        'cut inside a path': body(good[:4 + 4 + len(a) + 4 + 2]),
        'two lists': body(lists([a, b], [c])[:-4]),
        'trailing bytes': body(good + b'\x00\x00\x00\x01junk'),
        'huge count': body(struct.pack('>i', INT32_MAX) +
                           struct.pack('>i', len(a)) + a),
        'huge length': body(struct.pack('>i', 1) +
                            struct.pack('>i', INT32_MAX)),
        'minimum length': body(struct.pack('>i', 1) +
                               struct.pack('>i', INT32_MIN) + lists()[4:]),
        'no list': body(b''),
        'half a count': body(b'\x00\x00'),
        'short body': body(b'')[:11],
        'empty body': b'',
    }


def test_named_cases(prog, tmp_path):
    a, b = b'/a/bb', b'/ccc'
    good = body(lists([a, b], [b], [a, a, b]))
    cases = [_case(good)]
    names = sorted(malformed())
    cases += [_case(malformed()[n], piece=p) for n in names
              for p in (3, 64)]
    # the frame rule: refusals, segments, slots, opcodes
    cases += [
        _case(good, bad=1), _case(good, bad=-1),
        _case(good, seg=1, seg_state=(0, 1)),
        _case(good, seg=1, seg_state=(1, 2)),
        _case(good, seg=-1), _case(good, seg=2), _case(good, seg=INT32_MAX),
        _case(good, wslots=(-1, 0)), _case(good, wslots=(64, 0)),
        _case(good, wslots=(INT32_MIN, 0)), _case(good, wslots=(0, 0)),
        _case(good, seg=1), _case(body(lists(), op=4)),
        _case(body(lists())[:19]), _case(body(lists())[:20]),
    ]
    # the session rule: every branch on both sides of relZxid
    dec = [(k, t, mz, pz, 10) for k in (0, 1, 2) for t in (0, 1)
           for mz in (9, 10, 11) for pz in (9, 10, 11)]
    cases.append(_case(good, decide=dec))
    # entries -> frames: frames that list nothing own nothing
    base = [0, 0, 3, 3, 3, 7, 7]
    cases.append(_case(good, base=base, query=list(range(-2, 12))))
    cases.append(_case(good, base=[], query=[0, 5]))
    got = _check(prog, cases, tmp_path)
    assert got[0]['frame'] == 5 and got[0]['whole'][:2] == (1, 6)
    by = {n: got[1 + 2 * i] for i, n in enumerate(names)}
    # what the listing keeps of a frame that is cut: the paths before the cut
    assert by['count past the frame']['whole'][:2] == (0, 1)
    assert by['negative count']['whole'][:2] == (1, 2)
    assert by['negative length']['whole'][:2] == (1, 2)
    assert by['negative length']['whole'][2][0][2] == 0
    assert by['length past the frame']['whole'][:2] == (0, 1)
    assert by['cut inside a length word']['whole'][:2] == (0, 1)
    assert by['cut inside a path']['whole'][:2] == (0, 1)
    assert by['two lists']['whole'][:2] == (0, 3)
    assert by['trailing bytes']['whole'][:2] == (1, 4)
    assert by['empty body']['whole'][:2] == (0, 0)
    assert by['empty body']['frame'] == NONE
    n = 1 + 2 * len(names)
    assert [g['frame'] for g in got[n:n + 15]] == [
        NONE, NONE, NONE, 63, NONE, NONE, NONE, NO_SLOT, NO_SLOT, NO_SLOT, 0,
        63, NONE, NONE, 5]


def test_random_frames(prog, tmp_path):
    """Well-formed lists of random sizes and path lengths, fed whole and in
    pieces of every size of PIECES, and the same frames damaged: cut at a
    random byte, or with one word overwritten by a hostile value."""
    rng = np.random.RandomState(41)
    edge = [-1, 0, 1, INT32_MAX, INT32_MIN, 1 << 20]
    cases = []
    for k in range(400):
        ls = []
        for _ in range(3):
            n = int(rng.choice([0, 0, 1, 2, 5, 40]))
            ls.append([bytes(rng.randint(47, 123, int(rng.choice(
                [0, 1, 2, 3, 4, 5, 9, 30, 59, 60, 61, 200])),
                dtype=np.uint8)) for _ in range(n)])
        frame = bytearray(body(lists(*ls), rel=int(rng.randint(0, 99))))
        if k % 3 == 1:
            frame = frame[:int(rng.randint(0, len(frame) + 1))]
        elif k % 3 == 2:
            at = 16 + 4 * int(rng.randint(0, (len(frame) - 16) // 4))
            v = int(edge[int(rng.randint(len(edge)))])
            frame[at:at + 4] = struct.pack('>i', v)
        cases.append(_case(bytes(frame),
                           piece=int(PIECES[k % len(PIECES)])))
    got = _check(prog, cases, tmp_path)
    assert all(g['whole'][0] == 1 for g in got[0::3])
    assert any(g['whole'][0] == 0 and g['whole'][1] > 0 for g in got)
