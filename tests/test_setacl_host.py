"""The rule of SET_ACL on the host: csrc/kernels/zk_setacl.h (setacl_frame,
setacl_admin, setacl_verdict) compiled by g++ into tools/setacl_host.cpp with
ASan + UBSan, a stand-alone program run as a child process with nothing
preloaded.  Every frame, vector and record block sits in a heap block of
exactly its length, so a read past one is a sanitizer report; the output is
compared with the Python mirror (tests/setacl_model.py) over generated frames
and every truncation of them, on a machine without a GPU."""

import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import aclperm_model as A
import auth_model as M
import setacl_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    exe = str(tmp_path_factory.mktemp('setacl') / 'setacl_host')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror',
         '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'setacl_host.cpp'), '-o', exe],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(prog, cases, tmp_path):
    """cases: (kind, a, b, bytes) -> the program's line per case."""
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as f:
        for kind, a, b, raw in cases:
            f.write(struct.pack('<4q', kind, a, b, len(raw)))
            f.write(raw)
    env = {k: v for k, v in os.environ.items() if k != 'LD_PRELOAD'}
    r = subprocess.run([prog, path], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.split('\n')
    assert len(lines) >= len(cases)
    return lines[:len(cases)]


def _frame_case(b, base=0):
    return (0, base, 0, b'\xaa' * base + b)


def _want_frame(b):
    return '%d %d %d %d %d %d %d' % S.parse(b)


OPEN = A.vector([(A.ALL, 'world', 'anyone')])
U = M.identity(b'u:pw')
SUPER = M.identity(b'super:test')
PEER = A.addr_of('10.1.2.9')
THREE = A.vector([(A.READ, 'world', 'anyone'), (A.ALL, 'digest', U),
                  (A.ADMIN, 'ip', '10.1.2.0/24')])
BIG = A.vector([(A.ALL, 'digest', b'x' * 278)])


def test_setacl_frame(prog, tmp_path):
    good = S.body(5, '/a', OPEN, -1)
    assert len(good) == 8 + 4 + 2 + len(OPEN) + 4
    assert len(BIG) == 300
    bodies = [good, S.body(-7, '/a/b', THREE, 3), S.body(1, '/n', BIG, 0),
              S.body(1, '/n', THREE, INT32_MIN), S.body(1, 'x' * 300, OPEN, 2),
              # an empty vector, a negative count: whole frames, INVALID_ACL
              S.body(9, '/a', struct.pack('>i', 0), 4),
              S.body(9, '/a', struct.pack('>i', -1), 4),
              S.body(9, '/a', struct.pack('>i', INT32_MIN), -1),
              # ... but entries behind a count of 0 are trailing bytes
              S.body(9, '/a', struct.pack('>i', 0) + OPEN[4:], 4),
              # empty and null strings inside an entry are well formed
              S.body(2, '/a', A.vector([(0, b'', b'')]), 0),
              S.body(2, '/a', struct.pack('>iiii', 1, 31, -1, -5), 0),
              # bytes behind the version, no version, half a version
              good + b'\x00', good + good, good[:-4], good[:-2],
              # a bad path length
              struct.pack('>iii', 3, 7, 0) + OPEN + struct.pack('>i', 0),
              struct.pack('>iii', 3, 7, -1) + OPEN + struct.pack('>i', 0),
              struct.pack('>iii', 3, 7, INT32_MAX) + b'/a' + OPEN +
              struct.pack('>i', 0),
              struct.pack('>iii', 3, 7, INT32_MIN) + b'/a' + OPEN +
              struct.pack('>i', 0),
              # a count that leaves the frame
              S.body(4, '/a', struct.pack('>i', 2) + OPEN[4:], 0),
              S.body(4, '/a', struct.pack('>i', INT32_MAX) + OPEN[4:], 0),
              # lengths inside an entry that leave it
              S.body(4, '/a', struct.pack('>iii', 1, 31, INT32_MAX) + b'world'
                     + A.ustr(b'anyone'), 0),
              S.body(4, '/a', struct.pack('>ii', 1, 31) + A.ustr(b'world') +
                     struct.pack('>i', INT32_MAX - 3) + b'anyone', 0),
              S.body(4, '/a', struct.pack('>ii', 1, 31) + A.ustr(b'world') +
                     struct.pack('>i', 11) + b'anyone', 0),
              # another opcode
              struct.pack('>ii', 5, 6) + good[8:],
              struct.pack('>ii', 5, 1) + good[8:],
              struct.pack('>ii', 5, -1000) + good[8:]]
    # truncated at every length
    n_whole = len(bodies)
    for g in (good, S.body(8, '/a/b', THREE, 1)):
        bodies += [g[:k] for k in range(len(g))]
    cases = [_frame_case(b) for b in bodies] + \
        [_frame_case(b, 13) for b in bodies]
    got = _run(prog, cases, tmp_path)
    for b, g in zip(bodies + bodies, got):
        assert g == _want_frame(b), (b, g)
    assert got[0] == '0 5 2 -1 12 14 %d' % len(OPEN)
    assert got[1] == '0 -7 4 3 12 16 %d' % len(THREE)
    assert got[2] == '0 1 2 0 12 14 300'
    assert [g.split()[0] for g in got[5:8]] == ['2', '2', '2']
    assert got[8].split()[0] == '1'
    assert got[9].split()[0] == got[10].split()[0] == '0'
    assert all(g.split()[0] == '1' for g in got[11:n_whole])
    # no truncation is a request
    assert all(g.split()[0] == '1' for g in got[n_whole:len(bodies)])


def _rule_case(exists, check, kind, addr, aversion, ids, cur, frame):
    blob = struct.pack('<6i', int(exists), int(check), kind, A.as_i32(addr),
                       aversion, -1 if ids is None else len(ids))
    for i in ids or []:
        blob += struct.pack('<i', len(i)) + i
    return (1, 0, 0, blob + struct.pack('<i', len(cur)) + cur + frame)


def _want_rule(exists, check, kind, addr, aversion, ids, cur, frame):
    p = S.parse(frame)
    ok = not check or S.admin(kind, cur, addr, ids)
    return str(S.verdict(p[0], exists, ok, p[3], aversion))


def test_precedence(prog, tmp_path):
    mine = A.vector([(A.ALL, 'digest', U)])
    noadm = A.vector([(A.ALL & ~A.ADMIN, 'world', 'anyone')])
    empty = S.body(1, '/a', struct.pack('>i', 0), 9)
    good9 = S.body(1, '/a', THREE, 9)
    rows = [
        # INVALID_ACL before NO_NODE, NO_AUTH and BAD_VERSION
        ((False, True, S.SA_VECTOR, PEER, 0, [], mine, empty), S.INVALID_ACL),
        ((True, True, S.SA_VECTOR, PEER, 0, [], mine, empty), S.INVALID_ACL),
        # NO_NODE before NO_AUTH and BAD_VERSION
        ((False, True, S.SA_VECTOR, PEER, 0, [], mine, good9), S.NO_NODE),
        # NO_AUTH before BAD_VERSION
        ((True, True, S.SA_VECTOR, PEER, 0, [], mine, good9), S.NO_AUTH),
        ((True, True, S.SA_VECTOR, PEER, 0, [SUPER], mine, good9), S.NO_AUTH),
        ((True, True, S.SA_VECTOR, PEER, 0, None, mine, good9), S.NO_AUTH),
        ((True, True, S.SA_VECTOR, PEER, 0, [U], noadm, good9), S.NO_AUTH),
        # a lost binding denies, the open ACL's word grants without a read
        ((True, True, S.SA_LOST, PEER, 9, [U], b'', good9), S.NO_AUTH),
        ((True, True, S.SA_OPEN, PEER, 9, None, b'', good9), S.OK),
        ((True, True, S.SA_VECTOR, PEER, 0, [U], mine, good9), S.BAD_VERSION),
        ((True, True, S.SA_VECTOR, PEER, 9, [SUPER, U], mine, good9), S.OK),
        ((True, True, S.SA_VECTOR, PEER, 9, None, THREE, good9), S.OK),
        ((True, True, S.SA_VECTOR, 0, 9, None, THREE, good9), S.NO_AUTH),
        # nothing is checked: any ACL lets the frame in
        ((True, False, S.SA_VECTOR, PEER, 9, None, mine, good9), S.OK),
        ((True, False, S.SA_LOST, PEER, 8, None, b'', good9), S.BAD_VERSION),
        ((True, True, S.SA_OPEN, PEER, 123,  None, b'',
          S.body(1, '/a', THREE, -1)), S.OK),
        # no request in the body
        ((True, True, S.SA_OPEN, PEER, 0, None, b'', good9[:-1]),
         S.BAD_ARGUMENTS),
    ]
    got = _run(prog, [_rule_case(*r) for r, _ in rows], tmp_path)
    for (r, want), g in zip(rows, got):
        assert g == str(want) == _want_rule(*r), r


def _random_vector(rng):
    schemes = [b'world', b'ip', b'digest', b'digest', b'auth', b'']
    pool = [b'anyone', b'10.1.2.0/24', b'10.1.3.9/32', U, SUPER, b'']
    n = int(rng.randint(0, 4))
    return A.vector([(int(rng.randint(0, 32)),
                      schemes[int(rng.randint(len(schemes)))],
                      pool[int(rng.randint(len(pool)))]) for _ in range(n)])


def test_random_frames_against_the_mirror(prog, tmp_path):
    rng = np.random.RandomState(31)
    addrs = [PEER, A.addr_of('10.1.3.9'), 0]
    frames, rules = [], []
    for _ in range(300):
        path = b'/' + bytes(rng.randint(97, 123, size=int(rng.randint(0, 9)))
                            .astype(np.uint8).tolist())
        b = S.body(int(rng.randint(-9, 1000)), path, _random_vector(rng),
                   int(rng.randint(-1, 3)))
        roll = rng.randint(0, 8)
        if roll == 0:
            b = b[:int(rng.randint(0, len(b)))]
        elif roll == 1:
            x = bytearray(b)
            x[int(rng.randint(len(x)))] ^= 1 << int(rng.randint(8))
            b = bytes(x)
        elif roll == 2:
            b += bytes(rng.randint(0, 256, size=int(rng.randint(1, 6)))
                       .astype(np.uint8).tolist())
        frames.append(b)
        k = int(rng.randint(0, 4))
        ids = None if k == 3 else [U, SUPER][:k]
        rules.append((bool(rng.randint(0, 4)), bool(rng.randint(0, 4)),
                      int(rng.randint(0, 3)), addrs[int(rng.randint(3))],
                      int(rng.randint(0, 3)), ids, _random_vector(rng), b))
    got = _run(prog, [_frame_case(b, 3) for b in frames] +
               [_rule_case(*r) for r in rules], tmp_path)
    for b, g in zip(frames, got):
        assert g == _want_frame(b), (b, g)
    want = [_want_rule(*r) for r in rules]
    assert got[len(frames):] == want
    # every answer of the rule was reached
    assert {str(c) for c in (S.OK, S.BAD_ARGUMENTS, S.INVALID_ACL, S.NO_NODE,
                             S.NO_AUTH, S.BAD_VERSION)} == set(want)


# ---- routing and the front end's cuts ---------------------------------------

def _frame(op, extra=b'', xid=1):
    body = struct.pack('>ii', xid, op) + extra
    return struct.pack('>i', len(body)) + body


def test_split_rule_sends_opcode_7_to_the_acl_class(prog, tmp_path):
    bodies = [struct.pack('>ii', 1, op) + b'/a' for op in
              (7, 6, 8, 12, 1, 5, 100, 0, -11)] + \
        [struct.pack('>ii', 1, 7), struct.pack('>ii', 1, 7)[:7], b'']
    cases = [(4, h, 0, b) for h in (0, 1) for b in bodies]
    got = _run(prog, cases, tmp_path)
    for (_, h, _, b), g in zip(cases, got):
        assert g == '%d %d' % (S.mix_class(b, h, True),
                               S.mix_class(b, h, False)), (h, b)
    # opcode 7: the ACL class with a table, the serve's without; the first
    # rule never sends it there
    assert got[len(bodies)] == '1 0' and got[0] == '0 0'
    assert got[len(bodies) + 9] == '1 0' and got[len(bodies) + 10] == '0 0'
    assert all(g.split()[0] == g.split()[1] for g, c in zip(got, cases)
               if len(c[3]) < 8 or struct.unpack_from('>i', c[3], 4)[0] != 7)


def test_cuts_take_a_set_acl_frame_alone(prog, tmp_path):
    rd, ga, ls = _frame(4, b'/a\0'), _frame(6, b'/a'), _frame(8, b'/a\0')
    wr, sa, cl = _frame(5, b'/a'), _frame(7, b'/a'), _frame(-11)
    segs = [sa + rd, rd + sa + rd, ga + sa + ga, sa + sa, wr + sa, sa + wr,
            rd + rd + wr, rd + ga + ls + rd + sa, cl + sa, sa[:-1], rd + sa[:-1],
            sa + b'\xff\xff\xff\xff', rd + struct.pack('>i', 1 << 30) + sa,
            wr + wr + rd + sa + wr, ga + wr, b'', sa]
    rng = np.random.RandomState(3)
    pool = [rd, ga, ls, wr, sa, cl, _frame(101, b'\0' * 20), _frame(11)]
    for _ in range(200):
        seg = b''.join(pool[int(rng.randint(len(pool)))]
                       for _ in range(int(rng.randint(0, 7))))
        if rng.randint(4) == 0 and seg:
            seg = seg[:int(rng.randint(len(seg)))]
        segs.append(seg)
    MP = 1 << 20
    cases = []
    for seg in segs:
        for quota in (1, 3, 1 << 40):
            cases.append((2, quota, MP, seg))
            cases.append((3, quota, (MP << 1) | 1, seg))
            cases.append((3, quota, MP << 1, seg))
    got = _run(prog, cases, tmp_path)
    for (kind, quota, b, seg), g in zip(cases, got):
        want = S.walk(seg, quota, MP) if kind == 2 else \
            S.walk_ordered(seg, quota, MP, b & 1)
        assert g == ' '.join(str(x) for x in want), (kind, quota, seg)
    by = {(c[0], c[1], c[2] & 1, c[3]): g for c, g in zip(cases, got)}
    big = 1 << 40
    n = len(sa)
    # first of its run: taken, and alone
    assert by[(2, big, 0, sa + rd)] == '%d 1 0' % n
    assert by[(3, big, 1, sa + rd)] == '%d 1 0 0' % n
    # behind reads: the run ends in front of it
    assert by[(2, big, 0, rd + sa + rd)] == '%d 1 0' % len(rd)
    assert by[(3, big, 1, ga + sa + ga)] == '%d 1 0 0' % len(ga)
    assert by[(3, big, 1, wr + wr + rd + sa + wr)] == \
        '%d 3 0 2' % (2 * len(wr) + len(rd))
