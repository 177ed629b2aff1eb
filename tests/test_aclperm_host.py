"""The rule of ACL enforcement on the host: csrc/kernels/zk_aclperm.h
(aclperm_need, aclperm_ip_match, aclperm_permits — the text tree_aclperm.hip
runs) compiled by g++ into tools/aclperm_host.cpp with ASan + UBSan, a
stand-alone program run as a child process with nothing preloaded.  Every
vector and every id sits in a heap block of exactly its length, so a read past
one is a sanitizer report; the output is compared with the Python mirror
(tests/aclperm_model.py), on a machine without a GPU."""

import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import aclperm_model as A

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
    exe = str(tmp_path_factory.mktemp('aclperm') / 'aclperm_host')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'aclperm_host.cpp'), '-o', exe],
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


def want(case):
    kind, a, b, raw = case
    if kind == 0:
        return '%d %d' % A.need(a)
    if kind == 1:
        return str(int(A.ip_match(raw, a)))
    if kind == 2:
        return str(int(A.permits(raw, a, b)))
    return str(A.parent_cut(raw))


def _check(prog, cases, tmp_path):
    got = _run(prog, cases, tmp_path)
    for k, (c, g) in enumerate(zip(cases, got)):
        assert g == want(c), (k, c, g)
    return got


PEER = A.addr_of('10.1.2.9')
OTHER = A.addr_of('10.1.3.9')


def test_need_every_opcode(prog, tmp_path):
    ops = sorted(set(A.OPS.values()) | {0, 10, 15, -1, -1000, INT32_MAX,
                                        INT32_MIN})
    got = _check(prog, [(0, op, 0, b'') for op in ops], tmp_path)
    by = dict(zip(ops, got))
    assert by[4] == by[8] == by[12] == '1 1'            # READ on the node
    assert by[5] == '2 1'                               # WRITE on the node
    assert by[1] == '4 2'                               # CREATE on the parent
    assert by[2] == '8 3'                               # DELETE on the parent
    for op in ops:
        if op not in (1, 2, 4, 5, 8, 12):
            assert by[op] == '0 0', op


def test_ip_ids(prog, tmp_path):
    ids = [b'10.1.2.0/0', b'10.1.2.0/1', b'138.1.2.0/1', b'10.1.2.0/24',
           b'10.1.2.9/32', b'10.1.2.9', b'10.1.2.8', b'10.1.2.0/33',
           b'10.1.2', b'10.1.2.256', b'10..2.9', b'10.1.2.9.', b'10.1.2.',
           b'10.1.2.0009', b'0010.1.2.9', b'10.1.2.9/', b'10.1.2.9/024',
           b'10.1.2.9/2x', b'10.1.2.9 ', b' 10.1.2.9', b'10.1.2.9/-1',
           b'10.1.2.9/08', b'010.001.002.009', b'', b'/', b'.', b'...',
           b'10.1.2.9/32/', b'10.1.2.9.1', b'a.b.c.d', b'10.1.3.0/23',
           b'10.1.3.0/24', b'255.255.255.255/32', b'0.0.0.0/0', b'10.1.2.9/3']
    cases = [(1, addr, 0, i) for i in ids
             for addr in (PEER, OTHER, 0, 0xFFFFFFFF, 1)]
    got = _check(prog, cases, tmp_path)
    g = {(c[3], c[1]): x for c, x in zip(cases, got)}
    assert g[(b'10.1.2.0/0', PEER)] == '1' and g[(b'10.1.2.0/0', 1)] == '1'
    assert g[(b'10.1.2.0/1', PEER)] == '1'
    assert g[(b'138.1.2.0/1', PEER)] == '0'
    assert g[(b'10.1.2.0/24', PEER)] == '1'
    assert g[(b'10.1.2.0/24', OTHER)] == '0'
    assert g[(b'10.1.2.9/32', PEER)] == '1' and g[(b'10.1.2.9', PEER)] == '1'
    assert g[(b'10.1.2.8', PEER)] == '0'
    for bad in (b'10.1.2.0/33', b'10.1.2', b'10.1.2.256', b'10..2.9',
                b'10.1.2.9.', b'10.1.2.0009', b'10.1.2.9/', b'10.1.2.9/024'):
        assert g[(bad, PEER)] == '0', bad
    # no IPv4 identity: nothing matches, not even /0
    assert all(x == '0' for c, x in zip(cases, got) if c[1] == 0)


def _vec_cases():
    ro = A.vector([(A.READ, 'world', 'anyone')])
    three = A.vector([(A.READ, 'digest', 'u:h'), (A.READ, 'ip', '10.1.2.0/24'),
                      (A.ALL, 'ip', '10.1.3.9')])
    # the first matching entry lacks the bit, a later one has it
    later = A.vector([(A.READ, 'world', 'anyone'), (0, 'world', 'anyone'),
                      (A.WRITE | A.CREATE, 'ip', '10.1.2.9/32')])
    zero = A.vector([(0, 'world', 'anyone'), (0, 'ip', '10.1.2.9')])
    other = A.vector([(A.ALL, 'world', 'somebody'), (A.ALL, 'world', ''),
                      (A.ALL, 'World', 'anyone'), (A.ALL, 'worl', 'anyone'),
                      (A.ALL, 'worldx', 'anyone'), (A.ALL, '', 'anyone')])
    digest = A.vector([(A.ALL, 'digest', 'anyone'), (A.ALL, 'auth', ''),
                       (A.ALL, 'sasl', 'anyone'), (A.ALL, 'x509', 'anyone')])
    return [ro, three, later, zero, other, digest, A.vector([])]


def test_vectors(prog, tmp_path):
    cases = [(2, perm, addr, v) for v in _vec_cases()
             for perm in (A.READ, A.WRITE, A.CREATE, A.DELETE, A.ADMIN)
             for addr in (PEER, OTHER, 0)]
    got = _check(prog, cases, tmp_path)
    vs = _vec_cases()
    g = {(vs.index(c[3]), c[1], c[2]): x for c, x in zip(cases, got)}
    assert g[(0, A.READ, 0)] == '1' and g[(0, A.WRITE, PEER)] == '0'
    assert g[(1, A.READ, PEER)] == '1' and g[(1, A.READ, 0)] == '0'
    assert g[(1, A.WRITE, PEER)] == '0' and g[(1, A.WRITE, OTHER)] == '1'
    assert g[(2, A.WRITE, PEER)] == '1' and g[(2, A.WRITE, OTHER)] == '0'
    assert g[(2, A.DELETE, PEER)] == '0'
    for k in (3, 4, 5, 6):
        assert all(x == '0' for key, x in g.items() if key[0] == k), k


def test_truncated_and_hostile(prog, tmp_path):
    cases = []
    for v in _vec_cases()[:3]:
        for cutat in range(len(v) + 1):
            for perm, addr in ((A.READ, PEER), (A.WRITE, OTHER)):
                cases.append((2, perm, addr, v[:cutat]))
    ent = struct.pack('>i', A.ALL) + A.ustr(b'world') + A.ustr(b'anyone')
    # counts: -1, 0, more than the bytes, the largest
    for n in (-1, 0, 2, 3, 1000, INT32_MAX, INT32_MIN):
        cases.append((2, A.READ, PEER, struct.pack('>i', n) + ent))
        cases.append((2, A.READ, PEER, struct.pack('>i', n) + ent + ent))
    # string lengths: negative (Jute's null: empty), past the vector, huge
    for sl in (-1, INT32_MIN, 6, 100, INT32_MAX):
        bad_s = struct.pack('>iii', 2, A.ALL, sl) + b'world' + A.ustr(
            b'anyone') + ent
        bad_i = struct.pack('>ii', 2, A.ALL) + A.ustr(b'world') + \
            struct.pack('>i', sl) + b'anyone' + ent
        cases += [(2, A.READ, PEER, bad_s), (2, A.READ, PEER, bad_i)]
    # a grant before the fault stands, one behind it is never reached
    cases.append((2, A.READ, PEER, struct.pack('>i', 5) + ent + b'\xff' * 7))
    cases.append((2, A.READ, PEER, struct.pack('>i', 5) +
                  struct.pack('>i', 0) + A.ustr(b'ip') +
                  struct.pack('>i', 99) + ent))
    got = _check(prog, cases, tmp_path)
    assert got[-2] == '1' and got[-1] == '0'
    # the whole one-entry vector grants, every proper prefix of it denies
    n0 = 2 * (len(_vec_cases()[0]) + 1)
    assert got[n0 - 2] == '1' and all(x == '0' for x in got[0:n0 - 2:2])


def test_parent_cut(prog, tmp_path):
    paths = [b'', b'/', b'/a', b'/a/b', b'/a/b/', b'a', b'//', b'/ab/cd/ef',
             b'ab/cd']
    got = _check(prog, [(3, 0, 0, p) for p in paths], tmp_path)
    assert got == ['0', '0', '0', '2', '4', '0', '1', '6', '2']


def random_vector(rng):
    """A vector as a CREATE could send it, or a damaged one."""
    schemes = [b'world', b'ip', b'digest', b'auth', b'', b'ipx']
    idents = [b'anyone', b'10.1.2.0/24', b'10.1.2.9', b'10.1.3.9/32',
              b'10.0.0.0/8', b'0.0.0.0/0', b'10.1.2', b'10.1.2.300', b'u:pw',
              b'']
    n = int(rng.randint(0, 5))
    v = A.vector([(int(rng.randint(0, 32)),
                   schemes[int(rng.randint(len(schemes)))],
                   idents[int(rng.randint(len(idents)))]) for _ in range(n)])
    roll = rng.randint(0, 10)
    if roll == 0 and len(v) > 4:
        v = v[:int(rng.randint(0, len(v)))]
    elif roll == 1:
        b = bytearray(v)
        b[int(rng.randint(len(b)))] ^= 1 << int(rng.randint(8))
        v = bytes(b)
    return v


def test_random_vectors(prog, tmp_path):
    rng = np.random.RandomState(11)
    addrs = [PEER, OTHER, 0, A.addr_of('10.9.9.9'), A.addr_of('192.168.0.1')]
    cases = [(2, 1 << int(rng.randint(0, 5)),
              addrs[int(rng.randint(len(addrs)))], random_vector(rng))
             for _ in range(300)]
    got = _check(prog, cases, tmp_path)
    assert {'0', '1'} == set(got)
