"""The rule of AUTH with digest identities on the host: csrc/kernels/
zk_auth.h (auth_frame, auth_sha1, auth_b64, auth_identity, auth_match,
aclperm_permits_auth — the text tree_auth.hip runs) compiled by g++ into
tools/auth_host.cpp with ASan + UBSan, a stand-alone program run as a child
process with nothing preloaded.  Every frame, credential, vector and record
block sits in a heap block of exactly its length, so a read past one is a
sanitizer report; the output is compared with ``hashlib`` / ``base64`` and
the Python mirror (tests/auth_model.py), on a machine without a GPU."""

import base64
import hashlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import aclperm_model as A
import auth_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1
INT32_MIN = -2 ** 31
# the padding and block edges of SHA-1 for messages of at most 119 bytes
EDGES = (0, 1, 54, 55, 56, 57, 63, 64, 65, 118, 119)


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
    exe = str(tmp_path_factory.mktemp('auth') / 'auth_host')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror',
         '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'auth_host.cpp'), '-o', exe],
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


def _cred(n, seed=0):
    """n credential bytes, 'user:' first where they fit."""
    rng = np.random.RandomState(1000 * seed + n)
    raw = bytes(rng.randint(1, 256, size=n).astype(np.uint8).tolist())
    raw = raw.replace(b':', b';')
    return (b'usr:' + raw[4:]) if n >= 5 else raw


def test_sha1_and_b64_edges(prog, tmp_path):
    msgs = [_cred(n) for n in EDGES] + [b'\x00' * n for n in EDGES] + \
        [b'\xff' * n for n in (55, 56, 119)] + [b'abc', b'super:test', b'u:pw']
    got = _run(prog, [(1, 0, 0, m) for m in msgs], tmp_path)
    for m, g in zip(msgs, got):
        assert g == hashlib.sha1(m).hexdigest(), len(m)
    hs = [hashlib.sha1(m).digest() for m in msgs] + [b'\x00' * 20,
                                                     b'\xff' * 20,
                                                     bytes(range(236, 256))]
    got = _run(prog, [(2, 0, 0, h) for h in hs], tmp_path)
    for h, g in zip(hs, got):
        assert g == base64.b64encode(h).decode()


def test_identities(prog, tmp_path):
    creds = [_cred(n) for n in EDGES] + [
        b'super:test', b'u:pw',
        # no ':' at all: the whole of it is the user
        b'nocolon', b'x' * 119, b'',
        # two: the user ends at the first
        b'a:b:c', b'::', b':pw', b'user:', b'a' * 117 + b':b', b':' * 119]
    got = _run(prog, [(3, 0, 0, c) for c in creds], tmp_path)
    for c, g in zip(creds, got):
        assert bytes.fromhex(g) == M.identity(c), c
        assert len(bytes.fromhex(g)) <= 148
    by = dict(zip(creds, got))
    # recorded vectors (ZooKeeper's DigestAuthenticationProvider)
    assert bytes.fromhex(by[b'super:test']) == \
        b'super:D/InIHSb7yEEbrWz8b9l71RjZJU='
    assert bytes.fromhex(by[b'u:pw']) == b'u:BvFaefuhWURhnvpD7ipe45CKTpk='
    assert bytes.fromhex(by[b'nocolon']).startswith(b'nocolon:')
    assert bytes.fromhex(by[b'a:b:c']).startswith(b'a:') and \
        len(bytes.fromhex(by[b'a:b:c'])) == 2 + 28
    assert len(bytes.fromhex(by[b'x' * 119])) == 148


def _frame_case(b, base=0):
    return (0, base, 0, b'\xaa' * base + b)


def _want_frame(b):
    return '%d %d %d %d %d' % M.parse(b)


def test_auth_frame(prog, tmp_path):
    good = M.body(-4, b'digest', b'u:pw')
    assert len(good) == 30
    bodies = [good, M.body(7, b'digest', b''), M.body(7, b'digest', b'x' * 119),
              M.body(7, b'digest', b'x' * 120), M.body(7, b'digest', b'x' * 500),
              M.body(1, b'ip', b'u:pw'), M.body(1, b'', b'u:pw'),
              M.body(1, b'digestx', b'u:pw'), M.body(1, b'diges', b'u:pw'),
              M.body(1, b'Digest', b'u:pw'), M.body(2, b'digest', b'u:pw', 99),
              # bytes behind `auth`
              good + b'\x00', good + good,
              # another opcode
              struct.pack('>ii', 5, 4) + good[8:],
              struct.pack('>ii', 5, -1000) + good[8:]]
    # truncated at every length
    bodies += [good[:k] for k in range(len(good))]
    # negative lengths read as empty
    for sl in (-1, INT32_MIN):
        bodies.append(struct.pack('>iiii', 3, 100, 0, sl) + A.ustr(b'u:pw'))
        bodies.append(struct.pack('>iii', 3, 100, 0) + A.ustr(b'digest') +
                      struct.pack('>i', sl))
        bodies.append(struct.pack('>iii', 3, 100, 0) + A.ustr(b'digest') +
                      struct.pack('>i', sl) + b'u:pw')
    # lengths that run past the frame, and the largest
    for al in (5, 6, 100, 120, INT32_MAX):
        bodies.append(struct.pack('>iii', 3, 100, 0) + A.ustr(b'digest') +
                      struct.pack('>i', al) + b'u:pw')
        bodies.append(struct.pack('>iiii', 3, 100, 0, al) + b'digest' +
                      A.ustr(b'u:pw'))
    cases = [_frame_case(b) for b in bodies] + \
        [_frame_case(b, 13) for b in bodies]
    got = _run(prog, cases, tmp_path)
    for b, g in zip(bodies + bodies, got):
        assert g == _want_frame(b), (b, g)
    assert got[0] == '0 -4 0 4 26'
    assert got[2].split()[0] == '0' and got[3].split()[0] == '3'
    assert got[5].split()[0] == '2'
    assert got[11].split()[0] == got[12].split()[0] == '1'
    assert all(g.split()[0] == '1' for g in got[15:15 + len(good)])


def _permits_case(perm, addr, ids, vec):
    blob = struct.pack('<i', len(ids))
    for i in ids:
        blob += struct.pack('<i', len(i)) + i
    return (5, perm, addr, blob + vec)


PEER = A.addr_of('10.1.2.9')
U = M.identity(b'u:pw')
SUPER = M.identity(b'super:test')
LONG = M.identity(b'x' * 119)


def test_digest_entries(prog, tmp_path):
    ro = A.vector([(A.READ, 'digest', U)])
    two = A.vector([(A.READ, 'digest', SUPER), (A.WRITE, 'digest', U),
                    (A.ADMIN, 'auth', b''), (A.ADMIN, 'sasl', U),
                    (A.DELETE, 'digest', LONG)])
    near = A.vector([(A.ALL, 'digest', U[:-1]), (A.ALL, 'digest', U + b'='),
                     (A.ALL, 'digest', b''), (A.ALL, 'digest', b'u:'),
                     (A.ALL, 'Digest', U), (A.ALL, 'digests', U)])
    cases, want = [], []
    for vec in (ro, two, near):
        for perm in (A.READ, A.WRITE, A.DELETE, A.ADMIN):
            for ids in ([], [U], [SUPER], [SUPER, U], [LONG, U[:-1] + b'x'],
                        [U, U, U, U], [b'', b'u:']):
                cases.append(_permits_case(perm, PEER, ids, vec))
                want.append(str(int(M.permits_auth(vec, perm, PEER, ids))))
    got = _run(prog, cases, tmp_path)
    assert got == want
    g = {(c[1], c[3]): x for c, x in zip(cases, got)}
    assert g[_permits_case(A.READ, PEER, [U], ro)[1::2]] == '1'
    assert g[_permits_case(A.READ, PEER, [], ro)[1::2]] == '0'
    assert g[_permits_case(A.READ, PEER, [SUPER], ro)[1::2]] == '0'
    assert g[_permits_case(A.WRITE, PEER, [U], ro)[1::2]] == '0'
    assert g[_permits_case(A.DELETE, PEER, [LONG, U[:-1] + b'x'],
                           two)[1::2]] == '1'
    # auth and sasl entries match nobody, whatever the connection holds
    assert g[_permits_case(A.ADMIN, PEER, [SUPER, U], two)[1::2]] == '0'
    assert all(x == '0' for c, x in zip(cases, got) if c[3].endswith(near))


def _random_vector(rng, idents):
    schemes = [b'world', b'ip', b'digest', b'digest', b'auth', b'sasl', b'']
    pool = [b'anyone', b'10.1.2.0/24', b'10.1.3.9/32', b'u:pw', b''] + idents
    n = int(rng.randint(0, 5))
    v = A.vector([(int(rng.randint(0, 32)),
                   schemes[int(rng.randint(len(schemes)))],
                   pool[int(rng.randint(len(pool)))]) for _ in range(n)])
    roll = rng.randint(0, 10)
    if roll == 0 and len(v) > 4:
        v = v[:int(rng.randint(0, len(v)))]
    elif roll == 1:
        b = bytearray(v)
        b[int(rng.randint(len(b)))] ^= 1 << int(rng.randint(8))
        v = bytes(b)
    return v


def test_random_vectors_against_the_mirror(prog, tmp_path):
    rng = np.random.RandomState(23)
    idents = [U, SUPER, LONG, M.identity(b'nocolon'), M.identity(b'a:b:c')]
    addrs = [PEER, A.addr_of('10.1.3.9'), 0]
    cases, want, plain = [], [], []
    for _ in range(400):
        vec = _random_vector(rng, idents)
        perm = 1 << int(rng.randint(0, 5))
        addr = addrs[int(rng.randint(len(addrs)))]
        k = int(rng.randint(0, 5))
        ids = [idents[int(rng.randint(len(idents)))] for _ in range(k)]
        cases.append(_permits_case(perm, addr, ids, vec))
        want.append(str(int(M.permits_auth(vec, perm, addr, ids))))
        # with no identities: aclperm_permits itself, on the same vector
        cases.append(_permits_case(perm, addr, [], vec))
        want.append(str(int(A.permits(vec, perm, addr))))
        plain.append((4, perm, addr, vec))
    got = _run(prog, cases + plain, tmp_path)
    assert got[:len(cases)] == want
    assert got[len(cases):] == got[1:len(cases):2]
    assert {'0', '1'} == set(got[0:len(cases):2])
    # a digest entry did decide some of them
    assert got[0:len(cases):2] != got[1:len(cases):2]
