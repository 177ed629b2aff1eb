"""The mixed-batch class function on the host: csrc/kernels/zk_mix.h
(mix_class — the text the split kernel of csrc/kernels/tree_mix.hip runs)
compiled by g++ into tools/mix_class_host.cpp with ASan + UBSan, a
stand-alone program.  Every body sits in a heap block of exactly its length;
the classes are compared with a Python model of the rule: the opcode word
alone decides, a body without one goes to the serve, GET_ACL goes to the ACL
engine only on a tree with an ACL table — on a machine without a GPU."""

import os
import shutil
import struct
import subprocess

import pytest
import torch

import malformed_corpus as M
from zkmi import consts, jute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX_A, MIX_C, MIX_L = 0, 1, 2


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


def model(body, has_acl):
    """The rule of the issue, from the bytes alone."""
    if len(body) < 8:
        return MIX_A
    op = struct.unpack_from('>i', body, 4)[0]
    if op in (consts.OP_CODES['GET_CHILDREN'],
              consts.OP_CODES['GET_CHILDREN2']):
        return MIX_L
    if op == consts.OP_CODES['GET_ACL'] and has_acl:
        return MIX_C
    return MIX_A


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('mix') / 'mix_class_host')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'mix_class_host.cpp'), '-o', exe],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _classes(prog, bodies, has_acl, tmp_path):
    path = str(tmp_path / ('frames%d.bin' % has_acl))
    with open(path, 'wb') as f:
        f.write(b''.join(jute.frame(b) for b in bodies))
    env = {k: v for k, v in os.environ.items() if k != 'LD_PRELOAD'}
    r = subprocess.run([prog, path, str(int(has_acl))], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return [int(x) for x in r.stdout.split()]


def _well_formed():
    acl = jute.DEFAULT_ACL
    pk = [
        {'opcode': 'GET_DATA', 'path': '/a', 'watch': False},
        {'opcode': 'EXISTS', 'path': '/a', 'watch': True},
        {'opcode': 'SET_DATA', 'path': '/a', 'data': b'x', 'version': -1},
        {'opcode': 'CREATE', 'path': '/a/b', 'data': b'', 'acl': acl,
         'flags': []},
        {'opcode': 'DELETE', 'path': '/a/b', 'version': -1},
        {'opcode': 'SYNC', 'path': '/a'},
        {'opcode': 'GET_CHILDREN', 'path': '/a', 'watch': False},
        {'opcode': 'GET_CHILDREN2', 'path': '/a', 'watch': True},
        {'opcode': 'GET_ACL', 'path': '/a'},
        {'opcode': 'PING'},
    ]
    return [jute.encode_request(dict(p, xid=7 + i)) for i, p in enumerate(pk)]


@pytest.mark.parametrize('has_acl', [False, True])
def test_classes_match_the_model(prog, tmp_path, has_acl):
    good = _well_formed()
    bodies = list(good)
    # every prefix of every well-formed body: the frames without an opcode
    # word (0..7 bytes) and the truncated list / GET_ACL frames among them
    for b in good:
        bodies += [b[:k] for k in range(len(b))]
    # the opcode word replaced: unknown, negative and neighbouring values
    for op in (0, 7, 10, 13, 14, 100, 9999, -1, -11, -2**31, 2**31 - 1,
               6 << 8, 8 << 24, 12 << 16):
        bodies.append(good[0][:4] + struct.pack('>i', op) + good[0][8:])
    # the generated and mutated request corpus of the decoder tests
    bodies += M.RequestCorpus().bodies
    got = _classes(prog, bodies, has_acl, tmp_path)
    want = [model(b, has_acl) for b in bodies]
    assert len(got) == len(bodies)
    bad = [(i, bodies[i][:12].hex(), g, w)
           for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:5]
    seen = set(want)
    assert seen == ({MIX_A, MIX_C, MIX_L} if has_acl else {MIX_A, MIX_L})
    # a truncated list frame stays a list frame, a truncated GET_ACL frame a
    # GET_ACL frame; a 6-byte frame goes to the serve
    assert model(good[6][:9], has_acl) == MIX_L
    assert model(good[8][:9], True) == MIX_C
    assert model(good[0][:6], has_acl) == MIX_A
