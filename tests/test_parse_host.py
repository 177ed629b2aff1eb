"""The device request parser on the host: csrc/kernels/zk_wire.h
(parse_request, skip_strings, skip_acl — the text the GPU server's kernels
run) compiled by g++ into tools/fuzz_reqparse.cpp with ASan + UBSan, a
stand-alone program.  Memory safety on generated and mutated bodies, each in
a heap block of exactly its length, and parity with the Jute oracle on the
request corpus of tests/test_gpu_decode_malformed.py — on a machine without
a GPU."""

import os
import shutil
import struct
import subprocess

import pytest
import torch

import malformed_corpus as M

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
    exe = str(tmp_path_factory.mktemp('fuzz') / 'fuzz_reqparse')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'fuzz_reqparse.cpp'), '-o', exe],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(args):
    env = {k: v for k, v in os.environ.items() if k != 'LD_PRELOAD'}
    return subprocess.run(args, capture_output=True, text=True, timeout=300,
                          env=env)


def test_fuzz_clean(prog):
    r = _run([prog, '--fuzz', '200000', '1'])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'fuzz: 200000 bodies' in r.stdout


def test_corpus_matches_oracle(prog, tmp_path):
    c = M.RequestCorpus()
    path = str(tmp_path / 'requests.bin')
    with open(path, 'wb') as f:
        f.write(c.stream())
    r = _run([prog, '--corpus', path])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(c.bodies)
    cols = ('status', 'xid', 'opcode', 'arg', 'path_off', 'path_len',
            'data_off', 'data_len', 'vec_count', 'rel_zxid')
    seen = []
    for body, line in zip(c.bodies, lines):
        row = dict(zip(cols, (int(x) for x in line.split())))
        st, want = M.expect_request(body)
        seen.append(st)
        if st == M.SKIP:
            continue
        if st != M.ST_OK:
            assert row['status'] == st, (body.hex(), line)
            continue
        M.check_request_row(body, 0, row, want)
    share = M.stats(seen)
    print('left out (text only): %.2f %%' % (100 * share[M.SKIP]))
    assert share[M.SKIP] <= 0.02
    for k in (M.ST_OK, M.ST_BAD_DECODE, M.ST_BAD_OPCODE):
        assert share[k] > 0
    # the length prefix of the file format is the stream's own framing
    assert struct.unpack_from('>i', c.stream())[0] == len(c.bodies[0])
