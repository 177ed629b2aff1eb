"""The tree image's structural checks on the host: csrc/kernels/zk_snap.h
(snap_check_header, snap_check_table, snap_check_record — the text the
load's check kernels run) compiled by g++ into tools/fuzz_snap.cpp with
ASan + UBSan, a stand-alone program.  Memory safety on generated and mutated
images, each in a heap block of exactly its length, and parity with
zkmi.utils.treeimage.check on the corpus of tests/image_corpus.py — on a
machine without a GPU."""

import os
import shutil
import subprocess

import pytest
import torch

import image_corpus as C
from zkmi.utils import treeimage as TI

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
    exe = str(tmp_path_factory.mktemp('fuzz') / 'fuzz_snap')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'fuzz_snap.cpp'), '-o', exe],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


def test_fuzz_clean(prog):
    r = _run([prog, '--fuzz', '100000', '1'])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'fuzz: 100000 images' in r.stdout


def test_corpus_matches_host_codec(prog, tmp_path):
    corpus = C.corpus()
    path = str(tmp_path / 'images.bin')
    with open(path, 'wb') as f:
        f.write(C.stream([c[1] for c in corpus]))
    r = _run([prog, '--corpus', path])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(corpus)
    for (name, img, _), line in zip(corpus, lines):
        got = tuple(int(x) for x in line.split())
        want = TI.check(img)
        if want[0] > TI.BAD_RECORD:       # the set's checks are the loader's
            want = (TI.OK, -1)
        assert got == want, (name, got, want)
