"""The arithmetic of K1's run gather on the host: csrc/kernels/zk_run_span.h
(run_want, run_word_in, run_accept, run_tiles_covered, run_tile — the text
zk_frame_tile.h ft_gather_issue / ft_gather_take run) compiled by g++ into
tools/run_span_host.cpp with ASan + UBSan, a stand-alone program run as a
child process with nothing preloaded.  Every stream sits in a heap block of
exactly its length, so a length word read one byte outside it is a sanitizer
report; the records the run arithmetic gives each covered tile are compared
with a byte-by-byte walk, for every entry offset in the first 256 bytes,
groups of 2, 4, 8 and 16 tiles and stream ends in every tile of the group, on
a machine without a GPU."""

import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [20, 45, 88, 192, 252, 1000, 4096]


def _have_asan():
    if shutil.which('gcc') is None or shutil.which('g++') is None:
        return False
    lib = subprocess.run(['gcc', '-print-file-name=libasan.so'],
                         capture_output=True, text=True).stdout.strip()
    return os.path.isabs(lib) and os.path.exists(lib)


pytestmark = [
    pytest.mark.skipif(not _have_asan(), reason='no g++ ASan runtime'),
    pytest.mark.skipif(torch.cuda.is_available(),
                       reason='sanitizer runs belong on the CPU box'),
]


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('rspan') / 'run_span_host')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'run_span_host.cpp'), '-o', exe],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_runs_against_the_walk(prog):
    """Frame sizes 20, 45 (odd: unaligned words), 88, 192, 252, and 1000
    and 4096 (one frame a tile): every
    case's covered tiles carry the walk's records, and the gather stops at
    the tile the walk cannot leave."""
    r = subprocess.run([prog] + [str(s) for s in SIZES], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out = [ln.split() for ln in r.stdout.splitlines()]
    assert [int(o[0]) for o in out] == SIZES
    # 256 entries x (1 + 3 + 7 + 15) end tiles x up to 5 ends, most of them
    # distinct
    assert all(int(o[1]) > 256 * 26 * 3 for o in out)


def test_sizes_out_of_range_are_refused(prog):
    """The gather is taken for frames of 16 bytes up to a tile."""
    for s in ('15', '4097'):
        r = subprocess.run([prog, s], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 2
