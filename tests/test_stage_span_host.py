"""The index arithmetic of the consumers' frame staging on the host:
csrc/kernels/zk_stage_span.h (span_fits, span_make, span_load_chunk — the
text zk_frame_rows.h fr_span_load / fr_span_store run) compiled by g++ into
tools/stage_span_host.cpp with ASan + UBSan, a stand-alone program run as a
child process with nothing preloaded.  Every stream sits in a heap block of
exactly its length, so a read one byte outside it is a sanitizer report; the
image is compared with a byte-wise copy for every head alignment 0..15 and
every tail 0..15, on a machine without a GPU."""

import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRV_STAGE = 4096              # csrc/kernels/tree.hip: a wave's image


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
    exe = str(tmp_path_factory.mktemp('sspan') / 'stage_span_host')
    r = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all',
         '-I' + os.path.join(ROOT, 'csrc', 'kernels'),
         os.path.join(ROOT, 'tools', 'stage_span_host.cpp'), '-o', exe],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(prog, budget, spans):
    r = subprocess.run([prog, str(budget)] + [str(s) for s in spans],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return [ln.split() for ln in r.stdout.splitlines()]


ALL = 6 * 16 * 16             # starts x tails x alignments


def _staged(budget, span):
    """Cases whose head + span fits the image: the heads 0 .. budget - span
    (one alignment in 16 each)."""
    return 6 * 16 * min(max(budget - span + 1, 0), 16)


def test_spans_of_the_serve(prog):
    """The spans of the GPU test's streams — 64 requests of 41-byte bodies,
    of long paths, a short wave, one frame, nothing — and spans around the
    budget: one of budget - 15 bytes is staged at every alignment, one of
    budget - 4 at heads 0..4, one of the budget only at head 0, one byte
    more never, nor a frame larger than the image."""
    spans = [64 * 45 - 4, 64 * 62 - 4, 22 * 45 - 4, 41, 1, 0, 15, 16, 17,
             SRV_STAGE - 16, SRV_STAGE - 15, SRV_STAGE - 14, SRV_STAGE - 4,
             SRV_STAGE - 1, SRV_STAGE, SRV_STAGE + 1, SRV_STAGE + 5000]
    out = _run(prog, SRV_STAGE, spans)
    assert [int(o[0]) for o in out] == spans
    assert [int(o[1]) for o in out] == [_staged(SRV_STAGE, s) for s in spans]
    assert int(out[0][1]) == ALL and int(out[-5][1]) == 6 * 16 * 5
    assert int(out[-3][1]) == 6 * 16 and int(out[-2][1]) == 0


def test_other_budgets(prog):
    """A 3 KiB image (16 replies at 192 B pitch: 3068 bytes) and a 12 KiB
    one (64 of them)."""
    for budget, spans in ((3072, [16 * 192 - 4, 16 * 129 - 4, 3057, 3072,
                                  3073]),
                          (12288, [64 * 192 - 4, 12288, 12289])):
        out = _run(prog, budget, spans)
        assert [int(o[1]) for o in out] == [_staged(budget, s)
                                            for s in spans]
