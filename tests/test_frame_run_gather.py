"""K1's group tail on runs of equal frames: a wave that leaves its mapped
tile after two frames of one size takes the run's length words by gather
from global memory and writes the covered tiles' records from arithmetic
(csrc/kernels/zk_frame_tile.h ft_gather_issue / ft_gather_take,
zk_run_span.h); the tile the run breaks in, and every group that is not in a
run, takes the staged walk.

Every case is differential on one stream: ``FrameScanner(group=G)`` against
``FrameScanner(group=1)`` and against the host framer — the count, every
(offset, length) row, the stop offset (the carried partial tail starts
there), the BAD_LENGTH flag and its frame — and the rows-deferred scan read
through ``decode_replies(..., tiles=)`` against the same rows.

Which path a case takes: the gather is compiled into the 256-byte window's
grouped instances and taken where the chain LEAVES A GROUP'S FIRST TILE in a
run.  The W = 512 parametrisations, and a run that begins later in a group
(``test_run_begins_in_the_third_tile``), therefore take the staged walk with
the frame size carried from tile to tile (``ft_walk``'s ``last``), not the
gather; they are here because the issue sets them and because the carried
state is new."""

import numpy as np
import pytest
import torch

from zkmi import codec
from zkmi.ops import batch as B

pytestmark = pytest.mark.gpu

TILE = 4096
MAXP = 4096                    # the scanners' max_packet in these tests
GROUPS = [2, 4, 8]
WINDOWS = [256, 512]
SIZES = [20, 45, 88, 192, 252]


@pytest.fixture(scope='module')
def xt(gpu):
    return B.XidTable(bits=16, device=gpu)


def _build(rng, sizes, fill=None):
    """Frames of the given sizes (header included) back to back: the bytes
    and the frame starts.  ``fill``: a 4-byte pattern every body repeats
    (default: random bytes)."""
    sizes = np.asarray(sizes, np.int64)
    starts = np.zeros(len(sizes), np.int64)
    np.cumsum(sizes[:-1], out=starts[1:])
    total = int(starts[-1] + sizes[-1])
    if fill is None:
        buf = rng.integers(0, 256, total, dtype=np.uint8)
    else:
        buf = np.zeros(total, np.uint8)
        body = np.arange(total) - np.repeat(starts, sizes)
        buf[:] = np.asarray(fill, np.uint8)[body % 4]
    lens = sizes - 4
    for k in range(4):
        buf[starts + k] = ((lens >> (8 * (3 - k))) & 0xff).astype(np.uint8)
    return buf, starts


def _equal(rng, S, nbytes, fill=None):
    return _build(rng, np.full(max(nbytes // S, 1), S), fill)


def _put(buf, at, value):
    buf[at:at + 4] = np.frombuffer(int(value).to_bytes(4, 'big', signed=True),
                                   np.uint8)


def _host(raw):
    frames, stop, bad = codec.scan_frames(raw, 0, len(raw), MAXP)
    off = np.fromiter((o for o, _ in frames), np.int64, len(frames))
    ln = np.fromiter((l for _, l in frames), np.int64, len(frames))
    return off, ln, stop, bad >= 0


def _rows(ft):
    res = ft.result.cpu().tolist()
    n = res[0]
    return res, ft.off[:n].cpu().numpy(), \
        ft.length[:n].cpu().numpy().astype(np.int64)


def _check(gpu, xt, buf, G, W, n=None, **kw):
    """The grouped scan, the rows-deferred grouped scan and the host framer
    against the one-tile-a-wave scan of the same bytes.  Returns the
    result."""
    d = torch.from_numpy(np.ascontiguousarray(buf)).to(gpu)
    ln = len(buf) if n is None else n
    nb = len(buf) if n is None else int(n.item())
    cap = len(buf) // 16 + 64
    mk = lambda g: B.FrameScanner(cap, gpu, window=W, group=g,    # noqa: E731
                                  max_packet=MAXP)
    one, grp, dfr = mk(1), mk(G), mk(G)
    assert grp.group == G
    res1, off1, len1 = _rows(one.scan(d, ln, **kw))
    resg, offg, leng = _rows(grp.scan(d, ln, **kw))
    assert resg == res1, (resg, res1)
    assert np.array_equal(offg, off1) and np.array_equal(leng, len1)
    hoff, hlen, stop, bad = _host(buf[:nb].tobytes())
    assert resg == [len(hoff), stop, int(bad), 0], (resg, len(hoff), stop, bad)
    assert np.array_equal(offg, hoff) and np.array_equal(leng, hlen)
    # the carried partial tail: the bytes from the stop offset on
    assert bytes(buf[resg[1]:nb]) == bytes(buf[stop:nb])
    # the rows pass deferred to the decode
    ft = dfr.scan(d, ln, rows=False, **kw)
    if dfr.pending is not None:
        B.decode_replies(d, ft, xt, tiles=dfr.pending)
        resd, offd, lend = _rows(ft)
        assert resd == res1
        assert np.array_equal(offd, off1) and np.array_equal(lend, len1)
    return resg


# ---- equal frames ----------------------------------------------------------

@pytest.mark.parametrize('W', WINDOWS)
@pytest.mark.parametrize('G', GROUPS)
@pytest.mark.parametrize('S', SIZES)
def test_equal_frames(gpu, xt, S, G, W):
    """(W = 256: the gather, every group; W = 512: the carried walk.)  Two
    whole groups, then a last group the stream ends in — in each of
    its tiles, at a frame's end and inside a trailing frame."""
    rng = np.random.default_rng(S * 100 + G)
    buf, starts = _equal(rng, S, (3 * G + 1) * TILE)
    for j in range(G):
        end = (2 * G + j) * TILE + 1000
        k = int(np.searchsorted(starts, end))           # frames kept whole
        whole = int(starts[k])
        for cut in (whole, whole + 2, whole + S // 2):
            res = _check(gpu, xt, buf[:cut], G, W)
            assert res == [k, whole, 0, 0]


@pytest.mark.parametrize('G', GROUPS)
@pytest.mark.parametrize('S', [1000, 2048, 4096])
def test_frames_up_to_a_tile(gpu, xt, S, G):
    """Runs of frames far larger than the 256-byte window, up to one frame a
    tile (S = 4096: every exit a whole tile on): the sizes the gather admits
    beyond the replies' (16 <= S <= 4096).  The stream ends in the last
    group's middle tile, after a whole frame and inside one."""
    rng = np.random.default_rng(S + G)
    buf, starts = _equal(rng, S, (3 * G + 1) * TILE)
    end = (2 * G + G // 2) * TILE + 1000
    k = int(np.searchsorted(starts, end))
    whole = int(starts[k])
    for cut in (whole, whole + S // 2, len(buf)):
        res = _check(gpu, xt, buf[:cut], G, 256)
        if cut == len(buf):
            assert res == [len(starts), len(buf), 0, 0]
        else:
            assert res == [k, whole, 0, 0]


# ---- a run broken at frame j -----------------------------------------------

def _break_positions(starts, G):
    """Frame indices in the stream's second group: the first frame a gather
    reads (the first starting in the group's second tile), the frames at
    lanes 63 and 64 of it, a frame across a tile boundary, the group's last
    frame and the next group's first."""
    g0 = G * TILE
    first = int(np.searchsorted(starts, g0 + TILE))
    strad = int(np.searchsorted(starts, g0 + min(3, G) * TILE)) - 1
    last = int(np.searchsorted(starts, 2 * G * TILE)) - 1
    pos = {'first': first, 'lane63': first + 63, 'lane64': first + 64,
           'straddle': strad, 'last': last, 'next': last + 1}
    return {k: v for k, v in pos.items() if v <= last + 1}


@pytest.mark.parametrize('W', WINDOWS)
@pytest.mark.parametrize('G', GROUPS)
@pytest.mark.parametrize('S', [45, 192])
def test_run_broken(gpu, xt, S, G, W):
    """(W = 256: the gather meets the break; W = 512: the carried walk.)"""
    rng = np.random.default_rng(S + G)
    n = (3 * G + 1) * TILE // S
    base, starts = _build(rng, np.full(n, S))
    for name, j in _break_positions(starts, G).items():
        at = int(starts[j])
        # another legal size: the chain goes on from the shifted start
        sizes = np.full(n, S)
        sizes[j] = S + 37
        buf, st2 = _build(rng, sizes)
        res = _check(gpu, xt, buf, G, W)
        assert res == [n, len(buf), 0, 0], name
        # a negative length, and one over max_packet: BAD_LENGTH at frame j
        for v in (-16, MAXP + 1):
            buf = base.copy()
            _put(buf, at, v)
            res = _check(gpu, xt, buf, G, W)
            assert res == [j, at, 1, 0], (name, v)
        # a legal length that overruns the stream: a partial frame, carried
        buf = base.copy()
        _put(buf, at, MAXP - 1)
        cut = min(len(buf), at + 2000)
        res = _check(gpu, xt, buf[:cut], G, W)
        assert res == [j, at, 0, 0], name


# ---- runs that begin late, payloads that imitate the run -------------------

@pytest.mark.parametrize('W', WINDOWS)
@pytest.mark.parametrize('G', GROUPS)
def test_run_begins_in_the_third_tile(gpu, xt, G, W):
    """Every group opens with varied frames and turns into a run of 192-byte
    frames only in its third tile (in its second for G = 2).  No gather
    here (it is taken at a group's first tile only): the walk's run steps
    with the size carried across tiles."""
    rng = np.random.default_rng(G)
    sizes, pos = [], 0
    for g in range(4):
        turn = g * G * TILE + min(2, G - 1) * TILE + 300
        while pos < turn:
            s = int(rng.integers(24, 250))
            sizes.append(s)
            pos += s
        while pos < (g + 1) * G * TILE:
            sizes.append(192)
            pos += 192
    buf, starts = _build(rng, sizes)
    res = _check(gpu, xt, buf, G, W)
    assert res == [len(sizes), len(buf), 0, 0]


@pytest.mark.parametrize('W', WINDOWS)
@pytest.mark.parametrize('G', GROUPS)
@pytest.mark.parametrize('S', [88, 192])
def test_payload_repeats_the_length_word(gpu, xt, S, G, W):
    """Every body is be32(S - 4) over and over: each aligned word of the
    stream starts a chain of S-byte frames.  Only the chain from the entry
    counts — and a frame of another size in every group moves it."""
    rng = np.random.default_rng(S)
    n = (3 * G + 1) * TILE // S
    sizes = np.full(n, S)
    per = G * TILE // S
    sizes[per // 2::per] = S + 6                   # moves the chain by 2 mod 4
    fill = list(int(S - 4).to_bytes(4, 'big'))
    buf, starts = _build(rng, sizes, fill=fill)
    res = _check(gpu, xt, buf, G, W)
    assert res == [n, len(buf), 0, 0]


# ---- the link repair, short and empty streams ------------------------------

@pytest.mark.parametrize('kw', [{'misspec': 2}, {'misspec': 3},
                                {'nospec': True}],
                         ids=['misspec2', 'misspec3', 'nospec'])
@pytest.mark.parametrize('G', GROUPS)
def test_misspeculated_entries(gpu, xt, G, kw):
    """The scanner's test flags on a grouped scan (a garbage entry into
    every P-th group's first tile, or no speculated entry at all): fs_link
    repairs the links over the gathered tiles' records (their entries,
    exits, candidate words and exit maps), and ends with the rows of the
    one-tile-a-wave scan.  A group's entry one byte off cannot be the exit
    of the group before, so the link pass must have had work: its counters
    say so."""
    rng = np.random.default_rng(7)
    buf, starts = _equal(rng, 192, (6 * G + 1) * TILE)
    res = _check(gpu, xt, buf, G, 256, **kw)
    assert res == [len(starts), len(buf), 0, 0]
    d = torch.from_numpy(buf).to(gpu)
    sc = B.FrameScanner(len(buf) // 16 + 64, gpu, window=256, group=G,
                        max_packet=MAXP)
    sc.scan(d, len(buf), **kw)
    st = sc.chain_stats()
    print(G, kw, st)
    if kw.get('nospec'):
        assert st['no_spec'] >= 6          # every group but the first
    else:
        assert st['rewalked'] + st['looked_up'] + st['rounds'] > 0


@pytest.mark.parametrize('G', GROUPS)
def test_short_and_empty_streams(gpu, xt, G):
    rng = np.random.default_rng(9)
    buf, starts = _equal(rng, 192, G * TILE)
    # shorter than one group (G > 2: more than one tile of it; else one tile)
    cut = max(G // 2, 1) * TILE + 500
    k = int(np.searchsorted(starts, cut, side='right')) - 1
    res = _check(gpu, xt, buf[:cut], G, 256)
    assert res == [k, int(starts[k]), 0, 0]
    # two frames: one tile
    res = _check(gpu, xt, buf[:384], G, 256)
    assert res == [2, 384, 0, 0]
    # empty: a device length of zero over the whole buffer
    n0 = torch.zeros(1, dtype=torch.int64, device=gpu)
    res = _check(gpu, xt, buf, G, 256, n=n0)
    assert res == [0, 0, 0, 0]
