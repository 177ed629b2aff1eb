"""The front end's staging kernels (csrc/kernels/front.hip): front_cut,
front_gather and front_tx_pieces against the Python mirror of zk_front.h
(tests/frontmodel.py) and numpy copies.  All comparisons are exact; the shapes
are the smallest at which the kernels can still go wrong."""

import struct

import numpy as np
import pytest
import torch

import frontmodel as M
from treemodel import _stream, create, dev_bytes, get, set_data
from watchmodel import wexists, wget

from zkmi.ops import _lib

pytestmark = pytest.mark.gpu

I64, I32, U8 = torch.int64, torch.int32, torch.uint8
D0 = '/bench/d000000'
BIG = 1 << 20


def dev_cut(dev, raw, starts, quota, max_packet=M.MAX_PACKET, shift=0):
    """front_cut of ``raw`` on the device -> (fault, [(take, nfr, flag)]).
    ``shift``: the stream begins that many bytes into its allocation."""
    S = len(starts) - 1
    buf = dev_bytes(b'\xee' * shift + raw + b'\xee' * 64, dev)
    take = torch.full((S,), -7, dtype=I64, device=dev)
    nfr = torch.full((S,), -7, dtype=I32, device=dev)
    flag = torch.full((S,), -7, dtype=I32, device=dev)
    fault = torch.full((1,), -7, dtype=I64, device=dev)
    _lib.front_cut(buf[shift:], len(raw),
                   torch.tensor(starts, dtype=I64, device=dev), quota,
                   max_packet, take, nfr, flag, fault)
    return int(fault.item()), list(zip(take.cpu().tolist(),
                                       nfr.cpu().tolist(),
                                       flag.cpu().tolist()))


def table(segs):
    starts = [0]
    for b in segs:
        starts.append(starts[-1] + len(b))
    return b''.join(segs), starts


def check_cut(dev, segs, quota, shift=0):
    raw, starts = table(segs)
    got = dev_cut(dev, raw, starts, quota, shift=shift)
    want = M.cut(raw, starts, quota)
    assert got[0] == want[0] == 0
    bad = [(s, g, w) for s, (g, w) in enumerate(zip(got[1], want[1]))
           if g != w]
    assert not bad, bad[:5]
    return got[1]


def rand_segment(rng, ops):
    b = b''
    for _ in range(int(rng.randint(0, 7))):
        body = bytes(rng.randint(0, 256, size=int(rng.randint(0, 40)),
                                 dtype=np.uint8))
        b += M.frame(int(rng.choice(ops)), body)
    r = rng.randint(0, 8)
    if r == 0:
        b += M.raw_frame(int(rng.choice([-1, M.INT32_MIN,
                                         M.MAX_PACKET + 1])))
    elif r == 1 and b:
        b = b[:len(b) - int(rng.randint(1, min(len(b), 9) + 1))]
    elif r == 2:
        b = b''
    return b


# ---- the cut -----------------------------------------------------------------

@pytest.mark.parametrize('S', [1, 3, 65, 257])
def test_cut_segment_counts(gpu, S):
    rng = np.random.RandomState(S)
    ops = list(M.OPS.values()) + [7, 13, 14]
    segs = [rand_segment(rng, ops) for _ in range(S)]
    if S == 1:
        segs = [M.frame(4, b'x' * 9) * 3 + M.frame(5, b'y' * 20)]
    if S == 3:
        segs[1] = b''
        segs[0] = segs[0] or M.frame(4, b'x' * 9)
        segs[2] = segs[2] or M.frame(4, b'x' * 9)
    g = M.frame(4, b'x' * 9)
    if S >= 65:
        segs[5] = M.raw_frame(-1)
        segs[6] = g + M.raw_frame(M.INT32_MIN) + g
        segs[S - 1] = g + g[:-1]
    cuts = check_cut(gpu, segs, 64)
    check_cut(gpu, segs, 2, shift=5)
    if S == 3:
        assert cuts[1] == (0, 0, 0)
    if S >= 65:
        assert cuts[5] == (0, 0, 1) and cuts[6] == (len(g), 1, 1)
        assert cuts[S - 1] == (len(g), 1, 0)


def test_cut_words_straddle_the_chunk(gpu):
    """A length word, an opcode word and a body's end at -3 .. +3 bytes from
    the end of the staged window (which begins at the 16-byte boundary of the
    stream at or before the segment's first byte), and the same distances
    from a chunk further on, for segments that begin at any residue."""
    CH = _lib.front_chunk()
    assert CH % 16 == 0 and CH >= 256
    rng = np.random.RandomState(2)
    noise = lambda k: bytes(rng.randint(1, 256, size=k, dtype=np.uint8))
    for pre in (b'', M.frame(4, b'p')):            # 0 and 13 bytes before it
        segs = [pre]
        pos = len(pre)

        def add(make):
            nonlocal pos
            for d in range(-3, 4):
                for w in (1, 2):
                    # `at` bytes into the segment is d bytes past the window
                    segs.append(make(w * CH + d - (pos & 15)))
                    pos += len(segs[-1])

        # the second frame's length word begins there: 300 bytes of body that
        # are there, then a frame that is not whole
        add(lambda at: M.frame(4, noise(at - 12)) + M.frame(3, noise(292)) +
            M.frame(4, noise(30))[:-1])
        # the second frame's opcode word begins there: a write, or a read
        # whose neighbouring words spell one
        add(lambda at: M.frame(4, noise(at - 20)) + M.frame(5, noise(17)) +
            M.frame(4, b'z'))
        add(lambda at: M.frame(4, noise(at - 20)) +
            M.frame(4, noise(17), xid=5) + M.frame(4, struct.pack('>i', 5)))
        # a body that ends there, and one that is a byte short of it
        add(lambda at: M.frame(8, noise(at - 12)) + M.frame(4, b'c' * 9))
        add(lambda at: M.frame(8, noise(at - 12))[:-1])
        cuts = check_cut(gpu, segs, 64)
        assert [c[1] for c in cuts[1:]] == [2] * 14 + [1] * 14 + [3] * 14 + \
            [2] * 14 + [0] * 14


def test_cut_long_segment_beside_short_ones(gpu):
    """One segment of 200 KiB of 20-byte frames (the window moves 50 times)
    beside 64 segments of one frame."""
    f = M.frame(4, b'12345678')
    assert len(f) == 20
    n = 200 * 1024 // 20
    long = f * n + f[:7]
    one = [M.frame(3, b'abc' * k) for k in range(64)]
    cuts = check_cut(gpu, one[:32] + [long] + one[32:], BIG, shift=9)
    assert cuts[32] == (20 * n, n, 0)
    cuts = check_cut(gpu, one[:32] + [long] + one[32:], 1000)
    assert cuts[32] == (20 * 1000, 1000, 0)
    # a write deep inside it stops the walk there
    k = 7000
    cuts = check_cut(gpu, [f * k + M.frame(2, b'd' * 8) + f * 100], BIG)
    assert cuts[0] == (20 * k, k, 0)


def test_cut_walk_cases(gpu):
    """The host test's walk cases, as one table a quota."""
    cases = M.walk_cases()
    for quota in sorted({q for _, _, q, _ in cases}):
        cuts = check_cut(gpu, [seg for _, seg, _, _ in cases], quota)
        for (name, _, q, want), c in zip(cases, cuts):
            if q == quota and want is not None:
                assert c == want, name


def test_cut_table_faults(gpu):
    g = M.frame(4, b'\x00' * 9)
    raw = g * 4
    L, n = len(g), 4 * len(g)
    for starts, fault in (([0, L, 2 * L, n], 0), ([1, L, 2 * L, n], 1),
                          ([0, 2 * L, L, n], 1), ([0, L, 2 * L, n + 1], 1),
                          ([-1, L, 2 * L, n], 1), ([0, L, n, 2 * L], 1),
                          ([0, n + 9, n + 9, n + 9], 1)):
        got = dev_cut(gpu, raw, starts, 8)
        assert got == M.cut(raw, starts, 8), starts
        assert got[0] == fault
        if fault:
            assert got[1] == [(0, 0, 0)] * 3


def test_cut_max_packet(gpu):
    body = b'\x00' * 40
    seg = M.raw_frame(40, body) + M.raw_frame(41, body + b'\x00')
    for mp, want in ((40, (44, 1, 1)), (41, (89, 2, 0)), (39, (0, 0, 1))):
        assert dev_cut(gpu, seg, [0, len(seg)], 8, mp)[1] == [want]


# ---- the gather --------------------------------------------------------------

def _scan(x):
    n = int(x.numel())
    off = torch.zeros(n + 1, dtype=I64, device=x.device)
    ws = torch.empty(_lib.lib().scan_workspace(n), dtype=I64, device=x.device)
    _lib.lib().scan_excl(x, off, off[n:], ws)
    return off


def dev_gather(dev, streams, pieces, slack=0, dshift=0, with_table=True):
    """pieces: [(stream, src, len)] -> (dst bytes, over, untouched?)."""
    st = torch.tensor([p[0] for p in pieces], dtype=I32, device=dev)
    src = torch.tensor([p[1] for p in pieces], dtype=I64, device=dev)
    ln = torch.tensor([p[2] for p in pieces], dtype=I64, device=dev)
    off = _scan(ln)
    total = sum(p[2] for p in pieces)
    assert int(off[-1].item()) == total
    room = total + slack
    buf = torch.full((dshift + max(room, 0) + 64,), 0xAB, dtype=U8,
                     device=dev)
    over = torch.full((1,), -7, dtype=I64, device=dev)
    _lib.front_gather([dev_bytes(s, dev) if s else
                       torch.empty(0, dtype=U8, device=dev) for s in streams],
                      st if with_table else None, src, off, len(pieces),
                      buf[dshift:dshift + room], over)
    out = bytes(buf.cpu().numpy().tobytes())
    return out, int(over.item()), dshift, room


def check_gather(dev, streams, pieces, dshift=0, with_table=True):
    out, over, a, room = dev_gather(dev, streams, pieces, dshift=dshift,
                                    with_table=with_table)
    want = b''.join(streams[s][o:o + n] for s, o, n in pieces)
    assert over == 0
    assert out[:a] == b'\xab' * a and out[a + room:] == b'\xab' * 64
    got = out[a:a + room]
    if got != want:
        k = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError('first difference at byte %d of %d' %
                             (k, len(want)))


def _streams(rng, sizes):
    return [bytes(rng.randint(0, 256, size=n, dtype=np.uint8))
            for n in sizes]


def test_gather_lengths_and_residues(gpu):
    rng = np.random.RandomState(4)
    streams = _streams(rng, (90000, 9000, 9000, 9000))
    pieces = []
    for L in (0, 1, 15, 16, 17, 255, 4096, 70000):
        for rs in (0, 1, 15):
            pieces.append((0, rs + 16 * int(rng.randint(0, 100)), L))
            pieces.append((0, 3, int(rng.randint(0, 16))))
    # every (source residue, destination residue) pair, with an interior
    at = sum(p[2] for p in pieces)
    seen = set()
    for rs in range(16):
        for rd in range(16):
            fill = (rd - at) % 16
            pieces.append((1 + rs % 3, int(rng.randint(0, 50)), fill))
            at += fill
            L = 48 + int(rng.randint(0, 40))
            pieces.append((1 + rd % 3, rs + 16 * int(rng.randint(0, 400)),
                           L))
            seen.add((rs, at % 16))
            at += L
    assert len(seen) == 256
    check_gather(gpu, streams, pieces)
    check_gather(gpu, streams, pieces, dshift=7)
    # pieces of stream 0 alone need no table
    only0 = [p for p in pieces if p[0] == 0]
    check_gather(gpu, streams[:1], only0, with_table=False, dshift=12)


@pytest.mark.parametrize('P', [1, 1025])
def test_gather_piece_counts(gpu, P):
    rng = np.random.RandomState(P)
    streams = _streams(rng, (5000, 5000, 0, 5000))
    pieces = []
    for _ in range(P):
        s = int(rng.choice([0, 1, 3]))
        L = int(rng.choice([0, 0, 1, 3, 16, 20, 37, 64, 200]))
        pieces.append((s, int(rng.randint(0, 5000 - L + 1)), L))
    if P == 1:
        pieces = [(1, 5, 333)]
    check_gather(gpu, streams, pieces)
    if P == 1:
        check_gather(gpu, streams, [(0, 0, 0)])


def test_gather_overflow_writes_nothing(gpu):
    rng = np.random.RandomState(6)
    streams = _streams(rng, (3000,))
    pieces = [(0, 5, 1000), (0, 1, 17), (0, 100, 600)]
    out, over, a, room = dev_gather(gpu, streams, pieces, slack=-1)
    assert over == 1 and room == 1616
    assert out == b'\xab' * len(out)               # the canary behind it too
    out, over, a, room = dev_gather(gpu, streams, pieces, slack=0)
    assert over == 0 and out[room:] == b'\xab' * 64
    assert out[:room] == b''.join(streams[0][o:o + n] for _, o, n in pieces)


def test_gather_skips_a_piece_outside_its_stream(gpu):
    rng = np.random.RandomState(8)
    streams = _streams(rng, (400, 100))
    pieces = [(0, 0, 100), (1, 50, 51), (0, 390, 10), (2, 0, 8), (1, -1, 4),
              (0, 200, 40)]
    out, over, a, room = dev_gather(gpu, streams, pieces)
    assert over == 0
    s0 = streams[0]
    want = s0[0:100] + b'\xab' * 51 + s0[390:400] + b'\xab' * 12 + s0[200:240]
    assert out[:room] == want and out[room:] == b'\xab' * 64


# ---- the assembly --------------------------------------------------------------

def _batch(dev, segs):
    from zkmi.server.engine import SessionSegments
    parts = []
    for _, _, pk in segs:
        for k, p in enumerate(pk):
            p['xid'] = 1 + k
        parts.append(_stream(pk))
    rx = b''.join(parts)
    cuts = [0] + [int(x) for x in np.cumsum([len(b) for b in parts])]
    tab = SessionSegments(
        torch.tensor(cuts, dtype=I64, device=dev),
        torch.tensor([s for s, _, _ in segs], dtype=I64, device=dev),
        torch.tensor([w for _, w, _ in segs], dtype=I32, device=dev))
    return dev_bytes(rx, dev), len(rx), tab


def _host(t, n=None):
    b = bytes(t.cpu().numpy().tobytes())
    return b if n is None else b[:n]


def test_tx_assembly_of_a_real_batch(gpu):
    """One serve_sessions_mixed(resume=True, close=True) batch of five
    connections — two that share nothing, one that watches, one that resumes,
    one that closes: every connection's TX span is its replies, then its
    watcher slot's catch-up, write-fired and close-fired slices, taken on the
    host from out / rep_off and the three slot_off tables."""
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(10, 16, fanout=10, device=gpu, spare=0.0, watch_cap=1024,
                   scratch=1 << 16)
    srv = GpuServer(tree, 256, 1 << 18)
    sid = [(1 << 56) | (0x100 + k) for k in range(5)]
    keep, other = D0 + '/n000000004', D0 + '/n000000005'
    mine = D0 + '/mine'
    L = _lib.lib()

    def serve(segs, **kw):
        rx, n, sg = _batch(gpu, segs)
        out, total, err, _ = srv.serve_sessions_mixed(rx, n, sg, **kw)
        assert int(err.item()) == 0
        return out, total, err, sg

    serve([(sid[4], 40, [create(mine, b'm', ['EPHEMERAL'])])])
    rel = int(tree.counters[_lib.TC_ZXID].item())
    serve([(sid[2], 7, [wget(keep), wexists(mine)]),
           (sid[0], -1, [set_data(other, b'later')])])
    out, total, err, sg = serve([
        (sid[0], -1, [get(keep), get(other)]),
        (sid[1], 3, [set_data(keep, b'fire'), get(D0 + '/n000000001')]),
        (sid[2], 7, [get(other)]),
        (sid[3], 12, [{'opcode': 'SET_WATCHES', 'relZxid': rel,
                       'events': {'dataChanged': [other, keep],
                                  'createdOrDestroyed': [],
                                  'childrenChanged': []}}]),
        (sid[4], 40, [{'opcode': 'CLOSE_SESSION'}])],
        resume=True, close=True)
    S = 5
    streams = [out, srv.resume_notif[0], srv.notif[0], srv.close_notif[0]]
    offs = [srv.resume_slots[1], srv.notif_slots[1], srv.close_slots[1]]
    caps = [int(s.numel()) for s in streams]
    owner = torch.zeros(64, dtype=I64, device=gpu)
    p_stream = torch.zeros(4 * S, dtype=I32, device=gpu)
    p_src = torch.zeros(4 * S, dtype=I64, device=gpu)
    p_len = torch.zeros(4 * S, dtype=I64, device=gpu)
    stats = torch.zeros(8, dtype=I64, device=gpu)
    _lib.front_tx_pieces(srv.seg.rep_off, sg.wslots, offs[0], offs[1],
                         offs[2], err, caps, owner, p_stream, p_src, p_len,
                         stats)
    p_off = _scan(p_len)
    tx = torch.full((1 << 16,), 0xAB, dtype=U8, device=gpu)
    over = torch.zeros(1, dtype=I64, device=gpu)
    _lib.front_gather(streams, p_stream, p_src, p_off, 4 * S, tx, over)
    # the host's own slicing
    rep = srv.seg.rep_off.cpu().tolist()
    so = [o.cpu().tolist() for o in offs]
    hs = [_host(s) for s in streams]
    ws = sg.wslots.cpu().tolist()
    want = []
    for s in range(S):
        b = [hs[0][rep[s]:rep[s + 1]]]
        for k in range(3):
            w = ws[s]
            b.append(hs[1 + k][so[k][w]:so[k][w + 1]] if 0 <= w < 64
                     else b'')
        want.append(b)
    off = p_off.cpu().tolist()
    got = _host(tx)
    assert int(over.item()) == 0 and int(stats[0].item()) == 0
    assert M.pieces(ws, rep, so, 0, caps)[1] == list(zip(
        p_stream.cpu().tolist(), p_src.cpu().tolist(), p_len.cpu().tolist()))
    for s in range(S):
        assert got[off[4 * s]:off[4 * s + 4]] == b''.join(want[s]), s
    assert got[off[-1]:] == b'\xab' * (len(got) - off[-1])
    # the batch was what the test says it was
    lens = [[len(x) for x in b] for b in want]
    assert all(l[0] > 0 for l in lens)
    assert lens[0][1:] == [0, 0, 0] and lens[1][1:] == [0, 0, 0]
    assert lens[2][1] == 0 and lens[2][2] > 0 and lens[2][3] > 0
    assert lens[3][1] > 0 and lens[3][2:] == [0, 0]
    assert lens[4][1:] == [0, 0, 0] and lens[4][0] == 20
    # err != 0: every piece is empty
    bad = torch.full((1,), 2, dtype=I32, device=gpu)
    _lib.front_tx_pieces(srv.seg.rep_off, sg.wslots, offs[0], offs[1],
                         offs[2], bad, caps, owner, p_stream, p_src, p_len,
                         stats)
    assert p_len.cpu().tolist() == [0] * 20


def test_tx_pieces_tables(gpu):
    """Slots -1, 0, 63 and 64, two segments on one slot across more than one
    block of the owner pass, absent streams."""
    rng = np.random.RandomState(9)
    S = 600
    ws = [int(x) for x in rng.randint(-2, 66, size=S)]
    ws[:4] = [-1, 0, 63, 64]
    ws[300], ws[599] = 17, 17
    caps = (5000, 4000, 3000, 2000)
    rep = sorted(int(x) for x in rng.randint(0, caps[0] + 1, size=S + 1))
    so = [[0] + sorted(int(x) for x in rng.randint(0, caps[k + 1] + 1,
                                                   size=64))
          for k in range(3)]
    T = lambda v, dt=I64: torch.tensor(v, dtype=dt, device=gpu)
    for have in ((1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 0), (1, 1, 0, 1),
                 (0, 0, 0, 1)):
        owner = torch.zeros(64, dtype=I64, device=gpu)
        p_stream = torch.zeros(4 * S, dtype=I32, device=gpu)
        p_src = torch.zeros(4 * S, dtype=I64, device=gpu)
        p_len = torch.zeros(4 * S, dtype=I64, device=gpu)
        stats = torch.zeros(8, dtype=I64, device=gpu)
        offs = [T(so[k]) if have[k + 1] else None for k in range(3)]
        _lib.front_tx_pieces(T(rep) if have[0] else None, T(ws, I32),
                             offs[0], offs[1], offs[2], None, caps, owner,
                             p_stream, p_src, p_len, stats)
        dup, want = M.pieces(ws, rep if have[0] else None,
                             [so[k] if have[k + 1] else None
                              for k in range(3)], None, caps)
        assert int(stats[0].item()) == dup and dup > 400
        assert owner.cpu().tolist() == M.owners(ws)[0]
        assert list(zip(p_stream.cpu().tolist(), p_src.cpu().tolist(),
                        p_len.cpu().tolist())) == want
