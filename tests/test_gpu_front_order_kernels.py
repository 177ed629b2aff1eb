"""The ordered front end's kernels alone: the cut's ordered instance
(csrc/kernels/front.hip front_cut_k<true>), the deferral stage of the ordered
session serve (csrc/kernels/tree_order.hip ord_clip_first_k / ord_clip_mark_k
/ ord_clip_ranges_k) and the reply ends of front_tx_pieces, against the
Python mirror (tests/ordermodel.py, tests/frontmodel.py) and numpy.  All
comparisons are exact; the shapes are the smallest at which the kernels can
still go wrong."""

import numpy as np
import pytest
import torch

import frontmodel as F
import ordermodel as M
from treemodel import dev_bytes

from zkmi.ops import _lib

pytestmark = pytest.mark.gpu

I64, I32, U8 = torch.int64, torch.int32, torch.uint8


def table(segs):
    starts = [0]
    for b in segs:
        starts.append(starts[-1] + len(b))
    return b''.join(segs), starts


def dev_cut(dev, raw, starts, quota, mode, has_acl=True, shift=0):
    """front_cut -> (fault, [(take, nfr, flag, nwr)]); nwr is the canary -7
    where the kernel left it alone."""
    S = len(starts) - 1
    buf = dev_bytes(b'\xee' * shift + raw + b'\xee' * 64, dev)
    take = torch.full((S,), -7, dtype=I64, device=dev)
    nfr = torch.full((S,), -7, dtype=I32, device=dev)
    flag = torch.full((S,), -7, dtype=I32, device=dev)
    nwr = torch.full((S,), -7, dtype=I32, device=dev)
    fault = torch.full((1,), -7, dtype=I64, device=dev)
    _lib.front_cut(buf[shift:], len(raw),
                   torch.tensor(starts, dtype=I64, device=dev), quota,
                   F.MAX_PACKET, take, nfr, flag, fault, mode=mode,
                   has_acl=has_acl, nwr=nwr)
    return int(fault.item()), list(zip(take.cpu().tolist(),
                                       nfr.cpu().tolist(),
                                       flag.cpu().tolist(),
                                       nwr.cpu().tolist()))


def check_cut(dev, segs, quota, has_acl=True, shift=0):
    raw, starts = table(segs)
    got = dev_cut(dev, raw, starts, quota, 1, has_acl, shift)
    want = M.cut_ordered(raw, starts, quota, has_acl)
    assert got[0] == want[0] == 0
    bad = [(s, g, w) for s, (g, w) in enumerate(zip(got[1], want[1]))
           if g != w]
    assert not bad, bad[:5]
    return got[1]


def rand_segment(rng, ops):
    b = b''
    for _ in range(int(rng.randint(0, 9))):
        body = bytes(rng.randint(0, 256, size=int(rng.randint(0, 40)),
                                 dtype=np.uint8))
        b += F.frame(int(rng.choice(ops)), body)
    r = rng.randint(0, 8)
    if r == 0:
        b += F.raw_frame(int(rng.choice([-1, F.INT32_MIN,
                                         F.MAX_PACKET + 1])))
    elif r == 1 and b:
        b = b[:len(b) - int(rng.randint(1, min(len(b), 9) + 1))]
    return b


# ---- the ordered cut -----------------------------------------------------------

@pytest.mark.parametrize('S', [1, 3, 65])
def test_ordered_cut_segment_counts(gpu, S):
    rng = np.random.RandomState(100 + S)
    ops = list(F.OPS.values()) + [7, 13, 14] + [1, 2, 5, 4, 3] * 3
    segs = [rand_segment(rng, ops) for _ in range(S)]
    w = F.frame(5, b'y' * 20)
    ls = F.frame(8, b'l' * 9)
    if S == 1:
        segs = [w * 3 + F.frame(4, b'x' * 9) + ls + w]
    if S == 3:
        segs[0] = w + w
        segs[1] = b''                                # 0 bytes
        segs[2] = ls + w
    if S == 65:
        segs[4] = b''
        # one longer than the staged window, its stop behind the window's end
        segs[7] = w * 200 + ls + w
        segs[64] = w + F.frame(-11) + w
    for acl in (True, False):
        cuts = check_cut(gpu, segs, 1 << 20, acl)
        check_cut(gpu, segs, 2, acl, shift=5)
    if S == 1:
        assert cuts[0] == (len(segs[0]) - len(w), 5, 0, 3)
    if S == 3:
        assert cuts == [(2 * len(w), 2, 0, 2), (0, 0, 0, 0),
                        (len(ls), 1, 0, 0)]
    if S == 65:
        assert len(segs[7]) > _lib.front_chunk()
        assert cuts[7] == (200 * len(w) + len(ls), 201, 0, 200)
        assert cuts[64] == (len(w) + 12, 2, 0, 2)


def test_ordered_cut_walk_cases(gpu):
    """The host test's cases: each as the only segment of a stream (the
    straddling words sit where the case puts them: the window begins at the
    segment's first byte) and all as one table, for either ACL setting."""
    cases = M.walk_cases()
    for name, seg, q, acl, want in cases:
        if len(seg) > 1024:
            got = dev_cut(gpu, seg, [0, len(seg)], q, 1, acl)
            assert got == (0, [want]), name
    for quota in sorted({q for _, _, q, _, _ in cases}):
        for acl in (True, False):
            cuts = check_cut(gpu, [seg for _, seg, _, _, _ in cases], quota,
                             acl)
            for (name, _, q, a, want), c in zip(cases, cuts):
                if q == quota and a == acl and want is not None:
                    assert c == want, name


def test_mode_0_is_the_plain_cut(gpu):
    """mode=0 with the keywords and the call without them: the same take /
    nfr / flag / fault, and nwr is left alone."""
    rng = np.random.RandomState(7)
    ops = list(F.OPS.values()) + [7, 13, 14]
    segs = [rand_segment(rng, ops) for _ in range(65)]
    raw, starts = table(segs)
    S = len(segs)
    buf = dev_bytes(raw + b'\xee' * 64, gpu)
    st = torch.tensor(starts, dtype=I64, device=gpu)
    outs = []
    for kw in (False, True):
        take = torch.full((S,), -7, dtype=I64, device=gpu)
        nfr = torch.full((S,), -7, dtype=I32, device=gpu)
        flag = torch.full((S,), -7, dtype=I32, device=gpu)
        fault = torch.full((1,), -7, dtype=I64, device=gpu)
        nwr = torch.full((S,), -7, dtype=I32, device=gpu)
        if kw:
            _lib.front_cut(buf, len(raw), st, 64, F.MAX_PACKET, take, nfr,
                           flag, fault, mode=0, has_acl=True, nwr=nwr)
        else:
            _lib.front_cut(buf, len(raw), st, 64, F.MAX_PACKET, take, nfr,
                           flag, fault)
        assert nwr.cpu().tolist() == [-7] * S
        outs.append((take.cpu().tolist(), nfr.cpu().tolist(),
                     flag.cpu().tolist(), fault.cpu().tolist()))
    assert outs[0] == outs[1]
    fault, cuts = F.cut(raw, starts, 64)
    assert outs[0] == ([c[0] for c in cuts], [c[1] for c in cuts],
                       [c[2] for c in cuts], [fault])


# ---- the clip ----------------------------------------------------------------

def dev_clip(dev, rank, cls, sub, f_seg, S, passes, nfr=None):
    """order_clip -> (clipf, f_seg after, [seg_c after] * 3, deferred).  The
    class tables start as the split would leave them."""
    ncap = len(cls)
    nfr = ncap if nfr is None else nfr
    seg_c = [[-9] * ncap for _ in range(3)]
    for i in range(nfr):
        if 0 <= cls[i] < 3 and 0 <= sub[i] < ncap:
            seg_c[cls[i]][sub[i]] = f_seg[i]
    d = lambda v, t: torch.tensor(v, dtype=t, device=dev)
    d_seg = d(f_seg, I32)
    d_c = [d(c, I32) for c in seg_c]
    clipf = torch.full((S,), -7, dtype=I64, device=dev)
    cnt = torch.full((1,), -7, dtype=I64, device=dev)
    _lib.order_clip(d(rank, U8), passes, ncap,
                    [d(cls, I32), d(sub, I32), d([nfr], I64), d_seg, *d_c,
                     clipf, cnt])
    return (clipf.cpu().tolist(), d_seg.cpu().tolist(),
            [c.cpu().tolist() for c in d_c], int(cnt.item()), seg_c)


def check_clip(dev, rank, cls, sub, f_seg, S, passes, nfr=None):
    ncap = len(cls)
    n = ncap if nfr is None else nfr
    clipf, seg_after, c_after, cnt, c_before = dev_clip(
        dev, rank, cls, sub, f_seg, S, passes, nfr)
    want_clipf, want_df = M.clip(rank, cls, sub, f_seg, S, passes, nfr)
    assert clipf == want_clipf
    assert cnt == sum(want_df)
    want_seg = [(-1 if i < n and want_df[i] else f_seg[i])
                for i in range(ncap)]
    assert seg_after == want_seg
    want_c = [list(c) for c in c_before]
    for i in range(n):
        if want_df[i] and 0 <= cls[i] < 3 and 0 <= sub[i] < ncap:
            want_c[cls[i]][sub[i]] = -1
    assert c_after == want_c
    return clipf, want_df


def _subs(classes):
    n = [0, 0, 0]
    sub = []
    for c in classes:
        sub.append(n[c])
        n[c] += 1
    return sub


def test_clip_hand_made_tables(gpu):
    P = 4
    # a segment spanning two waves (frames 40..99 of 150: ncap no multiple
    # of 64), its first overflow in the second wave; two segments in one wave
    # (0: frames 0..19, 1: 20..39) each with overflows of their own
    ncap = 150
    f_seg = [0] * 20 + [1] * 20 + [2] * 60 + [3] * 50
    cls = [0] * ncap
    sub = list(range(ncap))
    rank = [0] * ncap
    for i in (5, 9, 25, 26, 70, 71, 90):
        rank[i] = 4 + (i & 3)
    rank[8] = 0x83                                  # rank 3 and the snap bit
    clipf, df = check_clip(gpu, rank, cls, sub, f_seg, 4, P)
    assert clipf == [5, 25, 70, 150]
    assert sum(df) == 15 + 15 + 30
    # the same segment's overflow in its first wave only, and in both
    rank2 = [0] * ncap
    rank2[41] = 9
    assert check_clip(gpu, rank2, cls, sub, f_seg, 4, P)[0] == \
        [150, 150, 41, 150]
    rank2[99] = 9
    rank2[149] = 0x7f
    assert check_clip(gpu, rank2, cls, sub, f_seg, 4, P)[0] == \
        [150, 150, 41, 149]
    # an overflow in class 0 only: frames of the other classes index other
    # tables with their sub (a rank byte there that says "overflow" is not
    # theirs) and are deferred behind a class-0 overflow of their segment
    classes = [2, 0, 1, 2, 2, 0, 1, 0, 2]
    f_seg = [0, 0, 0, 0, 1, 1, 1, 2, 2]
    rank = [0, 9, 0, 9, 9, 9, 9, 9, 9]              # class 0: subs 0, 1, 2
    clipf, df = check_clip(gpu, rank, classes, _subs(classes), f_seg, 3, P)
    assert clipf == [9, 5, 9] and df == [0, 0, 0, 0, 0, 1, 1, 0, 0]
    # f_seg already -1, and outside the table: no overflow, not deferred
    f_seg = [0, -1, 0, 7, 0, 0]
    clipf, df = check_clip(gpu, [0, 9, 0, 9, 9, 0], [0] * 6, list(range(6)),
                           f_seg, 1, P)
    assert clipf == [4] and df == [0, 0, 0, 0, 1, 1]
    # frames past the device count are not looked at; a sub outside the table
    assert check_clip(gpu, [0, 0, 9, 9], [0] * 4, list(range(4)), [0] * 4, 1,
                      P, nfr=2)[0] == [4]
    assert check_clip(gpu, [9, 9], [0, 0], [-1, 2], [0, 0], 1, P)[0] == [2]
    # passes is the bound: a rank of passes - 1 stays
    assert check_clip(gpu, [3, 4], [0, 0], [0, 1], [0, 1], 2, P)[0] == [2, 1]
    assert check_clip(gpu, [3, 4], [0, 0], [0, 1], [0, 1], 2, 5)[0] == [2, 2]


@pytest.mark.parametrize('ncap,S', [(1, 1), (64, 3), (65, 65), (1000, 40)])
def test_clip_random_tables(gpu, ncap, S):
    rng = np.random.RandomState(ncap + S)
    for k in range(4):
        seg = np.sort(rng.randint(0, S, size=ncap)).tolist()
        for j in rng.randint(0, ncap, size=ncap // 8):
            seg[j] = int(rng.choice([-1, S, S + 3]))
        classes = rng.choice([0, 0, 0, 1, 2], size=ncap).tolist()
        rank = (rng.choice([0, 1, 2, 3, 3, 4, 6], size=ncap) |
                (rng.randint(0, 2, size=ncap) << 7)).tolist()
        if k == 1:
            rank = [r & 0x83 for r in rank]                # no overflow
        nfr = ncap if k < 3 else int(rng.randint(0, ncap + 1))
        check_clip(gpu, rank, classes, _subs(classes), seg, S, 4, nfr)


# ---- the ranges --------------------------------------------------------------

@pytest.mark.parametrize('S', [1, 3, 65, 300])
def test_ranges(gpu, S):
    rng = np.random.RandomState(S)
    ncap = 4 * S + 3
    d = lambda v: torch.tensor(v, dtype=I64, device=gpu)
    for k in range(4):
        nfr = int(rng.randint(0, ncap + 1)) if k else ncap
        starts = np.sort(rng.randint(0, 5000, size=S + 1)).tolist()
        rep = np.sort(rng.randint(0, 5000, size=S + 1)).tolist()
        rec = rng.randint(-10, 5100, size=ncap).tolist()
        off = rng.randint(-10, 5100, size=ncap).tolist()
        clipf = rng.randint(-2, ncap + 2, size=S).tolist()
        if k == 2:
            clipf = [ncap] * S                              # no clip
        rep_end = torch.full((S,), -7, dtype=I64, device=gpu)
        used = torch.full((S,), -7, dtype=I64, device=gpu)
        _lib.order_clip_ranges(d(clipf), d(rep), d(rec), d(off), d(starts),
                               d([nfr]), ncap, rep_end, used)
        want = M.ranges(clipf, rep, rec, off, starts, nfr)
        assert list(zip(rep_end.cpu().tolist(), used.cpu().tolist())) == want
        if k == 2:
            assert [w[0] for w in want] == rep[1:]
            assert [w[1] for w in want] == np.diff(starts).tolist()


# ---- the reply ends in the TX pieces ---------------------------------------------

def _pieces(dev, wslots, rep_off, so, caps, rep_end, with_kw):
    S = len(wslots)
    d = lambda v, t=I64: torch.tensor(v, dtype=t, device=dev)
    owner = torch.zeros(64, dtype=I64, device=dev)
    ps = torch.full((4 * S,), -7, dtype=I32, device=dev)
    src = torch.full((4 * S,), -7, dtype=I64, device=dev)
    ln = torch.full((4 * S,), -7, dtype=I64, device=dev)
    stats = torch.zeros(8, dtype=I64, device=dev)
    args = (d(rep_off), d(wslots, I32), d(so[0]), d(so[1]), d(so[2]), None,
            caps, owner, ps, src, ln, stats)
    if with_kw:
        _lib.front_tx_pieces(*args, rep_end=None if rep_end is None
                             else d(rep_end))
    else:
        _lib.front_tx_pieces(*args)
    return list(zip(ps.cpu().tolist(), src.cpu().tolist(),
                    ln.cpu().tolist()))


def test_tx_pieces_reply_ends(gpu):
    rng = np.random.RandomState(9)
    S = 70
    caps = (4000, 700, 800, 900)
    wslots = [int(x) for x in rng.randint(-1, 64, size=S)]
    rep = np.sort(rng.randint(0, caps[0] + 1, size=S + 1)).tolist()
    so = []
    for k in range(3):
        cuts = sorted(int(x) for x in rng.randint(0, caps[k + 1] + 1,
                                                  size=63))
        so.append([0] + cuts + [caps[k + 1]])
    # without rep_end: the call of before, with and without the keyword
    plain = _pieces(gpu, wslots, rep, so, caps, None, False)
    assert _pieces(gpu, wslots, rep, so, caps, None, True) == plain
    assert plain == F.pieces(wslots, rep, so, None, caps)[1]
    # with it: the reply piece ends there, nothing else moves
    ends = [int(rng.randint(rep[s], rep[s + 1] + 1)) for s in range(S)]
    ends[3] = rep[3]                                   # all of it deferred
    ends[4] = rep[5]                                   # none of it
    got = _pieces(gpu, wslots, rep, so, caps, ends, True)
    want = list(plain)
    for s in range(S):
        want[4 * s] = (0, rep[s], ends[s] - rep[s])
    assert got == want
    assert got[12][2] == 0
