"""GpuServer.serve_sessions_mixed(ordered=True, passes=P, defer=...): the
serve's class of a session batch of any op mix through the ordered session
serve, and deferral in place of the rank refusal (csrc/kernels/tree_order.hip
ord_clip_*; the rules: csrc/kernels/zk_order_clip.h).  time.time is frozen so
two trees' Stats compare exactly."""

import random
import time

import numpy as np
import pytest
import torch

from test_gpu_sessions import FANOUT, NLEAF, _segments, dirp, leaf
from treemodel import (TreeModel, _stream, create, delete, dev_bytes, exists,
                       get, set_data)
from watchmodel import ls, set_watches, wget

from zkmi import jute
from zkmi.ops import _lib

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000.0
I64, I32, U8 = torch.int64, torch.int32, torch.uint8


@pytest.fixture(autouse=True)
def _frozen_time(monkeypatch):
    monkeypatch.setattr(time, 'time', lambda: NOW)


def _server(gpu, acl=False, frames=1024):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(NLEAF, 16, fanout=FANOUT, device=gpu, seed=3,
                   watch_cap=4096, scratch=1 << 20,
                   ctime_ms=int(NOW * 1000), acl_cap=512 if acl else 0)
    return GpuServer(tree, frames, 1 << 21)


def _raw(buf, total):
    return bytes(buf[:int(total)].cpu().numpy().tobytes())


def _xids(conns):
    for _, _, pk in conns:
        for k, p in enumerate(pk):
            p['xid'] = 1 + k


def _table(gpu, conns, parts):
    cuts = [0] + [int(x) for x in np.cumsum([len(b) for b in parts])]
    return cuts, _segments(gpu, cuts, [s for s, _, _ in conns],
                           [w for _, w, _ in conns])


def _decode(part, pk):
    frames, used, bad = jute.scan_frames(part)
    assert bad < 0 and used == len(part)
    xmap = {p['xid']: p['opcode'] for p in pk}
    return [jute.decode_response(part[o:o + ln], xmap) for o, ln in frames]


def _notes(srv):
    """The batch's grouped notification bytes and their slot table."""
    buf, total, _, count = srv.notif
    return (_raw(buf, total.item()), int(count.item()),
            srv.notif_slots[1].cpu().tolist())


def _serve(srv, gpu, conns, parts=None, **kw):
    """One serve_sessions_mixed batch -> (per connection its decoded replies,
    raw out, rep_off).  ``parts``: the connections' bytes when they are not
    the whole of ``conns``' packets.  With ``defer`` a connection's replies
    are its slice up to rep_end."""
    if parts is None:
        _xids(conns)
        parts = [_stream(pk) for _, _, pk in conns]
    rx = b''.join(parts)
    _, segs = _table(gpu, conns, parts)
    out, total, err, ft = srv.serve_sessions_mixed(
        dev_bytes(rx, gpu), len(rx), segs, **kw)
    assert int(err.item()) == 0
    raw = _raw(out, total.item())
    off = srv.seg.rep_off.cpu().tolist()
    assert off[0] == 0 and off[-1] == len(raw) and off == sorted(off)
    end = off[1:]
    if kw.get('defer') is not None:
        end = kw['defer'].rep_end.cpu().tolist()
        assert all(a <= e <= b for a, e, b in zip(off, end, off[1:]))
    reps = []
    for s, (_, _, pk) in enumerate(conns):
        reps.append(_decode(raw[off[s]:end[s]], pk))
    return reps, raw, off


# ---- (a) serve-class batches equal serve_sessions(ordered=True) ----------------

def _serve_class_batch(rng, n, S):
    """n requests of the serve's class on a small pool of paths (chains of any
    length: a rank past the passes is refused alike on both sides), some reads
    with a watch, over S connections with empty ones among them."""
    pool = [leaf(i) for i in rng.sample(range(NLEAF), max(4, n // 5))]
    new = [dirp(rng.randrange(8)) + '/o%04d' % k for k in range(n // 6 + 1)]
    pk = []
    for _ in range(n):
        r = rng.random()
        if r < 0.3:
            pk.append(set_data(rng.choice(pool), b'v%d' % rng.randrange(99)))
        elif r < 0.4:
            pk.append(delete(rng.choice(pool)))
        elif r < 0.55:
            pk.append(create(rng.choice(new), b'n',
                             ['EPHEMERAL'] if rng.random() < 0.3 else []))
        elif r < 0.6:
            pk.append(create(dirp(rng.randrange(8)) + '/s', b'q',
                             ['SEQUENTIAL']))
        elif r < 0.8:
            pk.append(wget(rng.choice(pool + new), rng.random() < 0.5))
        else:
            pk.append(exists(rng.choice(pool + new)))
    at = sorted(rng.randrange(n + 1) for _ in range(S - 1))
    at = [0] + at + [n]
    return [(0x100 + s, (-1 if s % 5 == 4 else (7 * s) % 64), pk[a:b])
            for s, (a, b) in enumerate(zip(at, at[1:]))]


@pytest.mark.parametrize('n,S', [(1, 1), (65, 3), (300, 65)])
def test_serve_class_equals_serve_sessions_ordered(gpu, n, S):
    sx, sy = _server(gpu), _server(gpu)
    rng = random.Random(31 * n + S)
    fired = 0
    for gen in range(3):
        conns = _serve_class_batch(rng, n, S)
        _xids(conns)
        parts = [_stream(pk) for _, _, pk in conns]
        rx = b''.join(parts)
        _, segs = _table(gpu, conns, parts)
        ox, tx, ex, _ = sx.serve_sessions_mixed(
            dev_bytes(rx, gpu), len(rx), segs, ordered=True, passes=4)
        oy, ty, ey, _ = sy.serve_sessions(
            dev_bytes(rx, gpu), len(rx), segs, ordered=True, passes=4)
        assert int(ex.item()) == int(ey.item()) == 0
        assert _raw(ox, tx.item()) == _raw(oy, ty.item()), gen
        assert sx.seg.rep_off.cpu().tolist() == sy.seg.rep_off.cpu().tolist()
        assert _notes(sx) == _notes(sy), gen
        assert sx.tree.digest() == sy.tree.digest(), gen
        assert int(sx.tree.counters[_lib.TC_ZXID].item()) == \
            int(sy.tree.counters[_lib.TC_ZXID].item())
        assert sx.order_stats() == sy.order_stats()
        assert sx.tree.watch_census() == sy.tree.watch_census()
        fired += _notes(sx)[1]
    if n >= 65:
        assert sx.order_stats()[0] >= 1
    if n == 300:
        assert fired > 0                                # watches did fire


# ---- (b) chains over four connections against the model ----------------------

def test_chains_with_lists_against_the_model(gpu):
    """Four connections, each in a directory of its own: per path a chain
    create -> set -> get -> (delete), the chains interleaved, then lists of
    the directory and GET_ACL of what stayed — about 200 frames.  The model
    (the fake server's database) applies the batch request by request in
    batch order; with disjoint directories and a connection's lists behind
    its writes that is what the engines' fixed sequence gives too."""
    srv = _server(gpu, acl=True)
    m = TreeModel(srv.tree, srv, gpu)
    rng = random.Random(5)
    sid = [m.session() for _ in range(4)]
    conns = []
    for s in range(4):
        d = dirp(s)
        chains = []
        kept = []
        for k in range(11):
            p = d + '/c%02d' % k
            ops = [create(p, b'a%d' % k), set_data(p, b'bb%d' % k), get(p)]
            if k % 3 == 0:
                ops.append(delete(p))
            else:
                kept.append(p)
            chains.append(ops)
        # an existing leaf: set -> set -> get -> exists (ranks 0..3)
        old = leaf(s * FANOUT + 7)
        chains.append([set_data(old, b'x'), set_data(old, b'yy'), get(old),
                       exists(old)])
        pk = []
        live = [c for c in chains if c]
        while live:
            c = rng.choice(live)
            pk.append(c.pop(0))
            if not c:
                live.remove(c)
        pk += [ls(d, watch=False), ls(d, watch=False, stat=False)]
        pk += [{'opcode': 'GET_ACL', 'path': p} for p in kept[:3]]
        pk.append({'opcode': 'GET_ACL', 'path': d + '/c00'})     # deleted
        conns.append((sid[s], -1, pk))
    nfr = sum(len(pk) for _, _, pk in conns)
    assert 180 <= nfr <= 220
    base = m.counter(_lib.TC_ZXID)
    reps, _, _ = _serve(srv, gpu, conns, ordered=True, passes=4)
    assert srv.order_stats()[0] == 3                    # no rank was refused
    i = 0
    for (s_id, _, pk), rs in zip(conns, reps):
        assert [r['xid'] for r in rs] == [p['xid'] for p in pk]
        for p, r in zip(pk, rs):
            i += 1
            if p['opcode'] in ('GET_CHILDREN', 'GET_CHILDREN2', 'GET_ACL'):
                w = m.db.handle(dict(p), s_id)
                assert r['err'] == w['err'], (p, r)
                if w['err'] != 'OK':
                    continue
                if p['opcode'] == 'GET_ACL':
                    # (the model's reply through the codec: one spelling)
                    w = jute.decode_response(jute.encode_response(w),
                                             {p['xid']: 'GET_ACL'})
                    assert r['acl'] == w['acl'], (p, r)
                else:
                    assert sorted(r['children']) == sorted(w['children'])
                    assert len(r['children']) >= 7
            else:
                want = m._apply(p, s_id, base + i, False)
                assert m._reply_key(r, False) == want, (p, r, want)
    m.audit(zxids=False)


# ---- (c) deferral ------------------------------------------------------------

def test_deferral(gpu):
    from zkmi.server.engine import OrderDefer
    srv = _server(gpu)
    m = TreeModel(srv.tree, srv, gpu)
    hot, other = leaf(3), leaf(FANOUT + 4)
    S = 8
    sid = [m.session() for _ in range(S)]
    df = OrderDefer(S, gpu)
    # watcher 40 watches /hot; the eight connections' reads of /other set a
    # data watch for their own slots
    _serve(srv, gpu, [(sid[0], 40, [wget(hot)])])
    conns = [(sid[s], s, [set_data(hot, b'h%d' % s), wget(other)])
             for s in range(S)]
    _xids(conns)
    parts = [_stream(pk) for _, _, pk in conns]
    cuts, _ = _table(gpu, conns, parts)
    reps, raw, off = _serve(srv, gpu, conns, parts, ordered=True, passes=4,
                            defer=df)
    used = df.used.cpu().tolist()
    end = df.rep_end.cpu().tolist()
    clipf = df.clipf.cpu().tolist()
    assert used == [len(b) for b in parts[:4]] + [0] * 4
    assert end == off[1:5] + off[4:8]
    assert clipf == [1024] * 4 + [8, 10, 12, 14]
    assert int(df.deferred.item()) == 8
    assert srv.order_stats()[0] == 7
    # the first four: served, in batch order; the others: nothing
    for s in range(S):
        if s >= 4:
            assert reps[s] == []
            continue
        w = m._apply(conns[s][2][0], sid[s], 0, False)
        assert m._reply_key(reps[s][0], False) == w
        assert reps[s][0]['stat'].version == s + 1
        w = m._apply(conns[s][2][1], sid[s], 0, False)
        assert m._reply_key(reps[s][1], False) == w
    # the deferred frames' placeholders lie behind the ends and were not sent
    assert srv.seg.f_seg[:16].cpu().tolist() == \
        [0, 0, 1, 1, 2, 2, 3, 3] + [-1] * 8
    # one event (watcher 40, the first set); nothing is addressed from the
    # deferred frames, and their reads armed nothing
    note, count, slot_off = _notes(srv)
    assert count == 1 and slot_off[40] == 0 and slot_off[41] == len(note)
    assert srv.watch_stats()['events_fired'] == 1
    # a write of /other now reaches watchers 0..3 only (the model's version
    # of /other moves with it)
    wr = set_data(other, b'o')
    rs, _, _ = _serve(srv, gpu, [(sid[0], -1, [wr])])
    assert m._reply_key(rs[0][0], False) == m._apply(wr, sid[0], 0, False)
    note, count, slot_off = _notes(srv)
    assert count == 4
    assert [slot_off[w + 1] - slot_off[w] > 0 for w in range(9)] == \
        [True] * 4 + [False] * 5
    # the second call, with the remaining bytes
    rest = [b[u:] for b, u in zip(parts, used)]
    assert [len(b) for b in rest] == [0] * 4 + [len(b) for b in parts[4:]]
    reps, raw, off = _serve(srv, gpu, conns, rest, ordered=True, passes=4,
                            defer=df)
    assert df.used.cpu().tolist() == [len(b) for b in rest]
    assert df.rep_end.cpu().tolist() == off[1:]
    assert int(df.deferred.item()) == 0
    for s in range(4, S):
        w = m._apply(conns[s][2][0], sid[s], 0, False)
        assert m._reply_key(reps[s][0], False) == w
        assert reps[s][0]['stat'].version == s + 1
        w = m._apply(conns[s][2][1], sid[s], 0, False)
        assert m._reply_key(reps[s][1], False) == w
    assert reps[:4] == [[]] * 4
    rs, _, _ = _serve(srv, gpu, [(sid[0], -1, [get(hot)])])
    assert rs[0][0]['stat'].version == 8 and rs[0][0]['data'] == b'h7'
    m.audit(zxids=False)


def test_deferred_sequential_create_keeps_its_number(gpu):
    """SEQUENTIAL creates A, B, C, D under one parent from four connections,
    B behind an overflowing set on its connection: B is deferred after the
    numbering pass gave it a number.  That number stays out of use (a gap in
    the parent's cversion, as every refused numbered create leaves): were it
    handed back, B's name in the next batch would be D's.  The model applies
    the served frames in batch order and bumps the parent's cversion where
    the deferred numbered create stood; names, Stats and the parent's
    cversion / numChildren agree over both batches."""
    from zkmi.server.engine import OrderDefer
    srv = _server(gpu)
    m = TreeModel(srv.tree, srv, gpu)
    hot, d = leaf(3), dirp(5)
    sid = [m.session() for _ in range(4)]
    df = OrderDefer(4, gpu)
    seq = lambda: create(d + '/q-', b's', ['SEQUENTIAL'])
    conns = [(sid[0], -1, [seq()]),
             (sid[1], -1, [set_data(hot, b'h%d' % k) for k in range(5)] +
              [seq()]),
             (sid[2], -1, [seq()]),
             (sid[3], -1, [seq(), seq()])]
    _xids(conns)
    parts = [_stream(pk) for _, _, pk in conns]
    c0 = m.db.nodes[d].stat.cversion

    def parent():
        p = exists(d)
        rs, _, _ = _serve(srv, gpu, [(sid[0], -1, [p])])
        assert m._reply_key(rs[0][0], False) == m._apply(p, sid[0], 0, False)
        return rs[0][0]['stat']

    reps, _, _ = _serve(srv, gpu, conns, parts, ordered=True, passes=4,
                        defer=df)
    assert [len(rs) for rs in reps] == [1, 4, 1, 2]
    assert int(df.deferred.item()) == 2
    names = []
    for s, (_, _, pk) in enumerate(conns):
        for k, p in enumerate(pk):
            if k < len(reps[s]):
                want = m._apply(p, sid[s], 0, False)
                assert m._reply_key(reps[s][k], False) == want, (s, k)
                if p['opcode'] == 'CREATE':
                    names.append(reps[s][k]['path'])
            elif p['opcode'] == 'CREATE':
                m.db.nodes[d].stat.cversion += 1          # the gap
    assert names == [d + '/q-%010d' % (c0 + k) for k in (0, 2, 3, 4)]
    st = parent()
    assert st.cversion == c0 + 5 and st.numChildren == FANOUT + 4
    # the next batch: the deferred frames, B numbered past every name given
    used = df.used.cpu().tolist()
    rest = [b[u:] for b, u in zip(parts, used)]
    assert [len(b) > 0 for b in rest] == [False, True, False, False]
    reps, _, _ = _serve(srv, gpu, conns, rest, ordered=True, passes=4,
                        defer=df)
    assert int(df.deferred.item()) == 0 and len(reps[1]) == 2
    for p, r in zip(conns[1][2][4:], reps[1]):
        assert m._reply_key(r, False) == m._apply(p, sid[1], 0, False)
    assert reps[1][1]['err'] == 'OK'
    assert reps[1][1]['path'] == d + '/q-%010d' % (c0 + 5)
    st = parent()
    assert st.cversion == c0 + 6 and st.numChildren == FANOUT + 5
    m.audit(zxids=False)


def test_defer_none_refuses_as_the_library(gpu):
    """ordered=True without defer: the overflow is answered SYSTEMERROR, as
    serve_sessions(ordered=True) does."""
    srv = _server(gpu)
    hot = leaf(3)
    conns = [(0x100 + s, -1, [set_data(hot, b'h%d' % s)]) for s in range(6)]
    reps, _, _ = _serve(srv, gpu, conns, ordered=True, passes=4)
    assert [rs[0]['err'] for rs in reps] == ['OK'] * 4 + ['SYSTEM_ERROR'] * 2
    with pytest.raises(ValueError):
        from zkmi.server.engine import OrderDefer
        _serve(srv, gpu, conns, defer=OrderDefer(6, gpu))


# ---- (d) a deferred frame has no effect --------------------------------------

def test_deferred_frames_have_no_effect(gpu):
    """Behind an overflowing set on their connections: a CLOSE_SESSION closes
    nothing, a watch=1 list arms nothing, a SET_WATCHES catches nothing up."""
    from zkmi.server.engine import OrderDefer
    from zkmi.server.sessions import GpuSessionTable
    srv = _server(gpu)
    hot, d = leaf(3), dirp(5)
    S = 7
    df = OrderDefer(S, gpu)
    zx = int(srv.tree.counters[_lib.TC_ZXID].item())
    tail = [
        [{'opcode': 'CLOSE_SESSION'}],
        [ls(d, watch=True)],
        [set_watches((0, 0), data=[hot], child=[d])],
    ]
    conns = [(0x200 + s, s, [set_data(hot, b'h%d' % s)]) for s in range(4)]
    conns += [(0x200 + 4 + k, 4 + k, [set_data(hot, b'z')] + t)
              for k, t in enumerate(tail)]
    census = srv.tree.watch_census()
    reps, _, off = _serve(srv, gpu, conns, ordered=True, passes=4, defer=df,
                          resume=True, close=True)
    assert [len(rs) for rs in reps] == [1] * 4 + [0] * 3
    assert df.used.cpu().tolist()[4:] == [0, 0, 0]
    assert int(df.deferred.item()) == 6
    cs = srv.close_stats()
    assert cs['frames'] == 0 and cs['sessions'] == 0 and cs['removed'] == 0
    rs = srv.resume_stats()
    assert rs['events'] == 0 and rs['rearmed'] == 0 and rs['listed'] == 0
    assert srv.tree.watch_census() == census
    assert srv.watch_stats()['events_fired'] == 0
    # (the zxids of the serve's class are the batch's, deferred or not)
    assert int(srv.tree.counters[_lib.TC_ZXID].item()) == zx + 9
    # served on their own they do all three
    conns2 = [(c[0], c[1], c[2][1:]) for c in conns[4:]]
    reps, _, _ = _serve(srv, gpu, conns2, ordered=True, passes=4,
                        defer=OrderDefer(3, gpu), resume=True, close=True)
    assert [rs[0]['err'] for rs in reps] == ['OK'] * 3
    assert srv.close_stats()['frames'] == 1
    rs = srv.resume_stats()
    assert rs['listed'] == 2 and rs['events'] >= 1
    assert srv.tree.watch_census() != census


# ---- (e) ordered=False is the call of before ---------------------------------

def test_unordered_keywords_change_nothing(gpu):
    sx, sy = _server(gpu, acl=True), _server(gpu, acl=True)
    rng = random.Random(9)
    for gen in range(2):
        # (an unordered batch is deterministic only without conflicts: every
        # request has a path of its own)
        paths = [leaf(i) for i in rng.sample(range(NLEAF), 120)]
        pk = []
        for k, p in enumerate(paths):
            pk.append([set_data(p, b'v%d' % k), delete(p), wget(p, k % 2),
                       exists(p), create(p + 'x', b'n'),
                       create(dirp(k % 8) + '/s', b'q', ['SEQUENTIAL'])][k % 6])
        conns = [(0x100 + s, 7 * s, pk[24 * s:24 * s + 24]) for s in range(5)]
        conns[1][2].append(ls('/bench', watch=True))
        conns[3][2].append({'opcode': 'GET_ACL', 'path': dirp(2)})
        _xids(conns)
        parts = [_stream(pk) for _, _, pk in conns]
        rx = b''.join(parts)
        _, segs = _table(gpu, conns, parts)
        ox, tx, ex, _ = sx.serve_sessions_mixed(
            dev_bytes(rx, gpu), len(rx), segs, ordered=False, passes=4,
            defer=None)
        oy, ty, ey, _ = sy.serve_sessions_mixed(dev_bytes(rx, gpu), len(rx),
                                                segs)
        assert int(ex.item()) == int(ey.item()) == 0
        assert _raw(ox, tx.item()) == _raw(oy, ty.item())
        assert _notes(sx) == _notes(sy)
        assert sx.tree.digest() == sy.tree.digest()
        assert sx.seg.rep_off.cpu().tolist() == sy.seg.rep_off.cpu().tolist()
