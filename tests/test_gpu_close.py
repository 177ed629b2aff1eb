"""Closing and expiring many sessions in one pass (csrc/kernels/tree_close.hip;
the rules: zk_close.h): GpuServer.close_sessions against a loop of
GpuServer.expire calls on a twin tree, and the CLOSE_SESSION frames of a
session batch (serve_sessions / serve_sessions_mixed with close=True).

The models are tests/treemodel.py and tests/watchmodel.py, subclassed here:
``close`` applies the listed sessions' expiries to the fake server's database
one by one (session rank k's removals carry the counter + k + 1) and then
asks the GPU for all of them at once.  time.time is frozen, so twin models
hand out the same session ids and two trees' Stats compare exactly.  All
comparisons are exact."""

import collections
import struct
import time

import numpy as np
import pytest
import torch

from treemodel import (TreeModel, _parent, _stream, create, delete, dev_bytes,
                       get, set_data, window_names)
from watchmodel import (WatchModel, check_events, decode_notifications, ls,
                        wexists, wget)

from zkmi import jute
from zkmi.ops import _lib

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000.0
D0 = '/bench/d000000'
HCAP = 4096
I64, I32, U8 = torch.int64, torch.int32, torch.uint8
OK, SYSTEM, UNIMPLEMENTED, BAD_ARGUMENTS, SESSION_EXPIRED = 0, -1, -6, -8, -112
CLOSE_SESSION = -11


@pytest.fixture(autouse=True)
def _frozen_time(monkeypatch):
    monkeypatch.setattr(time, 'time', lambda: NOW)


# ---- the models -------------------------------------------------------------

class _Close(object):
    """The close pass on a model: mixed into TreeModel / WatchModel."""

    def model_close(self, sids):
        """Expire ``sids`` on the database one by one; the nodes each
        removed."""
        base = self.counter(_lib.TC_ZXID)
        want = []
        for k, sid in enumerate(sids):
            z = base + k + 1
            s = self.db.sessions.get(sid)
            gone = sorted(s.ephemerals) if s is not None else []
            for path in gone:
                assert path in self.db.nodes
                par = _parent(path)
                self.zx[par][2] = max(self.zx[par][2], z)
                self.touched.add(par)
                del self.zx[path]
                self.dead.add(path)
            self.db.expire_session(sid)
            want.append(len(gone))
        return base, want

    def gpu_close(self, sids, wslots=None):
        dev = self.dev
        w = None if wslots is None else \
            torch.tensor(list(wslots), dtype=I32, device=dev)
        r = self.srv.close_sessions(
            torch.tensor(list(sids), dtype=I64, device=dev), w)
        return r.cpu().tolist()


class CloseModel(_Close, TreeModel):
    def close(self, sids, audit=True):
        base, want = self.model_close(sids)
        got = self.gpu_close(sids)
        assert got == want, (got, want)
        assert self.counter(_lib.TC_ZXID) == base + len(sids)
        st = self.srv.close_stats()
        assert (st['frames'], st['sessions'], st['removed']) == \
            (0, len(sids), sum(want)), st
        if audit:
            self.audit()
        return got


def slot_events(notif, slots):
    """{slot: [(type, path)]} of a slot-major notification stream, each
    slot's decoded from its own slice of the bytes."""
    buf, total, sl, count = notif
    n = int(count.item())
    raw = bytes(buf[:int(total.item())].cpu().numpy().tobytes())
    ev = decode_notifications(buf, total.item(), n)
    sl = sl[:n].cpu().tolist()
    first, off = (x.cpu().tolist() for x in slots)
    assert first[0] == 0 and first[64] == n, (first, n)
    assert off[0] == 0 and off[64] == len(raw), (off, len(raw))
    assert first == sorted(first) and off == sorted(off)
    out = {}
    for w in range(64):
        a, b = first[w], first[w + 1]
        assert sl[a:b] == [w] * (b - a), (w, sl[a:b])
        part = raw[off[w]:off[w + 1]]
        frames, used, bad = jute.scan_frames(part)
        assert bad < 0 and used == len(part) and len(frames) == b - a
        got = []
        for o, ln in frames:
            pkt = jute.decode_response(part[o:o + ln], {})
            assert pkt['xid'] == -1
            got.append((pkt['type'], pkt['path']))
        assert got == ev[a:b]
        if got:
            out[w] = got
    return out


class CloseWatchModel(_Close, WatchModel):
    def close(self, sids, audit=True):
        """Close ``sids`` at once: removed[], the zxid counter, the
        survivors' events (multisets, each watcher's from its own slice),
        nothing for a closer, no loss.  Returns {slot: [(type, path)]}."""
        slot_of = {x: s for s, x in self.slot_sid.items()}
        wslots = [slot_of.get(sid, -1) for sid in sids]
        closers = {w for w in wslots if w >= 0}
        lens = self._lens()
        base, want_removed = self.model_close(sids)
        want = []
        self._since(lens, 0, want)
        want = [e for e in want if e[1] not in closers]
        got = self.gpu_close(sids, wslots)
        assert got == want_removed, (got, want_removed)
        assert self.counter(_lib.TC_ZXID) == base + len(sids)
        for w in closers:
            del self.slot_sid[w]
            del self.conns[w]
        sent = slot_events(self.srv.close_notif, self.srv.close_slots)
        assert not (set(sent) & closers), sent
        bad = check_events(sent, want, False)
        assert bad is None, bad
        st = self.srv.close_stats()
        assert st == {'frames': 0, 'sessions': len(sids),
                      'removed': sum(want_removed),
                      'events_fired': len(want), 'events_written': len(want),
                      'records_dropped': 0, 'encode_err': 0}, st
        if audit:
            self.audit()
        return sent


def _tree(gpu, cls=CloseModel, cap_frames=1024, **kw):
    """The churn tests' smallest tree: 12 static nodes, 1024 spare, 4096
    index entries (the windowed names are chosen for this table size)."""
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(10, 16, fanout=10, device=gpu, spare=0.0, **kw)
    assert (tree.cap, tree.hcap) == (1036, HCAP)
    srv = GpuServer(tree, cap_frames, 1 << 20)
    return cls(tree, srv, gpu)


def _twins(gpu, **kw):
    return _tree(gpu, **kw), _tree(gpu, **kw)


def _both(a, b, fn):
    ra, rb = fn(a), fn(b)
    assert ra == rb, (ra, rb)
    return ra


def _same(a, b):
    """The two trees hold the same znodes with the same Stats, and their
    zxid counters agree."""
    da, db = a.tree.digest(), b.tree.digest()
    assert da[:2] == db[:2], (da, db)
    assert a.counter(_lib.TC_ZXID) == b.counter(_lib.TC_ZXID)


def _serve_ok(m, pk, sid=0):
    reps, _ = m.serve(pk, sid=sid, audit=False)
    assert all(r['err'] == 'OK' for r in reps), \
        collections.Counter(r['err'] for r in reps)


# ---- 1. differential against the loop ---------------------------------------

def test_close_equals_expire_loop(gpu):
    """Three closing sessions', one surviving session's and persistent names
    interleaved in one 16-entry window of the index, over 20 create / close
    rounds on twin trees: close_sessions([s0, s1, s2]) on one,
    expire(s0); expire(s1); expire(s2) on the other.  Digest, zxid counter,
    removed[k] and — through each model's audit — every parent's cversion /
    numChildren / pzxid, every survivor (read back through the index the
    shift moved entries in while several sessions' erasers ran) and every
    removed name (NO_NODE, then created again the next round) agree; no
    create ever finds the index full."""
    a, b = _twins(gpu)
    names = window_names(300, HCAP)
    for k, p in enumerate(names):
        s = int(_lib.acl_hash(p.encode()) & (HCAP - 1))
        assert s >= HCAP - 8 or s < 8
    role = {p: k % 5 for k, p in enumerate(names)}     # 0..2 close, 3 stays
    stay = _both(a, b, lambda m: m.session())
    for m in (a, b):
        _serve_ok(m, [create(p, b'keep', ['EPHEMERAL']) for p in names
                      if role[p] == 3], sid=stay)
        _serve_ok(m, [create(p, b'plain') for p in names if role[p] == 4])
    removed_all = 0
    for r in range(20):
        sids = [_both(a, b, lambda m: m.session()) for _ in range(3)]
        for j, sid in enumerate(sids):
            # (a rotating part of each closer's names, so the runs differ)
            pk = [create(p, b'%d' % r, ['EPHEMERAL'])
                  for k, p in enumerate(names)
                  if role[p] == j and (k // 5 + r) % 4 != 0]
            for m in (a, b):
                _serve_ok(m, pk, sid=sid)
        if r % 4 == 3:
            # plain tombstones between the owners' entries
            gone = [p for p in names
                    if role[p] == 4 and p in a.db.nodes][r % 3::3]
            for m in (a, b):
                _serve_ok(m, [delete(p) for p in gone])
                _serve_ok(m, [create(p, b'again') for p in gone[::2]])
        assert a.counter(_lib.TC_ZXID) == b.counter(_lib.TC_ZXID)
        # (close checks removed[] and the counter, base + 3, before it
        # audits; the audits' reads move both trees' counters alike)
        got = a.close(sids)
        want = [b.expire(sids[0], audit=False),
                b.expire(sids[1], audit=False), b.expire(sids[2])]
        assert got == want and min(got) >= 40, (got, want)
        removed_all += sum(got)
        _same(a, b)
    assert removed_all > 2500
    for m in (a, b):
        _, live, used, tomb = m.tree.digest()
        # survivors, the static nodes and what is left of the plain names;
        # twenty rounds of ~135 removals left no tombstone pile behind
        assert 12 + 60 <= live <= 12 + 120 and used < HCAP // 4, (live, used)


# ---- 2. edge lists ----------------------------------------------------------

def test_edge_lists(gpu):
    """Each list against its sequential counterpart on the twin: K = 1, an
    id listed twice, id 0 and an unknown id (they remove nothing and take
    their zxid), a session without ephemerals, and 65 sessions of one node
    each whose nodes sit in neighbouring node slots (a wave of the removal
    meets as many distinct ranks as it has lanes)."""
    a, b = _twins(gpu)
    names = window_names(200, HCAP)

    def born(n, per, start):
        """n sessions with `per` ephemerals each, on both trees."""
        sids = []
        for j in range(n):
            sid = _both(a, b, lambda m: m.session())
            pk = [create(p, b'e', ['EPHEMERAL'])
                  for p in names[start + j * per:start + (j + 1) * per]]
            for m in (a, b):
                _serve_ok(m, pk, sid=sid)
            sids.append(sid)
        return sids

    def run(lst, seq):
        """close(lst) on a, the expiries `seq` on b."""
        got = a.close(lst)
        want = [b.expire(s, audit=False) for s in seq]
        b.audit()
        assert got == want, (got, want)
        _same(a, b)
        return got

    # K = 1 equals expire
    s, = born(1, 7, 0)
    assert run([s], [s]) == [7]
    # an id listed twice: removed at its first position
    s, t = born(2, 5, 0)
    assert run([s, t, s, t], [s, t, s, t]) == [5, 5, 0, 0]
    # id 0 and an unknown id (expire(0) is not the counterpart of a listed
    # 0: the one-session sweep takes "owner 0" at its word; an unknown id
    # stands in for it)
    s, = born(1, 4, 0)
    u, u2 = (1 << 56) | 0x7777, (1 << 56) | 0x7778
    persistent = a.tree.digest()[1]
    assert run([0, u, s, 0], [u2, u, s, u2]) == [0, 0, 4, 0]
    assert a.tree.digest()[1] == persistent - 4
    # a session without ephemerals, alone and among others
    e = _both(a, b, lambda m: m.session())
    assert run([e], [e]) == [0]
    s, t = born(2, 3, 0)
    e = _both(a, b, lambda m: m.session())
    assert run([s, e, t], [s, e, t]) == [3, 0, 3]
    # 65 sessions, one node each
    sids = born(65, 1, 20)
    a.audit()
    b.audit()
    nodes = sorted(a.node_of[p] for p in names[20:85])
    assert nodes[-1] - nodes[0] < 128          # at most two waves of nodes
    got = run(sids[::-1], sids[::-1])
    assert got == [1] * 65


# ---- 3. watches -------------------------------------------------------------

def test_close_watches(gpu):
    """Four watchers, two of them closing, with data, exist and child
    watches on the closing sessions' nodes and their parents.  The
    survivors' events of one close_sessions equal, as a multiset a watcher,
    the model's and those of expire; expire on the twin; each watcher's come
    from its own slice (close_slots); nothing is addressed to a closer.  A
    watch a closer held on a persistent node does not fire at the next
    write, and a new session bound to the slot inherits nothing."""
    a, b = _twins(gpu, cls=CloseWatchModel, watch_cap=4096)
    par = '/bench/p'
    keep = D0 + '/n000000003'
    wa = [_both(a, b, lambda m, w=w: m.session(w)) for w in range(4)]
    mine = {0: [par + '/a%d' % k for k in range(6)] +
               [D0 + '/ea%d' % k for k in range(3)],
            1: [par + '/b%d' % k for k in range(6)] +
               [D0 + '/eb%d' % k for k in range(3)]}
    for m in (a, b):
        m.serve([create(par)])
        for w in (0, 1):
            m.serve([create(p, b'x', ['EPHEMERAL']) for p in mine[w]],
                    sid=wa[w], wslot=w, audit=False)
        # data, exist and child watches of all four on the closers' nodes
        # and their parents; on a persistent node too
        for w in range(4):
            seen = mine[0][w:w + 4] + mine[1][w + 1:w + 5]
            pk = [wget(p) for p in seen[::2]] + \
                [wexists(p) for p in seen[1::2]] + \
                [wexists(par + '/never%d' % w), wget(keep), wget(par),
                 wexists(D0)]
            m.serve(pk, sid=wa[w], wslot=w, audit=False)
            m.serve([ls(par), ls(D0), ls(mine[1][0])], sid=wa[w], wslot=w,
                    how='list', audit=False)
    # the twin: two expiries, each checked against its model
    got_b = collections.defaultdict(list)
    for w in (0, 1):
        b.expire(wa[w], audit=w == 1)           # (one audit a tree)
        for s, ev in b._exp_sent.items():
            got_b[s] += ev
    sent = a.close([wa[0], wa[1]])
    assert set(sent) == {2, 3}
    for s in (2, 3):
        assert collections.Counter(sent[s]) == collections.Counter(got_b[s])
        kinds = {t for t, _ in sent[s]}
        assert kinds == {'DELETED', 'CHILDREN_CHANGED'}, kinds
    _same(a, b)
    # the closers' watches on what stays are gone: a write of `keep`, a new
    # child of the parents tell the survivors only (the model knows no
    # watcher 0 or 1 any more: any event for them fails the comparison)
    for m in (a, b):
        _, ev = m.serve([set_data(keep, b'new'), create(par + '/later'),
                         create(par + '/never0'), create(par + '/never2')],
                        audit=False)
        assert {e[1] for e in ev} == {2, 3}
    # a new session on a closer's slot inherits nothing, and its own arm
    # works
    for m in (a, b):
        n0 = m.session(0)
        m.serve([wget(par)], sid=n0, wslot=0, audit=False)
        m.serve([set_data(keep, b'newer'), delete(par + '/never0'),
                 set_data(D0, b'd')], audit=False)
        # (the survivors' data watches on the parent are still armed; the
        # closers' are not)
        _, ev = m.serve([set_data(par, b'p')])
        assert sorted((e[1], e[2]) for e in ev) == \
            [(w, 'DATA_CHANGED') for w in (0, 2, 3)]
    _same(a, b)


# ---- 4-6. CLOSE_SESSION frames of a session batch ---------------------------

def close_req():
    return {'opcode': 'CLOSE_SESSION'}


def _watch_tree(gpu, table=False):
    from zkmi.server.engine import GpuServer
    from zkmi.server.sessions import GpuSessionTable
    from zkmi.server.tree import GpuTree
    tree = GpuTree(10, 16, fanout=10, device=gpu, spare=0.0, watch_cap=1024,
                   scratch=1 << 16)
    srv = GpuServer(tree, 256, 1 << 18)
    tab = None
    if table:
        tab = GpuSessionTable(tree, cap=16)
        for k in range(6):
            tab.sid[k] = tab.sid_of(k)
            tab.state[k] = 1
        tab.next.fill_(6)
    return tree, srv, tab


def _sids(tab):
    if tab is not None:
        return [tab.sid_of(k) for k in range(6)]
    return [(1 << 56) | (0x100 + k) for k in range(6)]


def _batch(dev, segs, starts=None):
    """segs: [(session, watcher slot, [request dict or raw frame bytes])]
    -> (rx, its length, the segment table); xids count from 1 a segment."""
    from zkmi.server.engine import SessionSegments
    parts = []
    for _, _, pk in segs:
        b = b''
        for k, p in enumerate(pk):
            if isinstance(p, bytes):
                b += p
            else:
                p['xid'] = 1 + k
                b += _stream([p])
        parts.append(b)
    rx = b''.join(parts)
    cuts = [0] + [int(x) for x in np.cumsum([len(b) for b in parts])]
    tab = SessionSegments(
        torch.tensor(cuts if starts is None else starts, dtype=I64,
                     device=dev),
        torch.tensor([s for s, _, _ in segs], dtype=I64, device=dev),
        torch.tensor([w for _, w, _ in segs], dtype=I32, device=dev))
    return dev_bytes(rx, dev), len(rx), tab


def _call(srv, how, rx, n, tab, **kw):
    if how == 'mixed':
        return srv.serve_sessions_mixed(rx, n, tab, **kw)
    return srv.serve_sessions(rx, n, tab, ordered=how == 'ordered', passes=8,
                              **kw)


def _serve(srv, how, rx, n, tab, **kw):
    """-> [[(frame bytes, xid, err)] a segment], sliced by rep_off."""
    out, total, err, ft = _call(srv, how, rx, n, tab, **kw)
    assert int(err.item()) == 0
    raw = bytes(out[:int(total.item())].cpu().numpy().tobytes())
    off = srv.seg.rep_off.cpu().tolist()
    assert off[0] == 0 and off[-1] == len(raw) and off == sorted(off), off
    reps = []
    for s in range(tab.S):
        part = raw[off[s]:off[s + 1]]
        frames, used, bad = jute.scan_frames(part)
        assert bad < 0 and used == len(part), (s, used, len(part))
        rs = []
        for o, ln in frames:
            xid, _, e = struct.unpack_from('>iqi', part, o)
            rs.append((part[o - 4:o + ln], xid, e))
        reps.append(rs)
    return reps


def _kids(tree, path):
    return tree.children_host(path)


def _zxid(tree):
    return int(tree.counters[_lib.TC_ZXID].item())


def test_three_streams_keep_their_buffers(gpu):
    """One batch that fills all three notification streams — a write to a
    node another segment watches (write-fired), a SET_WATCHES that lists a
    node changed since relZxid 0 (catch-up), a CLOSE_SESSION whose segment
    owns an ephemeral under a directory another segment's list watches
    (close-fired) — served twice with the same ``rx`` shape: the second call
    allocates nothing, every published tensor is where the first left it."""
    tree, srv, _ = _watch_tree(gpu)
    s0, s1, s2 = _sids(None)[:3]
    na, nb, nc = (D0 + '/n%09d' % k for k in (1, 2, 3))
    mine = D0 + '/mine'
    rx, n, sg = _batch(gpu, [(s0, 5, [wget(na)])])
    _serve(srv, 'mixed', rx, n, sg)
    shapes, ptrs = [], []
    # (the data watch a call arms is on the node the next call writes: a
    # watch armed in the write's own batch may be fired by it.  The list's
    # child watch is armed after the batch's writes and before its close
    # pass, whose removal of ``mine`` fires it.)
    for arm, write in ((nb, na), (na, nb)):
        rx, n, sg = _batch(gpu, [
            (s0, 5, [wget(arm), ls(D0)]),
            (s1, 9, [set_data(write, b'w')]),
            (s2, 7, [create(mine, b'm', ['EPHEMERAL']),
                     {'opcode': 'SET_WATCHES', 'relZxid': 0,
                      'events': {'dataChanged': [nc],
                                 'createdOrDestroyed': [],
                                 'childrenChanged': []}},
                     close_req()])])
        reps = _serve(srv, 'mixed', rx, n, sg, resume=True, close=True)
        assert all(e == OK for rs in reps for _, _, e in rs), reps
        shapes.append((n, sg.S))
        streams = ((srv.notif, srv.notif_slots),
                   (srv.resume_notif, srv.resume_slots),
                   (srv.close_notif, srv.close_slots))
        assert all(int(nf[1].item()) > 0 for nf, _ in streams)
        ptrs.append([t.data_ptr() for nf, sl in streams
                     for t in (nf[0],) + tuple(sl)])
        fired, caught, closed = (slot_events(nf, sl) for nf, sl in streams)
        assert ('DATA_CHANGED', write) in fired[5]
        assert caught == {7: [('DATA_CHANGED', nc)]}
        assert closed == {5: [('CHILDREN_CHANGED', D0)]}
        assert _kids(tree, D0).count('mine') == 0
    assert shapes[0] == shapes[1] and ptrs[0] == ptrs[1]
    assert set(srv.watch_stats()) == {
        'lost_arms', 'events_fired', 'events_written', 'encode_err',
        'expiry_dropped', 'resume_dropped', 'resume_err'}
    assert set(srv.resume_stats()) == {
        'events', 'events_written', 'rearmed', 'listed', 'dropped',
        'no_slot', 'encode_err'}
    assert set(srv.close_stats()) == {
        'frames', 'sessions', 'removed', 'events_fired', 'events_written',
        'records_dropped', 'encode_err'}


HOWS = ('sessions', 'ordered', 'mixed')


@pytest.mark.parametrize('how', HOWS)
def test_close_frames_in_batch(gpu, how):
    """Two closing segments and one that stays, with a session table.  The
    closing frames' replies are 20 bytes, err OK, their own xid (on the
    parent commit the keyword does not exist and the answer is
    UNIMPLEMENTED); every reply slice is intact; the closing segments'
    ephemerals are gone after the batch — one created in the batch too —
    while another segment's GET of them in that batch succeeded; the zxid
    counter moved by the frames and the two closes; the closed sessions'
    next batch is answered SESSION_EXPIRED."""
    tree, srv, tab = _watch_tree(gpu, table=True)
    s0, s1, s2 = _sids(tab)[:3]
    e0 = [D0 + '/c0k%d' % k for k in range(3)]
    e1 = [D0 + '/c1k%d' % k for k in range(2)]
    e2 = [D0 + '/c2k%d' % k for k in range(2)]
    rx, n, sg = _batch(gpu, [
        (s0, 0, [create(p, b'0', ['EPHEMERAL']) for p in e0]),
        (s1, 1, [create(p, b'1', ['EPHEMERAL']) for p in e1]),
        (s2, 2, [create(p, b'2', ['EPHEMERAL']) for p in e2])])
    reps = _serve(srv, how, rx, n, sg, table=tab)
    assert all(e == OK for rs in reps for _, _, e in rs)
    static = [D0 + '/n%09d' % k for k in range(10)]
    names = lambda ps: sorted(p.rsplit('/', 1)[1] for p in ps)
    assert _kids(tree, D0) == names(static + e0 + e1 + e2)
    new = D0 + '/c0new'
    # (ordered: the survivor's GET of the node the closer creates in this
    # batch comes after it; unordered batches read what an earlier batch
    # made)
    seen = [new] if how == 'ordered' else []
    base = _zxid(tree)
    segs = [
        (s0, 0, [get(e0[0]), create(new, b'n', ['EPHEMERAL']), close_req(),
                 get(static[0])]),
        (s2, 2, [get(e0[1]), get(e1[0])] + [get(p) for p in seen] +
                [get(e2[0])]),
        (s1, 1, [close_req()])]
    rx, n, sg = _batch(gpu, segs)
    reps = _serve(srv, how, rx, n, sg, table=tab, close=True)
    assert [len(rs) for rs in reps] == [4, 3 + len(seen), 1]
    for s, k in ((0, 2), (2, 0)):
        frame, xid, err = reps[s][k]
        assert len(frame) == 20 and frame[:4] == struct.pack('>i', 16)
        assert (xid, err) == (k + 1, OK), (s, xid, err)
    # every other reply OK, in its own slice, with its own xid: the frame
    # after the CLOSE_SESSION is served, the other segment's GETs of the
    # closers' ephemerals succeeded
    for s, rs in enumerate(reps):
        assert [x for _, x, _ in rs] == list(range(1, len(rs) + 1))
        assert all(e == OK for _, _, e in rs), (s, rs)
    nframes = sum(len(pk) for _, _, pk in segs)
    assert _zxid(tree) == base + nframes + 2
    assert _kids(tree, D0) == names(static + e2)
    st = srv.close_stats()
    assert (st['frames'], st['sessions'], st['removed']) == (2, 2, 6), st
    assert st['records_dropped'] == 0 and st['encode_err'] == 0
    # segment order is stream order: s0's segment came first
    assert srv.close_removed.cpu().tolist() == [4, 2, 0]
    assert srv.session_stats()['expired_segments'] == 0
    # the next batch: the closed sessions are answered SESSION_EXPIRED
    rx, n, sg = _batch(gpu, [(s0, 0, [get(static[0])]),
                             (s2, 2, [get(e2[1])]),
                             (s1, 1, [get(static[1]), close_req()])])
    reps = _serve(srv, how, rx, n, sg, table=tab, close=True)
    assert [[e for _, _, e in rs] for rs in reps] == \
        [[SESSION_EXPIRED], [OK], [SESSION_EXPIRED, SESSION_EXPIRED]]
    assert srv.close_stats()['sessions'] == 0
    assert _kids(tree, D0) == names(static + e2)


@pytest.mark.parametrize('how', ('sessions', 'mixed'))
def test_close_with_resume(gpu, how):
    """resume=True and close=True: the watch a closing segment's
    SET_WATCHES re-arms does not survive the batch (the control, the same
    batch without the CLOSE_SESSION, shows that it was re-armed); the
    survivor's does.  The close pass's events go to the survivor alone."""
    keep = D0 + '/n000000004'
    for closing in (True, False):
        tree, srv, _ = _watch_tree(gpu)
        s0, s1 = _sids(None)[:2]
        mine = D0 + '/mine'
        # (two batches: a watch armed in the create's own batch may be fired
        # by it)
        for segs in ([(s0, 5, [create(mine, b'm', ['EPHEMERAL'])])],
                     [(s1, 9, [{'opcode': 'EXISTS', 'path': mine,
                                'watch': True}])]):
            rx, n, sg = _batch(gpu, segs)
            _serve(srv, how, rx, n, sg)
        rel = _zxid(tree)
        sw = lambda: {'opcode': 'SET_WATCHES', 'relZxid': rel,
                      'events': {'dataChanged': [keep],
                                 'createdOrDestroyed': [],
                                 'childrenChanged': [D0]}}
        rx, n, sg = _batch(gpu, [
            (s0, 5, [sw()] + ([close_req()] if closing else [])),
            (s1, 9, [sw()])])
        reps = _serve(srv, how, rx, n, sg, resume=True, close=True)
        assert all(e == OK for rs in reps for _, _, e in rs)
        assert srv.resume_stats()['rearmed'] == 4
        st = srv.close_stats()
        sent = slot_events(srv.close_notif, srv.close_slots)
        if closing:
            assert (st['frames'], st['removed']) == (1, 1)
            # the survivor's exist watch on the closer's node, its re-armed
            # child watch on the parent; nothing for the closer's slot
            assert {w: sorted(ev) for w, ev in sent.items()} == \
                {9: [('CHILDREN_CHANGED', D0), ('DELETED', mine)]}
            assert st['events_fired'] == st['events_written'] == 2
        else:
            assert (st['frames'], st['removed']) == (0, 0) and not sent
        rx, n, sg = _batch(gpu, [(0, -1, [set_data(keep, b'w'),
                                          create(D0 + '/kid')])])
        _serve(srv, how, rx, n, sg)
        got = slot_events(srv.notif, srv.notif_slots)
        want = {9: [('DATA_CHANGED', keep)]}
        if not closing:
            want = {5: [('DATA_CHANGED', keep), ('CHILDREN_CHANGED', D0)],
                    9: [('DATA_CHANGED', keep), ('CHILDREN_CHANGED', D0)]}
        assert {w: sorted(ev) for w, ev in got.items()} == \
            {w: sorted(ev) for w, ev in want.items()}


@pytest.mark.parametrize('how', HOWS)
def test_close_refusals(gpu, how):
    """What closes nothing: an unsound segment table (the reply stays
    SYSTEMERROR), a dead segment's CLOSE_SESSION (SESSION_EXPIRED), a
    7-byte body (BAD_ARGUMENTS)."""
    tree, srv, tab = _watch_tree(gpu, table=True)
    s0, s1, s2 = _sids(tab)[:3]
    eph = [D0 + '/r%d' % k for k in range(3)]
    rx, n, sg = _batch(gpu, [(s, k, [create(eph[k], b'', ['EPHEMERAL'])])
                             for k, s in enumerate((s0, s1, s2))])
    _serve(srv, how, rx, n, sg, table=tab)
    kids = _kids(tree, D0)
    assert len(kids) == 13

    def nothing(reps, want):
        assert [[e for _, _, e in rs] for rs in reps] == want
        st = srv.close_stats()
        assert (st['frames'], st['sessions'], st['removed']) == (0, 0, 0), st
        assert _kids(tree, D0) == kids
        assert tab.state[:3].cpu().tolist() == [1, 1, 1]

    # an unsound table: starts does not begin at 0
    segs = [(s0, 0, [close_req()]), (s1, 1, [get(eph[1]), close_req()])]
    rx, n, sg = _batch(gpu, segs, starts=[4, 20, 81])
    base = _zxid(tree)
    out, total, err, _ = _call(srv, how, rx, n, sg, table=tab, close=True)
    raw = bytes(out[:int(total.item())].cpu().numpy().tobytes())
    frames, used, bad = jute.scan_frames(raw)
    assert bad < 0 and used == len(raw) and len(frames) == 3
    assert [struct.unpack_from('>iqi', raw, o)[2] for o, _ in frames] == \
        [SYSTEM] * 3
    assert srv.session_stats()['bad'] > 0
    nothing([], [])
    assert _zxid(tree) == base + 3
    # a dead segment: the table does not hold s2 alive
    tab.close(torch.tensor([s2], dtype=I64, device=gpu))
    rx, n, sg = _batch(gpu, [(s0, 0, [get(eph[0])]),
                             (s2, 2, [close_req()])])
    reps = _serve(srv, how, rx, n, sg, table=tab, close=True)
    tab.state[2] = 1                        # (alive again for the next case)
    nothing(reps, [[OK], [SESSION_EXPIRED]])
    # a 7-byte body: no opcode word to read
    short = struct.pack('>i', 7) + struct.pack('>ii', 9, CLOSE_SESSION)[:7]
    rx, n, sg = _batch(gpu, [(s0, 0, [short]), (s1, 1, [get(eph[1])])])
    reps = _serve(srv, how, rx, n, sg, table=tab, close=True)
    nothing(reps, [[BAD_ARGUMENTS], [OK]])
    assert reps[0][0][1] == 0                   # (no xid in 7 bytes)


@pytest.mark.parametrize('how', HOWS)
def test_close_off_is_unchanged(gpu, how):
    """close=False is the call without the keyword, byte for byte: replies
    (CLOSE_SESSION answered UNIMPLEMENTED), slices, notifications and the
    tree."""
    res = []
    for kw in ({}, {'close': False}):
        tree, srv, _ = _watch_tree(gpu)
        s0, s1 = _sids(None)[:2]
        mine = D0 + '/mine'
        rx, n, sg = _batch(gpu, [
            (s0, 5, [create(mine, b'm', ['EPHEMERAL'])]),
            (s1, 9, [{'opcode': 'GET_DATA', 'path': D0 + '/n000000001',
                      'watch': True}])])
        _serve(srv, how, rx, n, sg)
        rx, n, sg = _batch(gpu, [
            (s0, 5, [get(mine), close_req(),
                     set_data(D0 + '/n000000001', b'z')]),
            (s1, 9, [close_req(), get(mine)])])
        reps = _serve(srv, how, rx, n, sg, **kw)
        assert [[e for _, _, e in rs] for rs in reps] == \
            [[OK, UNIMPLEMENTED, OK], [UNIMPLEMENTED, OK]]
        assert srv.close_notif is None and srv._cl is None
        buf, total, slots, count = srv.notif
        res.append((reps, srv.seg.rep_off.cpu().tolist(),
                    bytes(buf[:int(total.item())].cpu().numpy().tobytes()),
                    [x.cpu().tolist() for x in srv.notif_slots],
                    tree.digest(), _zxid(tree), _kids(tree, D0)))
    assert res[0] == res[1]
    assert 'mine' in res[0][6] and len(res[0][2]) > 0


# ---- 7. the op's checks -----------------------------------------------------

def test_close_op_checks(gpu):
    """A wrong dtype, device, length or a non-contiguous tensor to
    torch.ops.zkmi.close_sessions raises before anything is launched."""
    from zkmi.server.tree import GpuTree
    tree = GpuTree(10, 16, fanout=10, device=gpu, spare=0.0)
    cap, S = 64, 4
    ws = torch.empty(_lib.close_workspace(cap, S, tree.cap), dtype=I64,
                     device=gpu)
    sids = torch.tensor([(1 << 56) | 5, (1 << 56) | 6], dtype=I64, device=gpu)
    wsl = torch.tensor([-1, 3], dtype=I32, device=gpu)
    removed = torch.zeros(2, dtype=I64, device=gpu)
    stats = torch.zeros(8, dtype=I64, device=gpu)
    base = _zxid(tree)
    ok = dict(sids=sids, wslots=wsl, ws=ws, removed=removed, stats=stats)

    def call(**kw):
        a = dict(ok, **kw)
        _lib.close_sessions(tree.tensors, a['sids'], a['wslots'], S, cap,
                            a['ws'], a['removed'], a['stats'])

    call()
    assert _zxid(tree) == base + 2 and removed.cpu().tolist() == [0, 0]
    wide = torch.zeros(4, dtype=I64, device=gpu)
    bad = [dict(sids=sids.to(I32)), dict(wslots=wsl.to(I64)),
           dict(removed=removed.to(I32)), dict(stats=stats.to(I32)),
           dict(ws=ws.view(U8)),
           dict(sids=sids.cpu()), dict(wslots=wsl.cpu()),
           dict(removed=removed.cpu()), dict(ws=ws.cpu()),
           dict(wslots=wsl[:1]), dict(removed=removed[:1]),
           dict(stats=stats[:7]), dict(ws=ws[:-1]),
           dict(sids=torch.zeros(S + 1, dtype=I64, device=gpu)),
           dict(sids=wide[::2]),
           dict(wslots=torch.zeros(4, dtype=I32, device=gpu)[::2]),
           dict(removed=wide[::2])]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    assert _zxid(tree) == base + 2
    with pytest.raises(RuntimeError):
        _lib.close_workspace(cap, 0, tree.cap)
