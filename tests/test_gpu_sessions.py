"""GpuServer.serve_sessions: one batch carrying the whole frames of many
connections, a session and a watcher slot per segment
(csrc/kernels/tree_sess.hip, the serve's MS instances in tree.hip; the rule:
csrc/kernels/zk_sess.h).

The driver below puts tests/treemodel.py and tests/watchmodel.py under a
multi-session batch: the requests of every segment carry xids from 1 (they
collide across segments), request i of the stream is applied to the model
with its own segment's session, the replies are compared segment by segment
through ``rep_off`` and the notifications watcher by watcher through
``slot_off``.  time.time is frozen so two trees' Stats compare exactly."""

import collections
import random
import time

import numpy as np
import pytest
import torch

from treemodel import create, delete, dev_bytes, exists, get, set_data
from treemodel import _stream
from watchmodel import (WatchModel, check_events, decode_notifications, ls,
                        wexists, wget)

from zkmi import jute
from zkmi.ops import _lib

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000.0
FANOUT = 100
NLEAF = 2000
NDIR = NLEAF // FANOUT
POOL_DIRS = 8               # dirs 0..7: plain creates / sets / deletes / reads
SLOTS = (0, 1, 31, 62, 63)
I64, I32 = torch.int64, torch.int32


@pytest.fixture(autouse=True)
def _frozen_time(monkeypatch):
    monkeypatch.setattr(time, 'time', lambda: NOW)


def leaf(i):
    return '/bench/d%06d/n%09d' % (i // FANOUT, i)


def dirp(d):
    return '/bench/d%06d' % d


def _segments(dev, starts, sessions, wslots):
    from zkmi.server.engine import SessionSegments
    return SessionSegments(
        torch.tensor(list(starts), dtype=I64, device=dev),
        torch.tensor(list(sessions), dtype=I64, device=dev),
        torch.tensor(list(wslots), dtype=I32, device=dev))


def _tree(gpu, **kw):
    from zkmi.server.tree import GpuTree
    return GpuTree(NLEAF, 16, fanout=FANOUT, device=gpu, seed=3,
                   watch_cap=4096, scratch=1 << 20, **kw)


def _raw(buf, total):
    return bytes(buf[:int(total)].cpu().numpy().tobytes())


# ---- the multi-session driver -----------------------------------------------

class SessModel(WatchModel):
    """:class:`watchmodel.WatchModel` driven by session batches.  A batch is
    ``segs``: [(session, watcher slot, [request, ...]), ...]."""

    def session_as(self, sid, wslot=-1):
        """A model session with the id ``sid`` (a session table's)."""
        old = self.session(wslot)
        s = self.db.sessions.pop(old)
        s.sid = sid
        self.db.sessions[sid] = s
        if wslot >= 0:
            self.slot_sid[wslot] = sid
        return sid

    def build(self, segs, starts=None):
        flat = []
        for s, (_, _, pk) in enumerate(segs):
            for k, p in enumerate(pk):
                p['xid'] = 1 + k
                flat.append((s, p))
        parts = [_stream(pk) for _, _, pk in segs]
        rx = b''.join(parts)
        cuts = [0] + [int(x) for x in np.cumsum([len(b) for b in parts])]
        tab = _segments(self.dev, cuts if starts is None else starts,
                        [sid for sid, _, _ in segs],
                        [w for _, w, _ in segs])
        return flat, rx, cuts, tab

    def slot_events(self):
        """{slot: [(type, path)]} of the server's slot-major notification
        stream, each slot's decoded from its own slice of the bytes."""
        srv = self.srv
        buf, total, slots, count = srv.notif
        n = int(count.item())
        raw = _raw(buf, total.item())
        ev = decode_notifications(buf, total.item(), n)
        sl = slots[:n].cpu().tolist()
        first, off = (x.cpu().tolist() for x in srv.notif_slots)
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

    def serve_sessions(self, segs, ordered=False, passes=4, table=None,
                       dead=(), starts=None, refused=False, audit=True,
                       terminate=False):
        """One session batch on the server and on the model.  ``dead``: the
        segments whose session ``table`` does not hold alive; ``refused``
        (with a ``starts`` that is unsound): the whole batch.  Returns
        ([replies of segment s], model events)."""
        srv = self.srv
        flat, rx, cuts, tab = self.build(segs, starts)
        if ordered:
            self.zxids_ok = False
        zxids = self.zxids_ok
        base = self.counter(_lib.TC_ZXID)
        out, total, err, ft = srv.serve_sessions(
            dev_bytes(rx, self.dev), len(rx), tab, ordered=ordered,
            passes=passes, table=table, terminate=terminate)
        assert int(err.item()) == 0
        assert int(ft.count.item()) == len(flat)
        raw = _raw(out, total.item())
        if terminate:
            assert _raw(out, total.item() + 4)[-4:] == b'\xff' * 4
        st = srv.session_stats()
        assert self.counter(_lib.TC_ZXID) == base + len(flat)
        # ---- the replies, a slice a segment
        reps = []
        if refused:
            assert st['bad'] > 0
            frames, used, bad = jute.scan_frames(raw)
            assert bad < 0 and used == len(raw) and len(frames) == len(flat)
            for (o, ln), (_, p) in zip(frames, flat):
                r = jute.decode_response(raw[o:o + ln],
                                         {p['xid']: p['opcode']})
                assert (r['xid'], r['err']) == (p['xid'], 'SYSTEM_ERROR'), r
            keys = None
        else:
            assert st['bad'] == 0 and st['first_bad_segment'] == -1, st
            assert st['expired_segments'] == len(set(dead)), st
            f_seg = srv.seg.f_seg[:len(flat)].cpu().tolist()
            assert f_seg == [s for s, _ in flat]
            first = srv.seg.first.cpu().tolist()
            want_first = [0] + [int(x) for x in
                                np.cumsum([len(pk) for _, _, pk in segs])]
            assert first == want_first
            off = srv.seg.rep_off.cpu().tolist()
            assert off[0] == 0 and off[-1] == len(raw), (off[0], off[-1])
            assert off == sorted(off)
            rec = srv.last_rec_off[:len(flat)].cpu().tolist()
            for s, (_, _, pk) in enumerate(segs):
                part = raw[off[s]:off[s + 1]]
                if pk:
                    assert off[s] == rec[want_first[s]]
                frames, used, bad = jute.scan_frames(part)
                assert bad < 0 and used == len(part), (s, used, len(part))
                assert len(frames) == len(pk), (s, len(frames), len(pk))
                xmap = {p['xid']: p['opcode'] for p in pk}
                rs = [jute.decode_response(part[o:o + ln], xmap)
                      for o, ln in frames]
                assert [r['xid'] for r in rs] == list(range(1, len(pk) + 1))
                reps.append(rs)
        # ---- the model, request by request in stream order
        want, writes, keys = [], [], []
        for i, (s, p) in enumerate(flat):
            sid = segs[s][0]
            if refused:
                continue
            if s in dead:
                keys.append((p['xid'], 'SESSION_EXPIRED'))
                continue
            lens = self._lens()
            k = self._apply(p, sid or None, base + i + 1, zxids)
            keys.append(k)
            if k[1] == 'OK' and p['opcode'] in ('CREATE', 'DELETE'):
                writes.append((i, k[2] if p['opcode'] == 'CREATE'
                               else p['path']))
            self._since(lens, i, want)
        if not refused:
            got = [r for rs in reps for r in rs]
            for i, (r, w) in enumerate(zip(got, keys)):
                g = self._reply_key(r, zxids)
                assert g == w, 'request %d (segment %d) %r: got %r, want %r' \
                    % (i, flat[i][0], {k: v for k, v in flat[i][1].items()
                                       if k != 'acl'}, g, w)
                if zxids and flat[i][0] not in dead:
                    wr = flat[i][1]['opcode'] in ('CREATE', 'SET_DATA',
                                                  'DELETE')
                    assert r['zxid'] == (base + i + 1 if wr else base), (i, r)
        # ---- the notifications, a slice a watcher
        sent = self.slot_events()
        ev_total = srv.ev_total.cpu().tolist()
        assert ev_total == [len(want), len(want)], (ev_total, len(want))
        ws = srv.watch_stats()
        assert ws['encode_err'] == 0 and ws['lost_arms'] == 0, ws
        assert ws['events_fired'] == ws['events_written'] == len(want)
        bad = check_events(sent, want, ordered, writes)
        assert bad is None, bad
        self.batches += 1
        if audit:
            self.audit(zxids=self.zxids_ok)
        return reps, want


def _model(gpu, frames=1024):
    from zkmi.server.engine import GpuServer
    tree = _tree(gpu)
    srv = GpuServer(tree, frames, 1 << 21)
    return SessModel(tree, srv, gpu)


def _data(rng, hi=60):
    return bytes(rng.getrandbits(8) for _ in range(rng.randint(0, hi)))


def _pool():
    out = []
    for d in range(POOL_DIRS):
        out += [leaf(FANOUT * d + k) for k in range(FANOUT)]
        out += ['%s/m%s%02d' % (dirp(d), 'x' * (j % 16), j)
                for j in range(40)]
    return out


def _sizes(rng, n, empties=True):
    """Segment sizes (1..40 frames, a few empty segments) adding up to n,
    with boundaries on, just before and just after frames 64 and 256."""
    forced = [f for f in (63, 64, 65, 255, 256, 257) if f < n]
    sizes, pos = [], 0
    while pos < n:
        nxt = min(n, pos + rng.randint(1, 40))
        cut = [f for f in forced if pos < f < nxt]
        if cut:
            nxt = cut[0]
        if empties and rng.random() < 0.15:
            sizes.append(0)
        sizes.append(nxt - pos)
        pos = nxt
    return sizes


def _request(m, rng, path):
    """One request on ``path`` of the pool by the model's present state."""
    node = m.db.nodes.get(path)
    r = rng.random()
    if node is None:
        if r < 0.55:
            return create(path, _data(rng),
                          ['EPHEMERAL'] if rng.random() < 0.5 else [])
        if r < 0.7:
            return get(path)
        if r < 0.85:
            return exists(path)
        if r < 0.93:
            return delete(path)
        return set_data(path, b'x')
    ver = node.stat.version
    if r < 0.3:
        v = rng.choice([-1, ver, ver, ver + 1])
        return set_data(path, _data(rng), v)
    if r < 0.45:
        return delete(path, rng.choice([-1, ver, ver + 3]))
    if r < 0.7:
        return get(path)
    if r < 0.9:
        return exists(path)
    return create(path, b'dup')


def _batch(m, rng, sids, n, empties=True):
    """A conflict-free batch of n frames in segments: every pool path at
    most once, no directory read, SEQUENTIAL creates (their parents get
    nothing else) under the segment's own parent."""
    paths = rng.sample(_pool(), n)
    segs, k = [], 0
    for s, size in enumerate(_sizes(rng, n, empties)):
        sid = rng.choice(sids)
        pk = []
        for path in paths[k:k + size]:
            if rng.random() < 0.12:
                fl = ['SEQUENTIAL'] + (['EPHEMERAL'] if rng.random() < 0.5
                                       else [])
                pk.append(create('%s/q-' % dirp(POOL_DIRS + s %
                                                (NDIR - POOL_DIRS)),
                                 _data(rng, 20), fl))
            else:
                pk.append(_request(m, rng, path))
        k += size
        if not sid:                 # no session, no EPHEMERAL
            for p in pk:
                if 'flags' in p:
                    p['flags'] = [f for f in p['flags'] if f != 'EPHEMERAL']
        segs.append((sid, -1, pk))
    assert k == n
    return segs


# ---- 1. against the model, unordered ----------------------------------------

def test_model_unordered(gpu):
    m = _model(gpu)
    rng = random.Random(11)
    sids = [m.session() for _ in range(6)] + [0]
    owners = collections.Counter()
    for n in (1, 63, 64, 65, 255, 256, 257, 600):
        segs = _batch(m, rng, sids, n)
        cuts = set(np.cumsum([len(pk) for _, _, pk in segs]).tolist())
        for f in (63, 64, 65, 255, 256, 257):
            assert f >= n or f in cuts
        reps, _ = m.serve_sessions(segs)
        # every EPHEMERAL's owner is its segment's session
        for (sid, _, pk), rs in zip(segs, reps):
            for p, r in zip(pk, rs):
                if p['opcode'] == 'CREATE' and r['err'] == 'OK' and \
                        'EPHEMERAL' in p['flags']:
                    node = m.db.nodes[r['path']]
                    assert node.stat.ephemeralOwner == (sid or 0)
                    owners[sid] += 1
    assert len([s for s in owners if s]) >= 4, owners
    # an expiry removes that session's nodes only (the audit reads the rest)
    for sid in sids[:3]:
        mine = len(m.db.sessions[sid].ephemerals)
        removed, _ = m.expire(sid)
        assert removed == mine > 0
    # and the others' are still there for a later batch
    left = [p for s in sids[3:6] for p in m.db.sessions[s].ephemerals]
    assert left
    m.serve_sessions([(sids[3], -1, [get(p) for p in left[:30]]),
                      (sids[4], -1, [exists(p) for p in left[30:60]])])


# ---- 2. against the model, ordered ------------------------------------------

def _chains(m, rng, nchains, passes):
    """Same-path chains of at most ``passes`` requests, merged at random
    (each chain's order kept)."""
    pool = rng.sample(_pool(), nchains)
    chains = []
    for path in pool:
        there = path in m.db.nodes
        ops = []
        for _ in range(rng.randint(1, passes)):
            r = rng.random()
            if not there:
                if r < 0.7:
                    ops.append(create(path, _data(rng),
                                      ['EPHEMERAL'] if rng.random() < 0.4
                                      else []))
                    there = True
                else:
                    ops.append(rng.choice([get, exists])(path))
            elif r < 0.35:
                ops.append(set_data(path, _data(rng)))
            elif r < 0.5:
                ops.append(delete(path))
                there = False
            else:
                ops.append(rng.choice([get, exists])(path))
        chains.append(ops)
    flat = []
    live = [c for c in chains if c]
    while live:
        c = rng.choice(live)
        flat.append(c.pop(0))
        if not c:
            live.remove(c)
    return flat


def test_model_ordered(gpu):
    m = _model(gpu)
    rng = random.Random(12)
    sids = [m.session() for _ in range(5)]
    for n_chains in (3, 40, 150):
        flat = _chains(m, rng, n_chains, 4)
        segs, k = [], 0
        for size in _sizes(rng, len(flat)):
            segs.append((rng.choice(sids), -1, flat[k:k + size]))
            k += size
        # chains do cross segments
        where = collections.defaultdict(set)
        for s, (_, _, pk) in enumerate(segs):
            for p in pk:
                where[p['path']].add(s)
        if n_chains >= 40:
            assert sum(len(v) > 1 for v in where.values()) >= 10
        m.serve_sessions(segs, ordered=True, passes=4)
        assert m.srv.order_stats()[0] < 4        # no rank was refused
    m.expire(sids[0])


# ---- 3. differential: one session batch against a serve a segment -----------

def test_differential(gpu):
    from zkmi.server.engine import GpuServer
    mx = _model(gpu)
    ty = _tree(gpu)
    sy = GpuServer(ty, 1024, 1 << 21)
    rng = random.Random(13)
    sids = [mx.session(w) for w in (0, 63)] + [mx.session() for _ in range(3)]
    slot = {sids[0]: 0, sids[1]: 63}
    assert mx.tree.digest()[:2] == ty.digest()[:2]
    # (the model's audits are reads, and reads consume zxids: Y starts where
    # X stands, and X runs its batches without an audit in between)
    ty.counters[_lib.TC_ZXID] = mx.counter(_lib.TC_ZXID)
    for n in (65, 300):
        segs = [(sid, slot.get(sid, -1), pk)
                for sid, _, pk in _batch(mx, rng, sids, n)]
        flat, rx, cuts, _ = mx.build(segs)
        by = mx.counter(_lib.TC_ZXID)
        assert int(ty.counters[_lib.TC_ZXID].item()) == by
        repx, _ = mx.serve_sessions(segs, audit=False)
        rawx = _raw(mx.srv.out, mx.srv.result[1].item())
        offx = mx.srv.seg.rep_off.cpu().tolist()
        for s, (sid, w, pk) in enumerate(segs):
            if not pk:
                continue
            part = rx[cuts[s]:cuts[s + 1]]
            out, total, err, _ = sy.serve(dev_bytes(part, gpu), len(part),
                                          session=sid, wslot=w)
            assert int(err.item()) == 0
            rawy = _raw(out, total.item())
            x = rawx[offx[s]:offx[s + 1]]
            assert len(x) == len(rawy)
            frames, _, _ = jute.scan_frames(rawy)
            assert len(frames) == len(pk)
            for (o, ln), p in zip(frames, pk):
                fx, fy = x[o - 4:o + ln], rawy[o - 4:o + ln]
                if p['opcode'] in ('GET_DATA', 'EXISTS'):
                    # a read's header zxid is its batch's base: X's batch
                    # starts earlier than Y's serve of this segment
                    zx = int.from_bytes(fx[8:16], 'big')
                    zy = int.from_bytes(fy[8:16], 'big')
                    assert zx == by and zy == by + len(
                        [1 for t, _ in flat if t < s])
                    fx, fy = fx[:8] + fx[16:], fy[:8] + fy[16:]
                assert fx == fy, (s, p['opcode'], p['path'])
        assert int(ty.counters[_lib.TC_ZXID].item()) == \
            mx.counter(_lib.TC_ZXID)
        assert mx.tree.digest()[:2] == ty.digest()[:2]
    mx.audit()


# ---- 4. slices --------------------------------------------------------------

def test_slices(gpu):
    m = _model(gpu)
    a, b = m.session(), m.session()
    rd = [get(leaf(k)) for k in range(900, 960)]
    # S = 1; empty segments first, last, three in a row; S above the frames
    m.serve_sessions([(a, -1, rd[:7])], audit=False)
    m.serve_sessions([(a, -1, []), (b, -1, rd[:3]), (a, -1, []), (a, -1, []),
                      (b, -1, []), (a, -1, rd[3:5]), (b, -1, [])],
                     audit=False)
    off = m.srv.seg.rep_off.cpu().tolist()
    assert off[0] == off[1] == 0 and off[2] == off[3] == off[4] == off[5]
    assert off[6] == off[7]
    m.serve_sessions([(a, -1, [])] * 40 + [(b, -1, rd[:2])] +
                     [(a, -1, [])] * 40, audit=False)
    # nothing at all
    m.serve_sessions([(a, -1, []), (b, -1, [])], audit=False)
    assert m.srv.seg.rep_off.cpu().tolist() == [0, 0, 0]
    # with the terminator behind the stream, and a large table
    m.serve_sessions([(a, -1, rd[:9]), (b, -1, rd[9:12])], terminate=True,
                     audit=False)
    m.serve_sessions([(a if k % 2 else b, -1, rd[k % 50:k % 50 + 1])
                      for k in range(1000)], audit=False)
    # a table of 100 000 entries, all but three empty
    segs = [(a, -1, [])] * 100_000
    segs[0] = (a, -1, rd[:1])
    segs[70_000] = (b, -1, rd[1:4])
    segs[99_999] = (a, -1, rd[4:6])
    m.serve_sessions(segs)


# ---- 5. watches -------------------------------------------------------------

def _arm_and_fire(gpu, ordered):
    m = _model(gpu)
    w = {s: m.session(s) for s in SLOTS}
    plain = [m.session() for _ in range(2)]
    lv = [leaf(k) for k in range(POOL_DIRS * FANOUT, POOL_DIRS * FANOUT + 400)]
    miss = ['%s/w%02d' % (dirp(9), j) for j in range(10)]
    kw = {'ordered': ordered}
    # child watches come through serve_list, a session each
    for s in SLOTS:
        m.serve([ls(dirp(9)), ls(dirp(10))], sid=w[s], wslot=s, how='list')
    # arm data and exists watches in a session batch, beside unrelated writes
    segs = []
    for j, s in enumerate(SLOTS):
        segs.append((w[s], s, [wget(lv[10 * j + k]) for k in range(4)] +
                     [wexists(miss[j]), wexists(miss[5 + j], False)]))
        segs.append((plain[j % 2], -1,
                     [set_data(lv[300 + 3 * j + k], b'u') for k in range(3)]))
    _, ev = m.serve_sessions(segs, **kw)
    assert ev == []                               # 0 events
    # exactly one event: slot 31's first leaf
    _, ev = m.serve_sessions([(plain[0], -1, [get(lv[399])]),
                              (plain[1], -1, [set_data(lv[20], b'one')])],
                             **kw)
    assert [(e[1], e[2]) for e in ev] == [(31, 'DATA_CHANGED')]
    # the writers: segments without a slot, and a watcher's own segment;
    # slots 0, 1 and 62 have no segment in this batch
    segs = [
        (plain[0], -1, [set_data(lv[0], b'a'), delete(lv[10]),
                        create(miss[0], b'n'), set_data(lv[301], b'v')]),
        (w[63], 63, [set_data(lv[30], b'b'), set_data(lv[40], b'c'),
                     create(miss[3], b'n', ['EPHEMERAL'])]),
        (plain[1], -1, [delete(leaf(10 * FANOUT + 5)), set_data(lv[41], b'd'),
                        create(miss[4], b'n'), get(lv[398])]),
    ]
    _, ev = m.serve_sessions(segs, **kw)
    got = collections.Counter((e[1], e[2]) for e in ev)
    # every slot hears of the children of d9 and d10 once each
    for s in SLOTS:
        assert got[(s, 'CHILDREN_CHANGED')] == 2, (s, got)
    assert got[(0, 'DATA_CHANGED')] == 1 and got[(1, 'DELETED')] == 1
    assert got[(0, 'CREATED')] == 1 and got[(62, 'CREATED')] == 1
    assert got[(63, 'DATA_CHANGED')] == 2 and got[(63, 'CREATED')] == 1
    # what was not fired is still armed: a later batch fires it
    _, ev = m.serve_sessions([(0, -1, [set_data(lv[1], b'e'),
                                       set_data(lv[31], b'f')])], **kw)
    assert sorted((e[1], e[2]) for e in ev) == [(0, 'DATA_CHANGED'),
                                               (62, 'DATA_CHANGED')]
    return m, w, lv


@pytest.mark.parametrize('ordered', [False, True])
def test_watches(gpu, ordered):
    _arm_and_fire(gpu, ordered)


@pytest.mark.parametrize('ordered', [False, True])
def test_watches_many_events(gpu, ordered):
    """More than 256 events (a block boundary of the grouping): all to one
    slot, and spread over the 64 slots."""
    m = _model(gpu)
    kw = {'ordered': ordered}
    lv = [leaf(k) for k in range(1000, 1000 + 64 * 5)]
    one = m.session(63)
    m.serve_sessions([(one, 63, [wget(p) for p in lv[:150]]),
                      (one, 63, [wexists(p) for p in lv[150:300]])], **kw)
    _, ev = m.serve_sessions([(0, -1, [set_data(p, b'1') for p in lv[:100]]),
                              (0, -1, [delete(p) for p in lv[100:300]])],
                             **kw)
    assert len(ev) == 300 and {e[1] for e in ev} == {63}
    m.expire(one)
    sid = {s: m.session(s) for s in range(64)}
    lv = [leaf(k) for k in range(1400, 1400 + 64 * 5)]
    m.serve_sessions([(sid[s], s, [wget(p) for p in lv[5 * s:5 * s + 3]] +
                       [wexists(p) for p in lv[5 * s + 3:5 * s + 5]])
                      for s in range(64)], **kw)
    # the writers interleave the slots: slot-major order is the grouping's
    order = [set_data(lv[5 * s + k], b'2') if k < 4 else delete(lv[5 * s + k])
             for k in range(5) for s in range(64)]
    segs = [(0, -1, order[:200]), (sid[7], 7, order[200:])]
    _, ev = m.serve_sessions(segs, **kw)
    assert len(ev) == 320
    assert collections.Counter(e[2] for e in ev) == \
        collections.Counter({'DATA_CHANGED': 256, 'DELETED': 64})
    assert collections.Counter(e[1] for e in ev) == \
        collections.Counter({s: 5 for s in range(64)})
    # (the driver read watch_stats() before its audit: nothing lost)
    assert m.tree.watch_census()[2] == 0


# ---- 6. torn and bad tables -------------------------------------------------

def test_bad_tables(gpu):
    m = _model(gpu)
    a, b, c = m.session(0), m.session(), m.session()
    la, lb, lc = leaf(1200), leaf(1201), leaf(1202)
    gone = '%s/gone' % dirp(12)
    seqp = dirp(13)
    # armed before: slot 0 watches la's data and the missing `gone`
    m.serve_sessions([(a, 0, [wget(la), wexists(gone)]),
                      (b, -1, [create('%s/s-' % seqp, b'', ['SEQUENTIAL'])])])

    def refused_batch():
        return [(a, 0, [wget(lc), set_data(lb, b'no')]),
                (b, -1, [set_data(la, b'no'), create(gone, b'no'),
                         create('%s/s-' % seqp, b'no', ['SEQUENTIAL']),
                         create('%s/s-' % seqp, b'no',
                                ['SEQUENTIAL', 'EPHEMERAL'])]),
                (c, -1, [delete(leaf(1203)), get(leaf(1204)),
                         create('%s/s-' % dirp(14), b'no', ['SEQUENTIAL'])])]

    _, _, cuts, _ = m.build(refused_batch())
    cases = [
        # a boundary moved into a frame's length word, and into its body
        ([0, cuts[1] + 2, cuts[2], cuts[3]], 1, 0),
        ([0, cuts[1], cuts[2] - 3, cuts[3]], 1, 1),
        # starts[0] = 4: frame 0 has no segment, and the table's own fault
        ([4, cuts[1], cuts[2], cuts[3]], 2, 0),
        # a descending pair
        ([0, cuts[2], cuts[1], cuts[3]], None, None),
    ]
    for starts, nbad, first_bad in cases:
        dig = m.tree.digest()
        census = m.tree.watch_census()
        m.serve_sessions(refused_batch(), starts=starts, refused=True)
        st = m.srv.session_stats()
        if nbad is None:
            assert st['bad'] >= 1 and 0 <= st['first_bad_segment'] <= 1, st
        else:
            assert (st['bad'], st['first_bad_segment']) == (nbad, first_bad)
        assert m.tree.digest() == dig
        assert m.tree.watch_census() == census
        assert m.srv.ev_total.cpu().tolist() == [0, 0]
    # the parents of the refused SEQUENTIAL creates: numChildren and cversion
    # as the model has them (the audit above read them too)
    reps, _ = m.serve_sessions([(c, -1, [exists(seqp), exists(dirp(14))])])
    for r, p in zip(reps[0], (seqp, dirp(14))):
        st = m.db.nodes[p].stat
        assert (r['stat'].numChildren, r['stat'].cversion) == \
            (st.numChildren, st.cversion)
    # a sound batch: the same requests are served, and what was armed before
    # the refused ones fires now — lc was never armed
    _, ev = m.serve_sessions([(b, -1, [set_data(la, b'yes'),
                                       create(gone, b'yes'),
                                       set_data(lc, b'yes')])])
    assert sorted((e[1], e[2], e[3]) for e in ev) == \
        sorted([(0, 'DATA_CHANGED', la), (0, 'CREATED', gone)])
    m.serve_sessions(refused_batch())


# ---- 7. the session table ---------------------------------------------------

def test_session_table(gpu):
    from zkmi.server.sessions import GpuSessionTable
    m = _model(gpu)
    tab = GpuSessionTable(m.tree, cap=64)
    sid = [tab.sid_of(k) for k in range(5)]
    # three live sessions, one closed, one never allocated
    for k in range(4):
        tab.sid[k] = sid[k]
        tab.state[k] = 1
    tab.next.fill_(4)
    tab.close(torch.tensor([sid[3]], dtype=I64, device=gpu))
    live = [m.session_as(s, w) for s, w in zip(sid[:3], (0, 63, -1))]
    rng = random.Random(17)
    lw = leaf(1500)
    m.serve_sessions([(live[0], 0, [wget(lw)])], table=tab)
    for n in (80, 300):
        segs = _batch(m, rng, live + [0], n, empties=False)
        # every fourth segment is a dead session's; its requests would fire,
        # arm, create and delete if they were served
        dead = set()
        for s in range(1, len(segs), 4):
            k = len(dead)
            segs[s] = (sid[3 + k % 2], 1, [
                set_data(lw, b'dead'), wget(leaf(1501 + k)),
                create('%s/dead%d' % (dirp(15), k), b'', ['EPHEMERAL']),
                delete(leaf(1600 + k))])
            dead.add(s)
        assert dead
        reps, ev = m.serve_sessions(segs, table=tab, dead=dead)
        assert ev == []
        for s in dead:
            assert [r['err'] for r in reps[s]] == ['SESSION_EXPIRED'] * 4
        assert m.srv.session_stats()['expired_segments'] == len(dead)
    # the dead segments armed and spent nothing: lw's watch is still slot 0's
    _, ev = m.serve_sessions([(live[1], 63, [set_data(lw, b'live'),
                                             set_data(leaf(1501), b'x')])],
                             table=tab)
    assert [(e[1], e[2]) for e in ev] == [(0, 'DATA_CHANGED')]
    # without a table every segment is served
    m.serve_sessions([(live[2], -1, [get(lw)]), (0, -1, [exists(lw)])])


# ---- 8. the interface -------------------------------------------------------

def test_interface_refusals(gpu):
    from zkmi.server.engine import GpuServer, SessionSegments
    from zkmi.server.tree import GpuTree
    tree = _tree(gpu)
    rx = dev_bytes(_stream([dict(get(leaf(1)), xid=1)]), gpu)
    segs = _segments(gpu, [0, rx.numel()], [0], [-1])
    ro = GpuServer(tree, 64, 1 << 16)
    ro.read_only = True
    with pytest.raises(ValueError):
        ro.serve_sessions(rx, rx.numel(), segs)
    plain = GpuTree(200, 16, fanout=FANOUT, device=gpu, seed=3)
    fr = GpuServer(plain, 64, 1 << 16, seq_order=False, fused_rows=True)
    with pytest.raises(ValueError):
        fr.serve_sessions(rx, rx.numel(), segs)
    with pytest.raises(ValueError):
        SessionSegments(segs.starts, segs.sessions, segs.wslots.repeat(2))
    with pytest.raises(ValueError):
        SessionSegments(segs.starts[:1], segs.sessions, segs.wslots)
    with pytest.raises(TypeError):
        GpuServer(tree, 64, 1 << 16).serve_sessions(rx, rx.numel(), None)


def test_wslots_out_of_range_arm_nothing(gpu):
    """wt_arm's rule (zk_tree.h): a watcher slot below 0 or above 63 arms
    nothing."""
    from zkmi.server.engine import GpuServer
    tree = _tree(gpu)
    srv = GpuServer(tree, 64, 1 << 16)
    census = tree.watch_census()
    parts = [_stream([dict(wget(leaf(5)), xid=1), dict(wexists(leaf(6)),
                                                      xid=2)]),
             _stream([dict(wget(leaf(7)), xid=1)]),
             _stream([dict(wexists('/bench/none'), xid=1)])]
    cuts = [0] + np.cumsum([len(p) for p in parts]).tolist()
    rx = dev_bytes(b''.join(parts), gpu)
    out, total, err, ft = srv.serve_sessions(
        rx, rx.numel(), _segments(gpu, cuts, [0, 0, 0], [64, -5, 1 << 20]))
    assert int(err.item()) == 0 and int(ft.count.item()) == 4
    assert srv.session_stats() == {'bad': 0, 'first_bad_segment': -1,
                                   'expired_segments': 0}
    assert tree.watch_census() == census
    assert srv.watch_stats()['lost_arms'] == 0
    w = _stream([dict(set_data(leaf(k), b'w'), xid=k) for k in (5, 6, 7)])
    rx = dev_bytes(w, gpu)
    srv.serve_sessions(rx, rx.numel(), _segments(gpu, [0, len(w)], [0], [0]))
    assert srv.ev_total.cpu().tolist() == [0, 0]
    assert srv.notif_slots[1].cpu().tolist() == [0] * 65


def test_ops_check_their_tensors(gpu):
    L = _lib.lib()
    S, cap = 3, 16
    z64 = lambda n: torch.zeros(n, dtype=I64, device=gpu)     # noqa: E731
    z32 = lambda n: torch.zeros(n, dtype=I32, device=gpu)     # noqa: E731
    good = dict(frame_off=z64(cap), frame_len=z32(cap), count=z64(1),
                starts=z64(S + 1), sessions=z64(S), f_seg=z32(cap),
                first=z64(S + 1), seg_state=z32(S), bad=z64(2))

    def assign(**kw):
        a = dict(good, **kw)
        _lib.sess_assign(a['frame_off'], a['frame_len'], a['count'], cap,
                         a['starts'], a['sessions'], a['f_seg'], a['first'],
                         a['seg_state'], a['bad'])

    assign()
    for name, wrong in (('starts', z64(S)), ('starts', z64(S + 2)),
                        ('starts', z32(S + 1)), ('sessions', z32(S)),
                        ('f_seg', z32(cap - 1)), ('f_seg', z64(cap)),
                        ('first', z64(S)), ('seg_state', z32(S - 1)),
                        ('bad', z64(1)), ('frame_len', z64(cap)),
                        ('frame_off', z64(cap - 1)),
                        ('starts', z64(S + 1).cpu()),
                        ('first', z64(2 * (S + 1))[::2]),
                        ('sessions', z64(0))):
        with pytest.raises(RuntimeError):
            assign(**{name: wrong})
    # sess_ranges
    rg = dict(first=z64(S + 1), rec_off=z64(cap), count=z64(1), total=z64(1),
              err=z32(1), rep_off=z64(S + 1))

    def ranges(**kw):
        a = dict(rg, **kw)
        extra = {k: a[k] for k in a if k not in rg}
        _lib.sess_ranges(a['first'], a['rec_off'], a['count'], cap,
                         a['total'], a['err'], a['rep_off'], **extra)

    ranges()
    for name, wrong in (('rep_off', z64(S)), ('rep_off', z32(S + 1)),
                        ('rec_off', z64(cap - 1)), ('err', z64(1)),
                        ('total', z64(1).cpu()), ('first', z64(1)),
                        ('slot_first', z64(65))):
        with pytest.raises(RuntimeError):
            ranges(**{name: wrong})
    with pytest.raises(RuntimeError):
        ranges(slot_first=z64(64), ev_rec_off=z64(8), ev_count=z64(1),
               ev_bytes=z64(1), ev_err=z32(1), slot_off=z64(65))
    with pytest.raises(RuntimeError):
        ranges(slot_first=z64(65), ev_rec_off=z64(8), ev_count=z64(1),
               ev_bytes=z64(1), ev_err=z32(1), slot_off=z64(64))
    # sess_group_events
    ecap = 300
    ws = z64(_lib.sess_group_workspace(ecap))
    ge = [z32(ecap), z32(ecap), z64(ecap), z32(ecap), z64(2), ws, z32(ecap),
          z32(ecap), z64(ecap), z32(ecap), z64(65)]
    _lib.sess_group_events(*ge)
    for k, wrong in ((1, z32(ecap - 1)), (2, z32(ecap)), (4, z64(1)),
                     (5, ws[:-1]), (5, ws.view(torch.uint8)),
                     (6, z32(ecap).cpu()), (8, z64(ecap - 1)),
                     (10, z64(64)), (0, z32(0))):
        bad = list(ge)
        bad[k] = wrong
        with pytest.raises(RuntimeError):
            _lib.sess_group_events(*bad)
    with pytest.raises(RuntimeError):
        _lib.sess_group_workspace(0)
    # the serves: a table whose rows disagree, a short f_seg
    from zkmi.server.engine import GpuServer
    tree = _tree(gpu)
    srv = GpuServer(tree, cap, 1 << 16)
    r = srv.resp
    out = [r.opcode, r.xid, r.err, r.node, r.zxid, r.path_off, r.path_len,
           r.slot, srv.presized[0], srv.presized[1]]
    rx = torch.zeros(64, dtype=torch.uint8, device=gpu)

    def frames(**kw):
        a = dict(f_seg=z32(cap), sessions=z64(S), wslots=z32(S),
                 seg_state=z32(S), bad=z64(2))
        a.update(kw)
        _lib.tree_serve_frames_sessions(
            tree.tensors, rx, z64(cap), z32(cap), z64(1), cap, out, 0, None,
            None, [a['f_seg'], a['sessions'], a['wslots'], a['seg_state'],
                   a['bad']])

    frames()
    for name, wrong in (('f_seg', z32(cap - 1)), ('wslots', z32(S + 1)),
                        ('wslots', z64(S)), ('seg_state', z32(S - 1)),
                        ('bad', z32(2)), ('sessions', z64(0)),
                        ('sessions', z64(S).cpu())):
        with pytest.raises(RuntimeError):
            frames(**{name: wrong})
    ows = torch.empty(L.tree_order_workspace(cap), dtype=torch.uint8,
                      device=gpu)
    with pytest.raises(RuntimeError):
        _lib.tree_serve_ordered_sessions(
            tree.tensors, rx, srv.rt.tensors(), z64(1), cap, out, 0, ows, 4,
            tree.scratch, None, None, [z32(cap), z64(S), z32(S + 1), z32(S),
                                       z64(2)])
    with pytest.raises(RuntimeError):
        _lib.tree_serve_ordered_sessions(
            tree.tensors, rx, srv.rt.tensors(), z64(1), cap, out, 0,
            ows[:-1], 4, tree.scratch, None, None, [z32(cap), z64(S), z32(S),
                                                    z32(S), z64(2)])


def test_segment_table_list_is_checked_once_for_all(gpu):
    """Every op of a session batch takes the segment table as one list,
    ``[f_seg, sessions, wslots, seg_state, bad]``, and refuses a malformed
    one before it launches anything: its outputs stay zero."""
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    L = _lib.lib()
    S, cap, ecap = 3, 256, 64
    tree = GpuTree(NLEAF, 16, fanout=FANOUT, device=gpu, seed=3,
                   watch_cap=4096, scratch=1 << 20, acl_cap=512)
    srv = GpuServer(tree, cap, 1 << 16)
    srv._mix_buffers()
    z64 = lambda n: torch.zeros(n, dtype=I64, device=gpu)     # noqa: E731
    z32 = lambda n: torch.zeros(n, dtype=I32, device=gpu)     # noqa: E731
    z8 = lambda n: torch.zeros(n, dtype=torch.uint8, device=gpu)  # noqa: E731
    rec = lambda: [z32(ecap), z32(ecap), z64(ecap), z32(ecap)]    # noqa: E731
    rx = z8(256)
    foff, flen, count = z64(cap), z32(cap), z64(1)
    good = [z32(cap), z64(S), z32(S), z32(S), z64(2)]
    out = [z32(cap), z32(cap), z32(cap), z64(cap), z64(cap), z64(cap),
           z32(cap), z64(cap), z64(cap), z64(1)]
    ows = torch.ones(L.tree_order_workspace(cap), dtype=torch.uint8,
                     device=gpu)
    clip = [z32(cap), z32(cap), z64(1), z32(cap), good[0], z32(cap),
            z32(cap), z64(S), z64(1)]
    l_out, c_out = z8(4096), z8(4096)
    l_res, c_res = [z64(cap), z64(1), z32(1)], [z64(cap), z64(1), z32(1)]
    ev, grouped = rec(), rec()
    rs = [z64(_lib.watch_resume_sessions_workspace(cap, ecap)), z64(2),
          z64(65), z64(8)]
    cl = [z32(cap), z64(_lib.close_workspace(cap, S, tree.cap)), z64(8)]

    def ordered(sg, with_clip):
        c = None
        if with_clip:                     # (seg_c0 is the table's f_seg)
            c = clip[:4] + [sg[0]] + clip[5:]
        _lib.tree_serve_ordered_sessions(
            tree.tensors, rx, srv.rt.tensors(), count, cap, out, 0, ows, 4,
            tree.scratch, None, None, sg, c)

    ops = [
        lambda sg: _lib.tree_serve_frames_sessions(
            tree.tensors, rx, foff, flen, count, cap, out, 0, None, None, sg),
        lambda sg: ordered(sg, False),
        lambda sg: ordered(sg, True),
        lambda sg: _lib.tree_list_sessions(
            tree.tensors, rx, foff, flen, count, cap, sg, 1 << 20,
            srv.list_want, srv.list_ws, l_out, 4096, *l_res),
        lambda sg: _lib.tree_acl_get_sessions(
            tree.tensors, tree.acl, rx, foff, flen, count, cap, sg,
            srv._acl_workspace(), c_out, 4096, *c_res),
        lambda sg: _lib.watch_resume_sessions(
            tree.tensors, rx, foff, flen, count, cap, sg, rs[0], ev, rs[1],
            grouped, rs[2], rs[3]),
        lambda sg: _lib.close_frames(
            tree.tensors, rx, foff, flen, count, cap, sg, cl[0], cap, cl[1],
            cl[2]),
    ]
    wrong = [good[:4], good + [z64(2)],
             [good[0], good[1], z32(S + 1), good[3], good[4]],
             [good[0], good[1], good[2], z64(S), good[4]]]
    for op in ops:
        for sg in wrong:
            with pytest.raises(RuntimeError):
                op(sg)
    torch.cuda.synchronize()
    outs = (out + clip + [l_out, c_out] + l_res + c_res + ev + grouped +
            rs + cl + good)
    assert not any(bool(t.any().item()) for t in outs)
    assert bool((ows == 1).all().item())
    assert bool((srv.list_want == _lib.LIST_IDLE).all().item())
