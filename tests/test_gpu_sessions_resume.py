"""GpuServer.serve_sessions / serve_sessions_mixed with ``resume=True``: the
SET_WATCHES catch-up of a whole session batch (csrc/kernels/tree_resume.hip;
the rules: csrc/kernels/zk_resume.h).

The model is test_gpu_sessions.SessModel under the batch contract: the
batch's other requests are applied in stream order through the fake server's
database, then its SET_WATCHES frames in stream order, each for its own
segment's session; the watchers' connections collect the events as
WatchModel.serve collects a resume's.  The write-fired events are compared
with ``srv.notif`` slot by slot, the catch-up's with ``srv.resume_notif``
slot by slot and in order, the counters with ``srv.resume_stats()``."""

import collections
import itertools
import struct
import time

import numpy as np
import pytest
import torch

from test_gpu_sessions import (FANOUT, NLEAF, SessModel, _raw, _segments,
                               _tree, dirp, leaf)
from test_resume_host import lists as raw_lists
from test_resume_host import body as raw_body
from test_resume_host import malformed, want_walk
from treemodel import create, delete, dev_bytes, get, set_data
from treemodel import _stream
from watchmodel import check_events, ls, set_watches, wget

from zkmi import jute
from zkmi.ops import _lib

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000.0
I64, I32 = torch.int64, torch.int32
CHUNK = _lib.RESUME_CHUNK
KINDS = {'CREATED', 'DELETED', 'DATA_CHANGED', 'CHILDREN_CHANGED'}


@pytest.fixture(autouse=True)
def _frozen_time(monkeypatch):
    monkeypatch.setattr(time, 'time', lambda: NOW)


def _clean(p):
    return {k: v for k, v in p.items() if k != '_rel_db'}


def _slot_frames(raw, n, slots, first, off):
    """{slot: [(type, path)]} of a slot-major xid -1 stream: ``raw`` bytes of
    ``n`` frames, ``slots`` per frame, the [65] tables ``first`` / ``off``."""
    assert first[0] == 0 and first[64] == n, (first[0], first[64], n)
    assert off[0] == 0 and off[64] == len(raw), (off[0], off[64], len(raw))
    assert first == sorted(first) and off == sorted(off)
    out = {}
    for w in range(64):
        a, b = first[w], first[w + 1]
        assert slots[a:b] == [w] * (b - a), (w, slots[a:b][:8])
        part = raw[off[w]:off[w + 1]]
        frames, used, bad = jute.scan_frames(part)
        assert bad < 0 and used == len(part) and len(frames) == b - a
        got = []
        for o, ln in frames:
            pkt = jute.decode_response(part[o:o + ln], {})
            assert pkt['xid'] == -1 and pkt['state'] == 'SYNC_CONNECTED'
            assert pkt['zxid'] == -1 and pkt['err'] == 'OK', pkt
            got.append((pkt['type'], pkt['path']))
        if got:
            out[w] = got
    return out


def resume_events(srv):
    """{slot: [(type, path)]} of ``srv.resume_notif``, each slot's decoded
    from its own slice (``srv.resume_slots``), in stream order."""
    buf, total, slots, count = srv.resume_notif
    n = int(count.item())
    first, off = (x.cpu().tolist() for x in srv.resume_slots)
    return _slot_frames(_raw(buf, total.item()), n, slots[:n].cpu().tolist(),
                        first, off)


def notif_events(srv):
    """{slot: [(type, path)]} of ``srv.notif`` after a session batch."""
    buf, total, slots, count = srv.notif
    n = int(count.item())
    first, off = (x.cpu().tolist() for x in srv.notif_slots)
    return _slot_frames(_raw(buf, total.item()), n, slots[:n].cpu().tolist(),
                        first, off)


def _replies(srv, out, total, segs):
    """[[reply, ...] of segment s] through ``rep_off``."""
    raw = _raw(out, total.item())
    off = srv.seg.rep_off.cpu().tolist()
    assert off[0] == 0 and off[-1] == len(raw) and off == sorted(off)
    reps = []
    for s, (_, _, pk) in enumerate(segs):
        part = raw[off[s]:off[s + 1]]
        frames, used, bad = jute.scan_frames(part)
        assert bad < 0 and used == len(part) and len(frames) == len(pk), \
            (s, used, len(part), len(frames), len(pk))
        xmap = {p['xid']: p['opcode'] for p in pk}
        rs = [jute.decode_response(part[o:o + ln], xmap) for o, ln in frames]
        assert [r['xid'] for r in rs] == [p['xid'] for p in pk]
        reps.append(rs)
    return reps


class ResumeModel(SessModel):
    """:class:`test_gpu_sessions.SessModel` with the catch-up."""

    def build(self, segs, starts=None):
        for _, _, pk in segs:
            for k, p in enumerate(pk):
                p['xid'] = 1 + k
        flat = [(s, p) for s, (_, _, pk) in enumerate(segs) for p in pk]
        parts = [_stream([_clean(p) for p in pk]) for _, _, pk in segs]
        rx = b''.join(parts)
        cuts = [0] + [int(x) for x in np.cumsum([len(b) for b in parts])]
        tab = _segments(self.dev, cuts if starts is None else starts,
                        [sid for sid, _, _ in segs], [w for _, w, _ in segs])
        return flat, rx, cuts, tab

    def resume(self, segs, table=None, dead=(), starts=None, refused=False,
               audit=True, no_slot=0):
        """One session batch with ``resume=True`` on the server and on the
        model.  ``dead`` / ``refused`` as :meth:`serve_sessions`;
        ``no_slot``: the paths live SET_WATCHES frames list in segments
        without a valid watcher slot.  Returns (replies by segment,
        write-fired model events, the catch-up's model events, stats)."""
        srv = self.srv
        flat, rx, cuts, tab = self.build(segs, starts)
        zxids = self.zxids_ok
        base = self.counter(_lib.TC_ZXID)
        out, total, err, ft = srv.serve_sessions(
            dev_bytes(rx, self.dev), len(rx), tab, table=table, resume=True)
        assert int(err.item()) == 0
        assert int(ft.count.item()) == len(flat)
        assert self.counter(_lib.TC_ZXID) == base + len(flat)
        st = srv.session_stats()
        assert (st['bad'] > 0) == bool(refused), st
        if refused:
            # (an unsound table slices nothing: the stream as a whole)
            raw = _raw(out, total.item())
            frames, used, bad = jute.scan_frames(raw)
            assert bad < 0 and used == len(raw) and len(frames) == len(flat)
            reps = [[jute.decode_response(raw[o:o + ln],
                                          {p['xid']: p['opcode']})]
                    for (o, ln), (_, p) in zip(frames, flat)]
        else:
            reps = _replies(srv, out, total, segs)
        # ---- the model: the other requests, then the SET_WATCHES frames
        want, rwant, writes, keys = [], [], [], {}
        listed = 0
        for i, (s, p) in enumerate(flat):
            sid, wslot = segs[s][0], segs[s][1]
            if refused:
                keys[i] = (p['xid'], 'SYSTEM_ERROR')
            elif s in dead:
                keys[i] = (p['xid'], 'SESSION_EXPIRED')
            elif p['opcode'] == 'SET_WATCHES':
                keys[i] = (p['xid'], 'OK')
            else:
                lens = self._lens()
                k = keys[i] = self._apply(p, sid or None, base + i + 1, zxids)
                if k[1] == 'OK' and p['opcode'] in ('CREATE', 'DELETE'):
                    writes.append((i, k[2] if p['opcode'] == 'CREATE'
                                   else p['path']))
                self._since(lens, i, want)
        for i, (s, p) in enumerate(flat):
            sid, wslot = segs[s][0], segs[s][1]
            if refused or s in dead or p['opcode'] != 'SET_WATCHES':
                continue
            if not 0 <= wslot < 64:
                continue
            assert self.slot_sid[wslot] == sid
            lens = self._lens()
            rep = self.db.handle(dict(_clean(p), relZxid=p['_rel_db']), sid)
            assert rep['err'] == 'OK'
            self._since(lens, i, rwant)
            listed += sum(len(v) for v in p['events'].values())
        got = [r for rs in reps for r in rs]
        for i, r in enumerate(got):
            g = self._reply_key(r, zxids)
            assert g == keys[i], 'request %d (segment %d): got %r, want %r' \
                % (i, flat[i][0], g, keys[i])
        # ---- the write-fired events: self.notif, as without resume
        bad = check_events(notif_events(srv), want, False, writes)
        assert bad is None, bad
        assert srv.ev_total.cpu().tolist() == [len(want), len(want)]
        # ---- the catch-up: per slot, in order
        sent = resume_events(srv)
        by_slot = collections.defaultdict(list)
        for _, slot, t, path in rwant:
            by_slot[slot].append((t, path))
        assert set(sent) == set(by_slot), (sorted(sent), sorted(by_slot))
        for w in sent:
            assert sent[w] == by_slot[w], (w, sent[w][:4], by_slot[w][:4])
        rs = srv.resume_stats()
        assert rs == {'events': len(rwant), 'events_written': len(rwant),
                      'rearmed': listed - len(rwant), 'listed': listed,
                      'dropped': 0, 'no_slot': no_slot, 'encode_err': 0}, rs
        assert srv.watch_stats()['lost_arms'] == 0
        self.batches += 1
        if audit:
            self.audit(zxids=self.zxids_ok)
        return reps, want, rwant, rs


def _model(gpu, frames=1024, watch_cap=4096):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(NLEAF, 16, fanout=FANOUT, device=gpu, seed=3,
                   watch_cap=watch_cap, scratch=1 << 20)
    srv = GpuServer(tree, frames, 1 << 21)
    return ResumeModel(tree, srv, gpu)


def _interleave(*ls_):
    out = []
    for t in itertools.zip_longest(*ls_):
        out += [x for x in t if x is not None]
    return out


class World(object):
    """Three phases of writes on the model's tree with a mark before each
    (``rel[0..2]``, and ``rel[3]`` after the last), and the master lists a
    SET_WATCHES draws from: whichever mark a frame carries, its lists hold
    every outcome of the session rule.  Phase k changes leaves of directory
    9, deletes leaves of directory 6 + k, and creates names under directories
    2 k and 2 k + 1; directories 10.. stay calm."""

    Q = 12

    def __init__(self, m, writer):
        q = self.Q
        self.rel, self.changed, self.deleted, self.born = [], [], [], []
        for k in range(3):
            self.rel.append(m.mark())
            ch = [leaf(9 * FANOUT + q * k + j) for j in range(q)]
            de = [leaf((6 + k) * FANOUT + j) for j in range(q)]
            bo = ['%s/born%d_%d' % (dirp(2 * k + j % 2), k, j)
                  for j in range(q)]
            m.serve([set_data(p, b'chg%d' % k) for p in ch] +
                    [delete(p) for p in de] +
                    [create(p, b'born') for p in bo], sid=writer, audit=False)
            self.changed.append(ch)
            self.deleted.append(de)
            self.born.append(bo)
        self.rel.append(m.mark())
        self.same = [leaf(k) for k in range(10 * FANOUT, 20 * FANOUT)]
        self.never = ['%s/never%04d' % (dirp(10 + j % 10), j)
                      for j in range(600)]
        self.there = [leaf(k) for k in range(10 * FANOUT, 15 * FANOUT)]
        self.touched = [dirp(d) for d in range(9)]
        self.calm = [dirp(d) for d in range(10, 20)]
        gone = _interleave(*self.deleted)
        self.data = _interleave(_interleave(*self.changed), gone, self.same)
        self.exist = _interleave(_interleave(*self.born), self.never,
                                 self.there)
        self.child = _interleave(self.touched, self.calm, gone)

    def frame(self, rel, n, start=0):
        """A SET_WATCHES of ``n`` paths, about a third a list (the child
        list is short: the rest goes to the other two), drawn from the
        master lists from ``start`` on; past their ends they repeat."""
        nc = min(n // 3, len(self.child))
        ne = (n - nc) // 2
        nd = n - nc - ne
        take = lambda m_, k: [m_[(start + j) % len(m_)]       # noqa: E731
                              for j in range(k)]
        return set_watches(rel, take(self.data, nd), take(self.exist, ne),
                           take(self.child, nc))

    def fire(self, pk_lists):
        """Writes that hit every path the frames ``pk_lists`` may have
        re-armed, each once: a set of every listed data path that exists, a
        create of every listed exist path that does not, a child under
        every listed directory."""
        data, exist, child = set(), set(), set()
        for p in pk_lists:
            data |= set(p['events']['dataChanged'])
            exist |= set(p['events']['createdOrDestroyed'])
            child |= set(p['events']['childrenChanged'])
        gone = set(_interleave(*self.deleted))
        out = [set_data(p, b'fire') for p in sorted(data - gone)]
        out += [create(p, b'late') for p in sorted(exist & set(self.never))]
        out += [create('%s/fire' % d, b'') for d in sorted(
            child & set(self.touched + self.calm))]
        return out


def _fire(m, w, frames, writer, slots):
    """The writes of ``World.fire`` as session batches of one writer; the
    model checks who is told.  Returns the events per slot."""
    pk = w.fire(frames)
    fired = collections.Counter()
    cap = m.srv.cap_frames
    for o in range(0, len(pk), cap):
        _, ev = m.serve_sessions([(writer, -1, pk[o:o + cap])],
                                 audit=o + cap >= len(pk))
        for _, slot, _, _ in ev:
            assert slot in slots, slot
            fired[slot] += 1
    return fired


# ---- 1. all branches, several sessions ---------------------------------------

def test_all_branches_several_sessions(gpu):
    m = _model(gpu)
    writer = m.session()
    w = World(m, writer)
    slots = (0, 31, 63)
    sids = [m.session(s) for s in slots]
    # three connections, three marks: each sees the later phases as changes
    # and the earlier ones as the state it knows
    frames = [w.frame(w.rel[k], 90) for k in range(3)]
    segs = [(sids[k], slots[k], [frames[k]]) for k in range(3)]
    _, want, rwant, rs = m.resume(segs)
    assert want == []
    for k, slot in enumerate(slots):
        mine = [e for e in rwant if e[1] == slot]
        assert {e[2] for e in mine} == KINDS, (slot, {e[2] for e in mine})
        # data and child watches both report a deleted node
        gone = set(_interleave(*w.deleted))
        assert sum(e[2] == 'DELETED' and e[3] in gone for e in mine) >= 2
    assert rs['listed'] == 270 and 0 < rs['rearmed'] < 270
    # every re-armed watch fires exactly once, at its own slot
    m.zxids_ok = False
    fired = _fire(m, w, frames, m.session(), slots)
    # (the lists of one frame hold no path twice: one arm, one event)
    assert sum(fired.values()) == rs['rearmed'], (fired, rs)
    # and is spent: the same writes again tell nobody
    _, ev = m.serve_sessions([(writer, -1, [set_data(p, b'again')
                                            for p in w.same[:40]])])
    assert ev == []


# ---- 2. the batch contract ---------------------------------------------------

def test_batch_contract(gpu):
    m = _model(gpu)
    a, b = m.session(3), m.session(4)
    la, lb, lc, ld = (leaf(1200 + k) for k in range(4))
    born = '%s/contract' % dirp(12)
    rel = m.mark()
    # B sets, deletes and creates what A lists, in the same batch, before
    # and after A's segment: A is told by the catch-up
    segs = [(b, 4, [set_data(la, b'b-was-here'), delete(lb)]),
            (a, 3, [set_watches(rel, [la, lb, lc], [born], [dirp(12), ld])]),
            (b, 4, [create(born, b'x')])]
    _, want, rwant, rs = m.resume(segs)
    assert want == []                   # self.notif carries nothing for them
    assert [(e[1], e[2], e[3]) for e in rwant] == [
        (3, 'DATA_CHANGED', la), (3, 'DELETED', lb), (3, 'CREATED', born),
        (3, 'CHILDREN_CHANGED', dirp(12))]
    assert rs['rearmed'] == 2
    # the next write of them fires nothing stale; the re-armed ones fire
    _, ev = m.serve_sessions([(b, 4, [set_data(la, b'2'), delete(born),
                                      set_data(lc, b'3'), delete(ld)])])
    assert sorted((e[1], e[2], e[3]) for e in ev) == sorted([
        (3, 'DATA_CHANGED', lc), (3, 'DELETED', ld)])
    # a SET_WATCHES in the middle of a segment's requests, and two in one
    # segment with different relZxids
    l0, l1, l2 = (leaf(1300 + k) for k in range(3))
    rel0 = m.mark()
    m.serve_sessions([(b, 4, [set_data(l0, b'one')])])
    rel1 = m.mark()
    m.serve_sessions([(b, 4, [set_data(l1, b'two')])])
    segs = [(a, 3, [wget(l2), set_watches(rel0, [l0, l1]), get(l0),
                    set_watches(rel1, [l0, l1], ['/bench/nope']),
                    set_data(leaf(1310), b'w')]),
            (b, 4, [set_watches(rel1, [l1], [], [dirp(13)]), get(l1)])]
    _, want, rwant, rs = m.resume(segs)
    assert [(e[0], e[1], e[2], e[3]) for e in rwant] == [
        (1, 3, 'DATA_CHANGED', l0), (1, 3, 'DATA_CHANGED', l1),
        (3, 3, 'DATA_CHANGED', l1), (5, 4, 'DATA_CHANGED', l1)]
    assert rs['rearmed'] == 3 and rs['listed'] == 7
    _, ev = m.serve_sessions([(b, 4, [set_data(l0, b'f'), set_data(l2, b'f'),
                                      create('/bench/nope', b'f')])])
    assert sorted((e[1], e[2], e[3]) for e in ev) == sorted([
        (3, 'DATA_CHANGED', l0), (3, 'DATA_CHANGED', l2),
        (3, 'CREATED', '/bench/nope')])


# ---- 3. sizes at the edges ---------------------------------------------------

def test_list_sizes(gpu):
    """Frames of 0 .. 3000 paths, one a connection, an empty list between
    two full ones, empty segments around a resuming one."""
    m = _model(gpu, watch_cap=16384)
    writer = m.session()
    w = World(m, writer)
    sizes = [0, 1, 63, 64, 65, 1023, 1024, 1025, 3000]
    slots = list(range(10, 10 + len(sizes))) + [40]
    sids = [m.session(s) for s in slots]
    frames = [w.frame(w.rel[k % 3], n, start=7 * k)
              for k, n in enumerate(sizes)]
    hole = set_watches(w.rel[0], w.data[:40], [], w.child[:20])
    segs = []
    for k, f in enumerate(frames):
        segs += [(sids[k], slots[k], [f]), (writer, -1, [])]
    segs = [(writer, -1, [])] + segs + [(sids[-1], 40, [hole])]
    _, want, rwant, rs = m.resume(segs)
    assert rs['listed'] == sum(sizes) + 60
    per = collections.Counter(e[1] for e in rwant)
    assert per[10] == 0 and all(per[s] > 0 for s in slots[2:])
    m.zxids_ok = False
    fired = _fire(m, w, frames + [hole], m.session(), set(slots))
    assert all(fired[s] > 0 for s in slots[2:])


def _pad_path(n):
    assert n >= 16
    return '/bench/d000010/' + 'p' * (n - 15)


def _sw_bytes(p):
    return len(_stream([dict(_clean(p), xid=1)]))


def test_chunk_edges(gpu):
    """Length words and paths across the edges of the chunks the kernel
    stages a frame in, at every byte phase; a frame of exactly one chunk and
    one of a chunk plus one byte."""
    m = _model(gpu)
    writer = m.session()
    w = World(m, writer)
    rel = w.rel[1]
    segs, at = [], 0
    tail = w.data[:30]
    # phases 0..7 of the second length word against the first and the
    # second edge: 0 the word starts on the edge, 1..3 it straddles it, 4..7
    # the path before it ends short of the edge and the next path straddles
    for k, (edge, d) in enumerate([(e, d) for e in (1, 2) for d in range(8)]):
        off = at + 4                        # the frame's body
        c0 = (off + 16) & ~15
        # body: 16 head, count, length word, the pad path, the next word
        pad = c0 + edge * CHUNK - d - (off + 24)
        p = set_watches(rel, [_pad_path(pad)] + tail, w.exist[k:k + 9],
                        w.child[:5])
        body = jute.encode_request(dict(_clean(p), xid=1))
        assert struct.unpack_from('>i', body, 24 + pad)[0] == len(tail[0])
        assert off + 24 + pad == c0 + edge * CHUNK - d
        segs.append((m.session(k), k, [p]))
        at += _sw_bytes(p)
    # a frame ending exactly on its first edge, and one byte past it
    for k, extra in ((20, 0), (21, 1)):
        off = at + 4
        c0 = (off + 16) & ~15
        p0 = set_watches(rel, tail[:20], [_pad_path(16)], [])
        short = off + (_sw_bytes(p0) - 4)           # its end with a 16 pad
        pad = 16 + (c0 + CHUNK + extra) - short
        assert pad >= 16
        p = set_watches(rel, tail[:20], [_pad_path(pad)], [])
        assert off + (_sw_bytes(p) - 4) == c0 + CHUNK + extra
        segs.append((m.session(k), k, [p]))
        at += _sw_bytes(p)
    _, want, rwant, rs = m.resume(segs)
    # every frame's lists were read whole; the pad path (no such node) of a
    # data list is a NodeDeleted
    assert rs['listed'] == 16 * (31 + 9 + 5) + 2 * 21
    pads = [e for e in rwant if '/ppp' in e[3]]
    assert len(pads) == 16 and {e[2] for e in pads} == {'DELETED'}
    assert {e[1] for e in rwant} >= set(range(16))


# ---- 4. differential: one batch against S single-session resumes ------------

def _raw_frames(bodies):
    return b''.join(jute.frame(b) for b in bodies)


def _single_events(srv):
    buf, total, res = srv.resume_notif
    res = res.cpu().tolist()
    raw = _raw(buf, total.item())
    frames, used, bad = jute.scan_frames(raw)
    assert bad < 0 and used == len(raw) and len(frames) == res[0] == res[2]
    out = []
    for o, ln in frames:
        pkt = jute.decode_response(raw[o:o + ln], {})
        assert pkt['xid'] == -1
        out.append((pkt['type'], pkt['path']))
    return out, res[1]


def _twin(gpu, before, **kw):
    """Two trees and servers in the same state after the writes ``before``."""
    from zkmi.server.engine import GpuServer
    out = []
    for _ in range(2):
        tree = _tree(gpu, **kw)
        srv = GpuServer(tree, 1024, 1 << 21)
        if before:
            rx = _stream([dict(p, xid=1 + k) for k, p in enumerate(before)])
            _, _, err, _ = srv.serve(dev_bytes(rx, gpu), len(rx), session=0)
            assert int(err.item()) == 0
        out.append((tree, srv))
    return out


def _sent_by_slot(srv):
    """``srv.notif`` of a single-session serve, {slot: sorted events}."""
    buf, total, slots, count = srv.notif
    n = int(count.item())
    raw = _raw(buf, total.item())
    frames, used, bad = jute.scan_frames(raw)
    assert bad < 0 and used == len(raw) and len(frames) == n
    out = collections.defaultdict(list)
    for s, (o, ln) in zip(slots[:n].cpu().tolist(), frames):
        pkt = jute.decode_response(raw[o:o + ln], {})
        out[s].append((pkt['type'], pkt['path']))
    return {s: sorted(v) for s, v in out.items()}


def _against_singles(gpu, parts, slots, before, after, listed=None):
    """The connections' SET_WATCHES bytes ``parts`` as one session batch on
    one tree and as len(parts) ``serve(resume=True)`` calls on its twin: the
    same events per slot in order, the same re-arm count, and the writes
    ``after`` fire the same events on both."""
    (t1, s1), (t2, s2) = _twin(gpu, before)
    rx = b''.join(parts)
    cuts = [0] + [int(x) for x in np.cumsum([len(p) for p in parts])]
    tab = _segments(gpu, cuts, [0] * len(parts), slots)
    _, _, err, _ = s1.serve_sessions(dev_bytes(rx, gpu), len(rx), tab,
                                     resume=True)
    assert int(err.item()) == 0
    got = resume_events(s1)
    want, rearmed = collections.defaultdict(list), 0
    for part, slot in zip(parts, slots):
        _, _, err, _ = s2.serve(dev_bytes(part, gpu), len(part), session=0,
                                wslot=slot, resume=True)
        assert int(err.item()) == 0
        ev, re_ = _single_events(s2)
        want[slot] += ev
        rearmed += re_
    want = {s: v for s, v in want.items() if v}
    assert got == want, (sorted(got), sorted(want))
    rs = s1.resume_stats()
    assert rs['rearmed'] == rearmed and rs['dropped'] == 0, (rs, rearmed)
    assert rs['events'] == rs['events_written'] == \
        sum(len(v) for v in want.values())
    if listed is not None:
        assert rs['listed'] == listed, (rs, listed)
    wr = _stream([dict(p, xid=1 + k) for k, p in enumerate(after)])
    s1.serve_sessions(dev_bytes(wr, gpu), len(wr),
                      _segments(gpu, [0, len(wr)], [0], [-1]))
    s2.serve(dev_bytes(wr, gpu), len(wr), session=0)
    f1 = {s: sorted(v) for s, v in notif_events(s1).items()}
    assert f1 == _sent_by_slot(s2)
    assert t1.watch_census() == t2.watch_census()
    return rs, f1


def _plain_world():
    """Writes before (after zxid ``rel``: the trees are fresh, their static
    nodes have the zxids 1 .. n_static) and path lists with every branch."""
    changed = [leaf(900 + k) for k in range(20)]
    deleted = [leaf(600 + k) for k in range(20)]
    born = ['%s/born%d' % (dirp(k % 4), k) for k in range(20)]
    before = [set_data(p, b'c') for p in changed] + \
        [delete(p) for p in deleted] + [create(p, b'b') for p in born]
    same = [leaf(1000 + k) for k in range(400)]
    never = ['%s/never%d' % (dirp(10 + k % 8), k) for k in range(200)]
    data = _interleave(changed, deleted, same)
    exist = _interleave(born, never, same[200:])
    child = _interleave([dirp(d) for d in range(20)], deleted)
    after = [set_data(p, b'f') for p in same] + \
        [create(p, b'f') for p in never] + \
        [create('%s/fire' % dirp(d), b'') for d in range(8, 20)]
    return before, data, exist, child, after


def test_differential(gpu):
    before, data, exist, child, after = _plain_world()
    rng = np.random.RandomState(5)
    rel = 2021 + 5      # after the static nodes, before most of `before`
    parts, slots, listed = [], [], 0
    for s in range(7):
        bodies = []
        for _ in range(int(rng.randint(1, 4))):
            pick = lambda m_: [m_[int(i)].encode() for i in sorted(  # noqa
                rng.choice(len(m_), int(rng.randint(0, 40)), replace=False))]
            ls_ = (pick(data), pick(exist), pick(child))
            listed += sum(len(x) for x in ls_)
            bodies.append(raw_body(raw_lists(*ls_),
                                   rel=rel + int(rng.randint(0, 60))))
        parts.append(_raw_frames(bodies))
        slots.append((0, 1, 17, 31, 32, 62, 63)[s])
    rs, fired = _against_singles(gpu, parts, slots, before, after, listed)
    assert rs['events'] > 50 and rs['rearmed'] > 50 and len(fired) == 7


# ---- 5. malformed frames -----------------------------------------------------

def test_malformed_frames(gpu):
    """The malformed corpus (tests/test_resume_host.py), a connection a
    frame with a good frame after it: the kernel against wt_resume_k on the
    same bytes and against the host rule — a frame whose lists are not whole
    lists nothing."""
    before, data, exist, child, after = _plain_world()
    good = raw_body(raw_lists([p.encode() for p in data[:30]],
                              [p.encode() for p in exist[:30]],
                              [p.encode() for p in child[:30]]), rel=2030)
    corpus = malformed()
    # (a frame without a body is the frame scan's business, not the walk's)
    names = sorted(n for n in corpus if len(corpus[n]) > 0)
    parts, slots, listed = [], [], 0
    for k, n in enumerate(names):
        bad = corpus[n]
        for body in (bad, good):
            ok, paths = want_walk(body)
            if ok and len(body) >= 20 and \
                    struct.unpack_from('>i', body, 4)[0] == 101:
                listed += len(paths)
        parts.append(_raw_frames([bad, good]))
        slots.append(k)
    assert len(names) >= 8 and len(parts) <= 64
    rs, _ = _against_singles(gpu, parts, slots, before, after, listed)
    assert rs['listed'] >= 90 * len(names)


# ---- 6. refusals -------------------------------------------------------------

def _census_after(m, segs, **kw):
    census = m.tree.watch_census()
    out = m.resume(segs, **kw)
    assert m.tree.watch_census() == census       # nothing armed
    assert out[2] == [] and out[3]['events'] == 0 and \
        out[3]['rearmed'] == 0
    return out


def test_refusals(gpu):
    from zkmi.server.sessions import GpuSessionTable
    m = _model(gpu)
    tab = GpuSessionTable(m.tree, cap=64)
    sid = [tab.sid_of(k) for k in range(3)]
    for k in range(3):
        tab.sid[k] = sid[k]
        tab.state[k] = 1
    tab.next.fill_(3)
    tab.close(torch.tensor([sid[2]], dtype=I64, device=gpu))
    a = m.session_as(sid[0], 0)
    b = m.session_as(sid[1], 1)
    dead = m.session_as(sid[2], 2)
    rel = m.mark()
    m.serve_sessions([(a, 0, [set_data(leaf(1400), b'chg')])], table=tab)
    data = [leaf(1400 + k) for k in range(6)]
    exist = ['%s/refused%d' % (dirp(14), k) for k in range(3)]
    child = [dirp(14), dirp(15)]
    sw = lambda: set_watches(rel, data, exist, child)       # noqa: E731
    n = len(data) + len(exist) + len(child)
    # a dead session's segment between two live ones
    _, _, rwant, rs = m.resume(
        [(a, 0, [sw()]), (dead, 2, [sw(), get(leaf(3))]), (b, 1, [sw()])],
        table=tab, dead={1})
    assert {e[1] for e in rwant} == {0, 1} and rs['listed'] == 2 * n
    assert m.srv.session_stats()['expired_segments'] == 1
    # watcher slots outside 0..63: counted, nothing else
    c, d = m.session(), m.session()
    _census_after(m, [(c, -1, [sw()]), (d, 64, [get(leaf(4)), sw()])],
                  no_slot=2 * n)
    # a torn segment table refuses the whole batch
    segs = [(a, 0, [sw()]), (b, 1, [sw()])]
    _, _, cuts, _ = m.build(segs)
    _census_after(m, segs, starts=[0, cuts[1] - 3, cuts[2]], refused=True)
    _census_after(m, segs, starts=[4, cuts[1], cuts[2]], refused=True)
    # the dead segment armed nothing: a later write of every listed path
    # tells slots 0 and 1 (armed above) and never slot 2
    _, ev = m.serve_sessions(
        [(a, 0, [set_data(p, b'w') for p in data[1:]] +
          [create(p, b'w') for p in exist] +
          [create('%s/w' % child[1], b'w')])], table=tab)
    assert {e[1] for e in ev} == {0, 1}
    # (the sets, the creates, and one NodeChildrenChanged a directory)
    assert len(ev) == 2 * (len(data) - 1 + len(exist) + 2)


# ---- 7. mixed ----------------------------------------------------------------

def test_mixed(gpu):
    """serve_sessions_mixed(resume=True) with GET_CHILDREN2 and GET_ACL
    around the SET_WATCHES frames: the replies of the call without resume,
    the catch-up of serve_sessions(resume=True) on the SET_WATCHES frames
    alone."""
    from zkmi.server.engine import GpuServer
    before, data, exist, child, after = _plain_world()
    rel = 2030
    trees = []
    for _ in range(3):
        tree = _tree(gpu, acl_cap=512)
        srv = GpuServer(tree, 1024, 1 << 21)
        rx = _stream([dict(p, xid=1 + k) for k, p in enumerate(before)])
        srv.serve(dev_bytes(rx, gpu), len(rx), session=0)
        trees.append((tree, srv))
    slots = (2, 33, 63, 64)
    mixed, only = [], []
    for s, slot in enumerate(slots):
        sw = [dict(_clean(set_watches((rel + 7 * k, 0),
                                      data[20 * s + 9 * k:][:25],
                                      exist[15 * s:][:20 + k],
                                      child[5 * s:][:9])), xid=10 + k)
              for k in range(2)]
        pk = [dict(ls(dirp(s), watch=False), xid=1),
              {'xid': 2, 'opcode': 'GET_ACL', 'path': dirp(3)}, sw[0],
              dict(get(leaf(1000 + s)), xid=3),
              dict(ls(dirp(12), watch=False, stat=False), xid=4), sw[1],
              {'xid': 5, 'opcode': 'GET_ACL', 'path': '/bench/nope'}]
        mixed.append(_stream(pk))
        only.append(_stream(sw))

    def run(srv, parts, how, **kw):
        rx = b''.join(parts)
        cuts = [0] + [int(x) for x in np.cumsum([len(p) for p in parts])]
        tab = _segments(gpu, cuts, [0] * len(parts), slots)
        out, total, err, _ = getattr(srv, how)(dev_bytes(rx, gpu), len(rx),
                                               tab, **kw)
        assert int(err.item()) == 0
        # (the order of the names inside a list reply is the sweep's: two
        # trees need not agree on it)
        raw = _raw(out, total.item())
        off = srv.seg.rep_off.cpu().tolist()
        assert off[0] == 0 and off[-1] == len(raw) and off == sorted(off)
        keys = []
        for a, b in zip(off, off[1:]):
            frames, used, bad = jute.scan_frames(raw[a:b])
            assert bad < 0 and used == b - a
            seg = []
            for o, ln in frames:
                r = jute.decode_response(raw[a + o:a + o + ln], xmap)
                st = r.get('stat')
                seg.append((r['xid'], r['err'], r['zxid'], r['opcode'],
                            sorted(r.get('children') or []),
                            bytes(r.get('data') or b''), repr(r.get('acl')),
                            None if st is None else (
                                st.czxid, st.mzxid, st.pzxid, st.version,
                                st.cversion, st.dataLength, st.numChildren)))
            keys.append(seg)
        return keys

    xmap = {1: 'GET_CHILDREN2', 2: 'GET_ACL', 3: 'GET_DATA',
            4: 'GET_CHILDREN', 5: 'GET_ACL', 10: 'SET_WATCHES',
            11: 'SET_WATCHES'}
    r0 = run(trees[0][1], mixed, 'serve_sessions_mixed')
    assert trees[0][1].resume_notif is None
    r1 = run(trees[1][1], mixed, 'serve_sessions_mixed', resume=True)
    assert r0 == r1 and [len(x) for x in r0] == [7] * 4
    assert [k[1] for k in r0[0]] == ['OK'] * 6 + ['NO_NODE']
    run(trees[2][1], only, 'serve_sessions', resume=True)
    ev1, ev2 = resume_events(trees[1][1]), resume_events(trees[2][1])
    assert ev1 == ev2 and set(ev1) == {2, 33, 63}
    st1, st2 = trees[1][1].resume_stats(), trees[2][1].resume_stats()
    assert st1 == st2 and st1['no_slot'] > 0 and st1['rearmed'] > 0
    assert trees[1][0].watch_census() == trees[2][0].watch_census()
    assert notif_events(trees[1][1]) == {} == notif_events(trees[0][1])


# ---- 8. the default is unchanged ---------------------------------------------

def test_default_is_unchanged(gpu):
    """Without ``resume`` a SET_WATCHES frame gets its header-only reply and
    nothing else, from both entry points; ``resume_notif`` is not written;
    ``resume=True`` without a watch table raises."""
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    m = _model(gpu)
    a = m.session(7)
    rel = m.mark()
    m.serve_sessions([(a, 7, [set_data(leaf(1500), b'x')])])
    census = m.tree.watch_census()
    segs = [(a, 7, [get(leaf(1)), set_watches(rel, [leaf(1500), leaf(1501)],
                                              ['/bench/no'], [dirp(15)])])]
    flat, rx, cuts, tab = m.build(segs)
    for how in ('serve_sessions', 'serve_sessions_mixed'):
        out, total, err, ft = getattr(m.srv, how)(dev_bytes(rx, gpu), len(rx),
                                                  tab)
        assert int(err.item()) == 0
        reps = _replies(m.srv, out, total, segs)
        assert [(r['opcode'], r['err']) for r in reps[0]] == [
            ('GET_DATA', 'OK'), ('SET_WATCHES', 'OK')]
        assert m.srv.ev_total.cpu().tolist() == [0, 0]
        assert m.tree.watch_census() == census
        assert m.srv.resume_notif is None and m.srv.resume_slots is None
        with pytest.raises(ValueError):
            m.srv.resume_stats()
    plain = GpuTree(200, 16, fanout=FANOUT, device=gpu, seed=3)
    srv = GpuServer(plain, 64, 1 << 16)
    for how in ('serve_sessions', 'serve_sessions_mixed'):
        with pytest.raises(ValueError):
            getattr(srv, how)(dev_bytes(rx, gpu), len(rx), tab, resume=True)


# ---- 9. the op checks its tensors --------------------------------------------

def test_op_checks_its_tensors(gpu):
    tree = _tree(gpu)
    S, cap, ecap = 3, 16, 64
    z64 = lambda n: torch.zeros(n, dtype=I64, device=gpu)     # noqa: E731
    z32 = lambda n: torch.zeros(n, dtype=I32, device=gpu)     # noqa: E731
    rec = lambda n=ecap: [z32(n), z32(n), z64(n), z32(n)]     # noqa: E731
    nws = _lib.watch_resume_sessions_workspace(cap, ecap)
    good = dict(rx=torch.zeros(256, dtype=torch.uint8, device=gpu),
                frame_off=z64(cap), frame_len=z32(cap), count=z64(1),
                f_seg=z32(cap), sessions=z64(S), wslots=z32(S),
                seg_state=z32(S), bad=z64(2), ws=z64(nws), ev=rec(), ev_total=z64(2), grouped=rec(),
                slot_first=z64(65), stats=z64(8))

    def call(ncap=cap, **kw):
        a = dict(good, **kw)
        _lib.watch_resume_sessions(
            tree.tensors, a['rx'], a['frame_off'], a['frame_len'], a['count'],
            ncap, [a['f_seg'], a['sessions'], a['wslots'], a['seg_state'],
                   a['bad']], a['ws'], a['ev'], a['ev_total'], a['grouped'], a['slot_first'], a['stats'])

    call()
    torch.cuda.synchronize()
    assert good['stats'].cpu().tolist() == [0] * 8
    wrong = [('rx', good['rx'].to(I32)), ('rx', good['rx'].cpu()),
             ('rx', torch.zeros(512, dtype=torch.uint8, device=gpu)[::2]),
             ('frame_off', z64(cap - 1)), ('frame_off', z32(cap)),
             ('frame_len', z32(cap - 1)), ('frame_len', z64(cap)),
             ('count', z32(1)), ('count', z64(0)),
             ('f_seg', z32(cap - 1)), ('f_seg', z64(cap)),
             ('wslots', z64(S)), ('wslots', z32(0)),
             ('seg_state', z32(S - 1)), ('seg_state', z64(S)),
             ('seg_state', z32(2 * S)[::2]), ('bad', z64(1)),
             ('bad', z32(2)), ('ws', z64(nws - 1)), ('ws', z32(nws)),
             ('ws', z64(nws).cpu()), ('ev', rec()[:3]),
             ('ev', [z32(ecap), z32(ecap), z32(ecap), z32(ecap)]),
             ('ev', [z32(ecap), z32(ecap - 1), z64(ecap), z32(ecap)]),
             ('grouped', rec(ecap - 1)), ('grouped', rec() + [z32(1)]),
             ('ev_total', z64(1)), ('slot_first', z64(64)),
             ('slot_first', z32(65)), ('stats', z64(7)),
             ('stats', z64(8).cpu())]
    for name, t in wrong:
        with pytest.raises(RuntimeError):
            call(**{name: t})
    with pytest.raises(RuntimeError):
        call(ncap=0)
    with pytest.raises(RuntimeError):
        call(ncap=cap + 1)
    from zkmi.server.tree import GpuTree
    plain = GpuTree(200, 16, fanout=FANOUT, device=gpu, seed=3)
    with pytest.raises(RuntimeError):
        _lib.watch_resume_sessions(
            plain.tensors, good['rx'], good['frame_off'], good['frame_len'],
            good['count'], cap, [good['f_seg'], good['sessions'],
                                 good['wslots'], good['seg_state'],
                                 good['bad']], good['ws'], good['ev'],
            good['ev_total'], good['grouped'], good['slot_first'],
            good['stats'])
