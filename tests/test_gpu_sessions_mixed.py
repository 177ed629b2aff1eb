"""GpuServer.serve_sessions_mixed: one batch carrying the whole frames of many
connections, whatever ops they mix (csrc/kernels/tree_sess.hip
sess_split_seg_k, the session instances of the list and GET_ACL engines in
tree_list.hip / tree_acl.hip; the rules: csrc/kernels/zk_sess.h).

The batch contract under test: one segment assign and one split over the
whole frame table, the engines in the order serve, GET_ACL, list, each frame
for its own segment's session and watcher slot; refusals (an unsound table,
a dead session) header-only and without effect.  time.time is frozen so two
trees' Stats compare exactly."""

import collections
import random
import struct
import time

import numpy as np
import pytest
import torch

from test_gpu_mixed import (A, ACL2, C, L, LEAVES, _batch, _body, _class,
                            _dev_bytes, _leaf, _norm, _patterns, _read_only,
                            _replies, _stream)
from test_gpu_sessions import (NDIR, POOL_DIRS, SessModel, _pool, _request,
                               _segments, _tree, dirp)
from watchmodel import check_events, ls

from zkmi import jute
from zkmi.ops import _lib

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000.0
I64, I32, U8 = torch.int64, torch.int32, torch.uint8
CC = 'CHILDREN_CHANGED'


@pytest.fixture(autouse=True)
def _frozen_time(monkeypatch):
    monkeypatch.setattr(time, 'time', lambda: NOW)


def _server(gpu, fanout=10, frames=1024, acl=True, watch=True):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(LEAVES[fanout], 16, fanout=fanout, device=gpu, spare=4.0,
                   ctime_ms=int(NOW * 1000), acl_cap=512 if acl else 0,
                   watch_cap=2048 if watch else 0)
    return GpuServer(tree, frames, 1 << 20, window=512)


def _raw(buf, total):
    return bytes(buf[:int(total)].cpu().numpy().tobytes())


def _slot_slices(srv):
    """{watcher slot: [(type, path)]}, each slot's notifications decoded from
    its own slice notif_buf[slot_off[w]:slot_off[w + 1]]."""
    buf, total, slots, count = srv.notif
    n = int(count.item())
    raw = _raw(buf, total.item())
    first, off = (x.cpu().tolist() for x in srv.notif_slots)
    assert first[0] == 0 and first[64] == n and off[0] == 0
    assert off[64] == len(raw) and off == sorted(off)
    sl = slots[:n].cpu().tolist()
    out = {}
    for w in range(64):
        part = raw[off[w]:off[w + 1]]
        frames, used, bad = jute.scan_frames(part)
        assert bad < 0 and used == len(part)
        assert len(frames) == first[w + 1] - first[w]
        assert sl[first[w]:first[w + 1]] == [w] * len(frames)
        got = []
        for o, ln in frames:
            pkt = jute.decode_response(part[o:o + ln], {})
            assert pkt['xid'] == -1
            got.append((pkt['type'], pkt['path']))
        if got:
            out[w] = got
    return out


def _serve(srv, gpu, conns, starts=None, want_err=0, **kw):
    """One serve_sessions_mixed batch.  ``conns``: [(session, watcher slot,
    [packet, ...])], a connection a segment.  Returns [(frame bytes, decoded
    reply)] in request order; checks the frame table, the segments of the
    frames, the merged frame starts and every connection's rep_off slice."""
    parts = [_stream(pk) for _, _, pk in conns]
    rx = b''.join(parts)
    cuts = [0] + [int(x) for x in np.cumsum([len(b) for b in parts])]
    segs = _segments(gpu, cuts if starts is None else starts,
                     [s for s, _, _ in conns], [w for _, w, _ in conns])
    flat = [p for _, _, pk in conns for p in pk]
    out, total, err, ft = srv.serve_sessions_mixed(
        _dev_bytes(rx, gpu), len(rx), segs, **kw)
    assert int(err.item()) == want_err
    assert int(ft.count.item()) == len(flat)
    if want_err:
        return []
    # (xids collide across connections: every reply is decoded as its own
    # request's)
    raw = _raw(out, total.item())
    frames, used, bad = jute.scan_frames(raw)
    assert bad < 0 and used == len(raw) and len(frames) == len(flat)
    reps = [(raw[o - 4:o + ln], jute.decode_response(
        raw[o:o + ln], {p['xid']: p.get('opcode', 'PING')}))
        for (o, ln), p in zip(frames, flat)]
    assert [r['xid'] for _, r in reps] == [p['xid'] for p in flat]
    rec = srv.last_rec_off[:len(flat)].cpu().tolist()
    assert rec == list(np.cumsum([0] + [len(f) for f, _ in reps])[:-1])
    sg = srv.seg
    if starts is not None:              # (an unsound table: no slices)
        return reps
    off = sg.rep_off.cpu().tolist()
    assert off[0] == 0 and off[-1] == len(raw) and off == sorted(off)
    first = [0] + [int(x) for x in np.cumsum([len(pk) for _, _, pk in conns])]
    assert sg.first.cpu().tolist() == first
    for s in range(len(conns)):
        mine = b''.join(f for f, _ in reps[first[s]:first[s + 1]])
        assert raw[off[s]:off[s + 1]] == mine, s
    want_seg = [s for s, (_, _, pk) in enumerate(conns) for _ in pk]
    assert sg.f_seg[:len(flat)].cpu().tolist() == want_seg
    assert sg.bad.cpu().tolist() == [0, -1]
    return reps


# ---- 1. equals the existing entry points ------------------------------------

def _cut(rng, n, S):
    """n frames over S connections, empty ones among them (S > 1)."""
    if S == 1:
        return [n]
    at = sorted(int(x) for x in rng.integers(0, n + 1, S - 1))
    at = [0] + at + [n]
    return [b - a for a, b in zip(at, at[1:])]


def _dress(pk, k0):
    """test_gpu_mixed's batch with what makes the segment matter: some lists
    and reads set a watch, some creates are EPHEMERAL."""
    for k, p in enumerate(pk):
        op = p['opcode']
        if op in ('GET_CHILDREN', 'GET_CHILDREN2', 'GET_DATA', 'EXISTS'):
            p['watch'] = (k + k0) % 3 != 1
        if op == 'CREATE' and p['acl'] is not ACL2 and k % 2:
            p['flags'] = ['EPHEMERAL']
    return pk


def _existing(srv, gpu, conns):
    """The batch through the existing entry points: serve_sessions on the
    serve-class frames re-concatenated with their segment table, one
    serve_acl on all GET_ACL frames, serve_list a segment on its list frames
    with its watcher slot.  Returns the replies in request order, the class
    of every request, and the grouped notification slices."""
    cls = [[_class(_body(p)) for p in pk] for _, _, pk in conns]
    part = {c: [[p for p, k in zip(pk, ks) if k == c]
                for (_, _, pk), ks in zip(conns, cls)] for c in (A, C, L)}
    got = {A: [], C: [], L: []}
    parts = [_stream(pk) for pk in part[A]]
    rx = b''.join(parts)
    cuts = [0] + [int(x) for x in np.cumsum([len(b) for b in parts])]
    segs = _segments(gpu, cuts, [s for s, _, _ in conns],
                     [w for _, w, _ in conns])
    flat = [p for pk in part[A] for p in pk]
    out, total, err, _ = srv.serve_sessions(_dev_bytes(rx, gpu), len(rx),
                                            segs)
    assert int(err.item()) == 0
    got[A] = _replies(out, total, flat)
    notes = _slot_slices(srv)
    flat = [p for pk in part[C] for p in pk]
    if flat:
        s = _stream(flat)
        out, total, err, _ = srv.serve_acl(_dev_bytes(s, gpu), len(s))
        assert int(err.item()) == 0
        got[C] = _replies(out, total, flat)
    for (_, w, _), pk in zip(conns, part[L]):
        if pk:
            s = _stream(pk)
            # (serve_list takes -1..63; anything else arms nothing)
            out, total, err, _ = srv.serve_list(_dev_bytes(s, gpu), len(s),
                                                wslot=w if 0 <= w < 64
                                                else -1)
            assert int(err.item()) == 0
            got[L] += _replies(out, total, pk)
    its = {c: iter(got[c]) for c in got}
    flat_cls = [k for ks in cls for k in ks]
    return [next(its[c]) for c in flat_cls], flat_cls, notes


@pytest.mark.parametrize('n,fanout', [(1, 10), (63, 10), (64, 300), (65, 10),
                                      (255, 10), (256, 300), (257, 10),
                                      (600, 10)])
def test_equals_the_existing_entry_points(gpu, n, fanout):
    """Twin trees with an ACL table and a watch table; every class pattern
    of test_gpu_mixed (all of one class — a segment then holds list frames
    only —, alternating, a class absent) over S = 1, 3, 64, 65 and 200
    connections with empty ones among them.  Replies per request, rep_off
    slices (in _serve), grouped notification slices, digest, watch census
    and ACL statistics are equal; a scalar watcher slot or a missing gather
    of the segments shows in the census and the slices."""
    sx, sy = _server(gpu, fanout), _server(gpu, fanout)
    rng = np.random.default_rng(7 * n)
    sizes = (1, 3, 64, 65, 200)
    fired = 0
    for gen, (name, classes) in enumerate(_patterns(n)):
        S = sizes[gen % len(sizes)]
        pk = _dress(_batch(classes, fanout, gen), gen)
        conns, k = [], 0
        for s, size in enumerate(_cut(rng, n, S)):
            w = (-1, 64)[s % 2] if s % 5 == 4 else (7 * s + gen) % 64
            conns.append((0x100 + s % 11, w, pk[k:k + size]))
            k += size
        assert k == n and len(conns) == S
        x = _serve(sx, gpu, conns)
        y, cls, ynotes = _existing(sy, gpu, conns)
        assert cls == [int(c) for c in classes], name
        assert len(x) == len(y) == n
        for i, ((fx, rx), (fy, ry), c) in enumerate(zip(x, y, cls)):
            assert _norm(rx) == _norm(ry), (name, S, i, rx, ry)
            if c != L:
                assert fx == fy, (name, S, i)
            else:
                assert len(fx) == len(fy)
        # (which of a batch's concurrent creates under one parent takes the
        # parent's child watch is the batch's business: a multiset a slot,
        # as watchmodel.check_events compares an unordered batch)
        xnotes = _slot_slices(sx)
        assert {w: sorted(v) for w, v in xnotes.items()} == \
            {w: sorted(v) for w, v in ynotes.items()}, (name, S)
        fired += sum(len(v) for v in xnotes.values())
        assert sx.tree.digest() == sy.tree.digest(), (name, S)
        assert sx.tree.watch_census() == sy.tree.watch_census(), (name, S)
        assert sx.watch_stats()['lost_arms'] == 0
    assert sx.acl_stats() == sy.acl_stats()
    if n >= 255:
        assert fired > 0            # watches of several slots did fire
        assert sx.tree.watch_census()[1] > 0


# ---- 2. cross-connection visibility -----------------------------------------

def test_cross_connection_visibility(gpu):
    srv = _server(gpu)
    d = '/bench/d000000'
    gone = _leaf(10, 3)
    mk = {'xid': 1, 'opcode': 'CREATE', 'path': d + '/c', 'data': b'x',
          'acl': ACL2, 'flags': []}
    conns = [(0x11, -1, [mk]),
             (0x12, -1, [{'xid': 1, 'opcode': 'DELETE', 'path': gone,
                          'version': -1}]),
             (0x13, -1, [{'xid': 1, 'opcode': 'GET_CHILDREN2', 'path': d,
                          'watch': False}]),
             (0x14, -1, [{'xid': 1, 'opcode': 'GET_ACL', 'path': d + '/c'}])]
    for order in (conns, conns[::-1]):
        reps = [r for _, r in _serve(srv, gpu, order)]
        by = {c[0]: r for c, r in zip(order, reps)}
        if order is conns:
            assert [r['err'] for r in reps] == ['OK'] * 4
            assert 'c' in by[0x13]['children']
            assert gone.rpartition('/')[2] not in by[0x13]['children']
            assert len(by[0x13]['children']) == 10
            assert by[0x13]['stat'].numChildren == 10
            wire = jute.decode_request(jute.encode_request(mk))['acl']
            assert by[0x14]['acl'] == wire
        else:
            # the second time the writes fail; the reads see the same tree,
            # whichever side of the writers their connection is on
            assert by[0x11]['err'] == 'NODE_EXISTS'
            assert by[0x12]['err'] == 'NO_NODE'
            assert 'c' in by[0x13]['children'] and by[0x14]['err'] == 'OK'


# ---- 3. arms land on the right watcher --------------------------------------

def test_arms_land_on_the_right_watcher(gpu):
    srv = _server(gpu)
    tree = srv.tree
    slots = [0, 31, 32, 63, -1, 64]
    par = ['/bench/d%06d' % k for k in range(6)]

    def lists(ks):
        return [(0x20 + k, slots[k], [
            {'xid': 5, 'opcode': 'GET_CHILDREN2' if k % 2 else
             'GET_CHILDREN', 'path': par[k], 'watch': True}]) for k in ks]

    census = tree.watch_census()
    # the -1 and the 64 connection alone: nothing changes
    reps = _serve(srv, gpu, lists([4, 5]))
    assert [r['err'] for _, r in reps] == ['OK', 'OK']
    assert tree.watch_census() == census
    assert srv.watch_stats()['lost_arms'] == 0
    # all six, interleaved with a writer whose creates do not fire the arms
    # of their own batch
    conns = lists(range(6))
    conns.insert(3, (0x30, -1, [
        {'xid': 9, 'opcode': 'CREATE', 'path': par[0] + '/early',
         'data': b'', 'acl': jute.DEFAULT_ACL, 'flags': []}]))
    reps = _serve(srv, gpu, conns)
    assert all(r['err'] == 'OK' for _, r in reps)
    assert _slot_slices(srv) == {}
    after = tree.watch_census()
    assert after[1] == census[1] + 4 and after[2] == 0
    assert srv.watch_stats()['lost_arms'] == 0
    # another connection creates a child under each parent
    mk = [{'xid': 1 + k, 'opcode': 'CREATE', 'path': par[k] + '/kid',
           'data': b'', 'acl': jute.DEFAULT_ACL, 'flags': []}
          for k in range(6)]
    reps = _serve(srv, gpu, [(0x31, -1, mk[:2]), (0x32, 5, mk[2:])])
    assert all(r['err'] == 'OK' for _, r in reps)
    assert _slot_slices(srv) == {slots[k]: [(CC, par[k])] for k in range(4)}
    assert srv.ev_total.cpu().tolist() == [4, 4]
    # one-shot: a second child fires nothing
    mk = [dict(p, path=p['path'] + '2') for p in mk]
    _serve(srv, gpu, [(0x31, -1, mk)])
    assert _slot_slices(srv) == {}


# ---- 4. refusals have no effect ---------------------------------------------

def _trunc(p):
    body = jute.encode_request(p)
    return dict(p, raw=body[:-1])


def _refused_conns():
    d = ['/bench/d%06d' % k for k in range(4)]
    return [
        (0x41, 0, [
            {'xid': 1, 'opcode': 'GET_CHILDREN2', 'path': d[0],
             'watch': True},
            {'xid': 2, 'opcode': 'SET_DATA', 'path': _leaf(10, 5),
             'data': b'no', 'version': -1},
            {'xid': 3, 'opcode': 'GET_ACL', 'path': d[0]}]),
        (0x42, 9, [
            {'xid': 1, 'opcode': 'CREATE', 'path': d[1] + '/no', 'data': b'',
             'acl': ACL2, 'flags': []},
            {'xid': 2, 'opcode': 'GET_CHILDREN', 'path': d[1], 'watch': True},
            _trunc({'xid': 3, 'opcode': 'GET_CHILDREN2', 'path': d[1],
                    'watch': True}),
            {'xid': 4, 'opcode': 'GET_ACL', 'path': '/bench/nope'},
            {'xid': 5, 'opcode': 'GET_DATA', 'raw':
             struct.pack('>ii', 5, 9999) + b'\0' * 8}]),
        (0x43, 63, [
            _trunc({'xid': 1, 'opcode': 'GET_ACL', 'path': d[2]}),
            {'xid': 2, 'opcode': 'DELETE', 'path': _leaf(10, 6),
             'version': -1},
            {'xid': 3, 'opcode': 'GET_CHILDREN2', 'path': d[2],
             'watch': True}])]


def test_bad_tables_refuse_every_engine(gpu):
    srv = _server(gpu)
    tree = srv.tree
    conns = _refused_conns()
    parts = [_stream(pk) for _, _, pk in conns]
    cuts = [0] + [int(x) for x in np.cumsum([len(b) for b in parts])]
    n = sum(len(pk) for _, _, pk in conns)
    # a sound batch first, so that every table of the server has held rows
    _serve(srv, gpu, [(0, -1, _batch(np.array([A, C, L] * 8), 10, 0))])
    cases = [
        [0, cuts[1] + 2, cuts[2], cuts[3]],     # a torn frame (length word)
        [0, cuts[1], cuts[2] - 3, cuts[3]],     # a torn frame (body)
        [4, cuts[1], cuts[2], cuts[3]],         # starts[0] != 0
        [0, cuts[2], cuts[1], cuts[3]],         # a descending pair
    ]
    for starts in cases:
        dig, census = tree.digest(), tree.watch_census()
        acl = srv.acl_stats()
        zx = int(tree.counters[_lib.TC_ZXID].item())
        reps = _serve(srv, gpu, conns, starts=starts)
        assert srv.session_stats()['bad'] > 0
        assert len(reps) == n
        for f, r in reps:
            assert r['err'] == 'SYSTEM_ERROR' and len(f) == 20, (starts, r)
        assert tree.digest() == dig
        assert tree.watch_census() == census
        assert srv.acl_stats() == acl
        assert bool((srv.list_want == _lib.LIST_IDLE).all().item())
        assert srv.ev_total.cpu().tolist() == [0, 0]
        assert int(tree.counters[_lib.TC_ZXID].item()) >= zx
    # the same batch with its own table is served
    reps = [r for _, r in _serve(srv, gpu, conns)]
    errs = [r['err'] for r in reps]
    assert errs == ['OK', 'OK', 'OK', 'OK', 'OK', 'BAD_ARGUMENTS', 'NO_NODE',
                    'BAD_ARGUMENTS', 'BAD_ARGUMENTS', 'OK', 'OK']
    assert 'no' in reps[4]['children']


def test_dead_session_refuses_its_segment(gpu):
    from zkmi.server.sessions import GpuSessionTable
    srv = _server(gpu)
    tree = srv.tree
    tab = GpuSessionTable(tree, cap=64)
    sid = [tab.sid_of(k) for k in range(3)]
    for k in range(3):
        tab.sid[k] = sid[k]
        tab.state[k] = 1
    tab.next.fill_(3)
    tab.close(torch.tensor([sid[1]], dtype=I64, device=gpu))
    conns = _refused_conns()
    conns = [(sid[0],) + conns[0][1:], (sid[1],) + conns[1][1:],
             (sid[2],) + conns[2][1:]]
    census = tree.watch_census()
    reps = [r for _, r in _serve(srv, gpu, conns, table=tab)]
    assert srv.session_stats() == {'bad': 0, 'first_bad_segment': -1,
                                   'expired_segments': 1}
    # the dead segment: the malformed list frame and the unknown opcode too
    assert [r['err'] for r in reps[3:8]] == ['SESSION_EXPIRED'] * 5
    assert [r['xid'] for r in reps[3:8]] == [1, 2, 3, 4, 5]
    # the others are served
    assert [r['err'] for r in reps[:3]] == ['OK'] * 3
    assert [r['err'] for r in reps[8:]] == ['BAD_ARGUMENTS', 'OK', 'OK']
    # slots 0 and 63 armed one child watch each, slot 9 none
    assert tree.watch_census()[1] == census[1] + 2
    assert bool((srv.list_want == _lib.LIST_IDLE).all().item())
    d = ['/bench/d%06d' % k for k in range(3)]
    mk = [{'xid': 1 + k, 'opcode': 'CREATE', 'path': d[k] + '/later',
           'data': b'', 'acl': jute.DEFAULT_ACL, 'flags': []}
          for k in range(3)]
    reps = [r for _, r in _serve(srv, gpu, [(sid[2], 63, mk)], table=tab)]
    # (d1/no was refused with its segment: d1/later is that parent's first)
    assert [r['err'] for r in reps] == ['OK'] * 3
    assert _slot_slices(srv) == {0: [(CC, d[0])], 63: [(CC, d[2])]}
    # without a table every segment is served
    reps = [r for _, r in _serve(srv, gpu, conns)]
    assert [r['err'] for r in reps[3:8]] == ['OK', 'OK', 'BAD_ARGUMENTS',
                                             'NO_NODE', 'BAD_ARGUMENTS']


# ---- 5. the model -----------------------------------------------------------

def _acl_key(acl):
    return tuple((jute.perms_to_mask(a['perms']), a['id']['scheme'],
                  a['id']['id']) for a in acl)


def get_acl(path):
    return {'opcode': 'GET_ACL', 'path': path}


class MixSessModel(SessModel):
    """test_gpu_sessions.SessModel with ``ls`` and GET_ACL, under the batch
    contract: the fake server applies a batch's serve class first, then its
    GET_ACLs, then its lists (each in request order); the events are
    compared as multisets a watcher."""

    def _apply(self, p, sid, z, zxids):
        if p['opcode'] == 'GET_ACL':
            rep = self.db.handle(dict(p), sid)
            k = (p['xid'], rep['err'])
            if rep['err'] == 'OK':
                k += (self._stat_key(p['path'], zxids), _acl_key(rep['acl']))
            return k
        k = super()._apply(p, sid, z, zxids)
        if p['opcode'].startswith('GET_CHILDREN') and k[1] == 'OK':
            k += (tuple(sorted(self.db.nodes[p['path']].children)),)
        return k

    def refresh(self):
        """What the audit leaves for _apply's SET_DATA rule (a node's slot
        capacity), without the audit's reads."""
        nt = self._node_table()
        self.node_of = {p: v for v, p in enumerate(nt['paths'])
                        if p is not None}
        self.slot_cap = self.tree.slot_cap[:nt['n']].cpu().numpy()

    def _key(self, r):
        k = self._reply_key(r, False)
        if r['err'] == 'OK' and r['opcode'] == 'GET_ACL':
            k += (_acl_key(r['acl']),)
        if r['err'] == 'OK' and r['opcode'].startswith('GET_CHILDREN'):
            k += (tuple(sorted(r['children'])),)
        return k

    def serve_mixed(self, segs):
        srv = self.srv
        flat, rx, cuts, tab = self.build(segs)
        self.zxids_ok = False           # a mixed batch's zxids: not modelled
        base = self.counter(_lib.TC_ZXID)
        out, total, err, ft = srv.serve_sessions_mixed(
            _dev_bytes(rx, self.dev), len(rx), tab)
        assert int(err.item()) == 0
        assert int(ft.count.item()) == len(flat)
        raw = _raw(out, total.item())
        cls = [_class(jute.encode_request(p)) for _, p in flat]
        assert self.counter(_lib.TC_ZXID) == base + cls.count(A)
        assert srv.session_stats() == {'bad': 0, 'first_bad_segment': -1,
                                       'expired_segments': 0}
        off = srv.seg.rep_off.cpu().tolist()
        assert off[0] == 0 and off[-1] == len(raw) and off == sorted(off)
        got = []
        for s, (_, _, pk) in enumerate(segs):
            part = raw[off[s]:off[s + 1]]
            frames, used, bad = jute.scan_frames(part)
            assert bad < 0 and used == len(part) and len(frames) == len(pk)
            xmap = {p['xid']: p['opcode'] for p in pk}
            rs = [jute.decode_response(part[o:o + ln], xmap)
                  for o, ln in frames]
            assert [r['xid'] for r in rs] == list(range(1, len(pk) + 1))
            got += rs
        # the model: the serve class, then the GET_ACLs, then the lists
        want, writes, keys = [], [], [None] * len(flat)
        for c in (A, C, L):
            for i, (s, p) in enumerate(flat):
                if cls[i] != c:
                    continue
                lens = self._lens()
                k = self._apply(p, segs[s][0] or None, base + i + 1, False)
                keys[i] = k
                if k[1] == 'OK' and p['opcode'] in ('CREATE', 'DELETE'):
                    writes.append((i, k[2] if p['opcode'] == 'CREATE'
                                   else p['path']))
                self._since(lens, i, want)
        for i, (r, w) in enumerate(zip(got, keys)):
            g = self._key(r)
            assert g == w, 'request %d (segment %d) %r: got %r, want %r' % (
                i, flat[i][0], {k: v for k, v in flat[i][1].items()
                                if k != 'acl'}, g, w)
        sent = self.slot_events()
        assert srv.ev_total.cpu().tolist() == [len(want), len(want)]
        ws = srv.watch_stats()
        assert ws['encode_err'] == 0 and ws['lost_arms'] == 0, ws
        bad = check_events(sent, want, False, writes)
        assert bad is None, bad
        self.batches += 1
        self.events += len(want)
        return got, want


def test_model_churn(gpu):
    from zkmi.server.engine import GpuServer
    tree = _tree(gpu, acl_cap=512)
    m = MixSessModel(tree, GpuServer(tree, 1024, 1 << 21), gpu)
    rng = random.Random(31)
    slot_of = {}
    for w in (0, 31, 32, 63):
        slot_of[m.session(w)] = w
    sids = list(slot_of) + [m.session() for _ in range(4)]
    dirs = [dirp(d) for d in range(NDIR)]
    pool = _pool()
    sizes = [1, 63, 64, 65, 255, 256, 257] + [rng.randint(20, 150)
                                              for _ in range(25)]
    rng.shuffle(sizes)
    seen = collections.Counter()
    for n in sizes:
        fresh = iter(rng.sample(pool, n))
        reqs = []
        for _ in range(n):
            r = rng.random()
            if r < 0.6:
                p = _request(m, rng, next(fresh))
                if p['opcode'] == 'CREATE' and rng.random() < 0.3:
                    p['acl'] = ACL2
            elif r < 0.8:
                p = get_acl(rng.choice(
                    [rng.choice(pool), rng.choice(dirs), '/bench',
                     '/bench/nope']))
            else:
                p = ls(rng.choice([rng.choice(dirs[:POOL_DIRS + 2]),
                                   rng.choice(pool), '/bench/nope']),
                       watch=rng.random() < 0.6, stat=rng.random() < 0.5)
            reqs.append(p)
        segs, k = [], 0
        while k < n:
            size = min(n - k, rng.randint(0, 40))
            sid = rng.choice(sids)
            w = slot_of.get(sid, -1)
            pk = reqs[k:k + size]
            for p in pk:
                if w < 0 and 'watch' in p:
                    p['watch'] = False
                elif w >= 0 and p['opcode'] in ('GET_DATA', 'EXISTS'):
                    p['watch'] = rng.random() < 0.5
            segs.append((sid, w, pk))
            k += size
        got, want = m.serve_mixed(segs)
        for r in got:
            seen[(r['opcode'], r['err'])] += 1
        seen['events'] += len(want)
        if m.batches % 12 == 0:
            m.audit(zxids=False)
        else:
            m.refresh()
    assert m.batches >= 30
    # the churn did exercise what it is about
    for key in (('GET_ACL', 'OK'), ('GET_ACL', 'NO_NODE'),
                ('GET_CHILDREN', 'OK'), ('GET_CHILDREN2', 'OK'),
                ('GET_CHILDREN2', 'NO_NODE'), ('CREATE', 'OK'),
                ('DELETE', 'OK'), ('SET_DATA', 'OK')):
        assert seen[key] > 0, (key, seen)
    assert seen['events'] > 20, seen
    assert m.events == seen['events']
    m.touched |= set(dirs)
    m.audit(zxids=False)            # the tree audit and _audit_lists
    assert m.srv.acl_stats()[2] == 0


# ---- 6. edges ---------------------------------------------------------------

def test_tree_without_acl_table(gpu):
    srv = _server(gpu, acl=False)
    pk = _batch(np.array([A, C, L] * 20), 10, 0)
    conns = [(0x51, 1, pk[:25]), (0x52, -1, []), (0x53, 2, pk[25:])]
    reps = _serve(srv, gpu, conns)
    for p, (f, r) in zip(pk, reps):
        if p['opcode'] == 'GET_ACL':
            assert r['err'] == 'UNIMPLEMENTED' and len(f) == 20
    assert sum(r['err'] == 'OK' for _, r in reps) > 25
    assert bool((srv.mix_cls[:60] != C).all().item())


def test_overflow_and_max_frame(gpu):
    srv = _server(gpu, 300)
    pk = _read_only(300, 40)
    conns = [(0, -1, pk[:13]), (0, -1, pk[13:14]), (0, -1, pk[14:])]
    parts = [_stream(p) for _, _, p in conns]
    rx = _dev_bytes(b''.join(parts), gpu)
    cuts = [0] + [int(x) for x in np.cumsum([len(b) for b in parts])]
    segs = _segments(gpu, cuts, [0, 0, 0], [-1, -1, -1])
    _, total, err, _ = srv.serve_sessions_mixed(rx, rx.numel(), segs)
    T = int(total.item())
    assert int(err.item()) == 0 and T > 10 * 300 * 14
    assert srv.seg.rep_off.cpu().tolist()[-1] == T
    out = torch.full((T - 1,), 0xAB, dtype=U8, device=gpu)
    o, total, err, _ = srv.serve_sessions_mixed(rx, rx.numel(), segs, out=out)
    assert o is out and int(err.item()) == 2 and int(total.item()) == 0
    assert bool((out == 0xAB).all().item())
    assert srv.seg.rep_off.cpu().tolist() == [0, 0, 0, 0]
    out = torch.full((T + 4,), 0xAB, dtype=U8, device=gpu)
    o, total, err, _ = srv.serve_sessions_mixed(rx, rx.numel(), segs, out=out,
                                                terminate=True)
    assert int(err.item()) == 0 and int(total.item()) == T
    assert out[T:].cpu().tolist() == [0xFF] * 4
    whole = _replies(out, total, pk)
    # max_frame: the one large list of connection 1 is demoted, the small
    # replies around it are whole
    assert pk[13]['opcode'] == 'GET_CHILDREN2'
    srv = _server(gpu, 300)
    small = [p for p in pk if p['opcode'] != 'GET_CHILDREN2']
    conns = [(0, -1, small[:10]), (0, -1, [pk[13]]), (0, -1, small[10:])]
    reps = _serve(srv, gpu, conns, max_frame=256)
    flat = [p for _, _, c in conns for p in c]
    by = {r['xid']: (f, r) for f, r in whole}
    for p, (f, r) in zip(flat, reps):
        fw, rw = by[p['xid']]
        if p['opcode'] == 'GET_CHILDREN2':
            assert r['err'] == 'SYSTEM_ERROR' and len(f) == 20
            assert len(rw['children']) == 300
        else:
            assert r['err'] == 'OK' and len(f) == len(fw)
            assert dict(_norm(r), zxid=0) == dict(_norm(rw), zxid=0)
    off = srv.seg.rep_off.cpu().tolist()
    assert off[2] - off[1] == 20


def test_empty_batch_with_terminator(gpu):
    srv = _server(gpu)
    rx = torch.zeros(64, dtype=U8, device=gpu)
    for segs in (_segments(gpu, [0, 0], [0], [-1]),
                 _segments(gpu, [0, 0, 0, 0], [5, 6, 7], [1, 2, 3])):
        out, total, err, ft = srv.serve_sessions_mixed(rx, 0, segs,
                                                       terminate=True)
        assert int(total.item()) == 0 and int(err.item()) == 0
        assert int(ft.count.item()) == 0
        assert out[:4].cpu().tolist() == [0xFF] * 4
        assert srv.seg.rep_off.cpu().tolist() == [0] * (segs.S + 1)
        assert srv.notif_slots[1].cpu().tolist() == [0] * 65
        # and after a batch that left rows in every table
        _serve(srv, gpu, [(0, -1, _batch(np.array([A, C, L] * 5), 10, 0))])


def test_interface_refusals(gpu):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    rx = torch.zeros(64, dtype=U8, device=gpu)
    segs = _segments(gpu, [0, 0], [0], [-1])
    tree = GpuTree(100, 16, fanout=10, device=gpu)
    srv = GpuServer(tree, 64, 1 << 16, seq_order=False, fused_rows=True)
    with pytest.raises(ValueError):
        srv.serve_sessions_mixed(rx, 0, segs)
    srv = GpuServer(GpuTree(100, 16, fanout=10, device=gpu), 64, 1 << 16)
    srv.read_only = True
    with pytest.raises(ValueError):
        srv.serve_sessions_mixed(rx, 0, segs)
    tree = GpuTree(100, 16, fanout=10, device=gpu, shard=(0, 2))
    srv = GpuServer(tree, 64, 1 << 16)
    with pytest.raises(ValueError, match='sharded'):
        srv.serve_sessions_mixed(rx, 0, segs)
    srv = GpuServer(GpuTree(100, 16, fanout=10, device=gpu), 64, 1 << 16)
    with pytest.raises(TypeError):
        srv.serve_sessions_mixed(rx, 0, None)


def test_capture_replay(gpu):
    """After a warm-up call a read-only batch of three connections is
    captured on one stream and replayed three times: the decoded replies and
    the rep_off slices of every replay equal the eager ones (the header's
    zxid apart, which the serve advances by its 25 requests a batch)."""
    srv = _server(gpu)
    pk = _read_only(10, 97)
    conns = [(0, 3, pk[:40]), (0, -1, []), (0, 4, pk[40:])]
    parts = [_stream(p) for _, _, p in conns]
    rx = _dev_bytes(b''.join(parts), gpu)
    cuts = [0] + [int(x) for x in np.cumsum([len(b) for b in parts])]
    segs = _segments(gpu, cuts, [0, 0, 0], [3, -1, 4])
    n_serve = sum(p['opcode'] == 'GET_DATA' for p in pk)
    first = [_norm(r) for _, r in _serve(srv, gpu, conns, terminate=True)]
    eager = [dict(r, zxid=0) for r in first]
    rep_off = srv.seg.rep_off.cpu().tolist()
    zxid = first[0]['zxid']
    torch.cuda.synchronize(gpu)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        out, total, err, _ = srv.serve_sessions_mixed(rx, rx.numel(), segs,
                                                      terminate=True)
    for _ in range(3):
        out.fill_(0)
        srv.seg.rep_off.fill_(-1)
        g.replay()
        torch.cuda.synchronize(gpu)
        assert int(err.item()) == 0
        got = [_norm(r) for _, r in _replies(out, total, pk)]
        zxid += n_serve
        assert [r['zxid'] for r in got] == [
            zxid if p['opcode'] == 'GET_DATA' else zxid + n_serve
            for p in pk]
        assert [dict(r, zxid=0) for r in got] == eager
        T = int(total.item())
        assert out[T:T + 4].cpu().tolist() == [0xFF] * 4
        assert srv.seg.rep_off.cpu().tolist() == rep_off


def test_ops_check_their_tensors(gpu):
    """Each new op raises on a wrong dtype, a CPU tensor and a short table;
    nothing is launched for them."""
    srv = _server(gpu, frames=16)
    tree = srv.tree
    srv._mix_buffers()
    S, cap = 3, 16
    z64 = lambda n: torch.zeros(n, dtype=I64, device=gpu)     # noqa: E731
    z32 = lambda n: torch.zeros(n, dtype=I32, device=gpu)     # noqa: E731
    z8 = lambda n: torch.zeros(n, dtype=U8, device=gpu)       # noqa: E731

    def split(**kw):
        a = dict(f_seg=z32(cap), cls=z32(cap), sub=z32(cap), count=z64(1),
                 f_seg_c=[z32(cap), z32(cap), z32(cap)])
        a.update(kw)
        _lib.sess_split_segments(a['f_seg'], a['cls'], a['sub'], a['count'],
                                 cap, a['f_seg_c'])

    split()
    for name, wrong in (('f_seg', z64(cap)), ('f_seg', z32(cap - 1)),
                        ('f_seg', z32(cap).cpu()), ('cls', z32(cap - 1)),
                        ('cls', z64(cap)), ('sub', z32(cap).cpu()),
                        ('sub', z32(2 * cap)[::2]), ('count', z32(1)),
                        ('f_seg_c', [z32(cap), z32(cap)]),
                        ('f_seg_c', [z32(cap), z32(cap - 1), z32(cap)]),
                        ('f_seg_c', [z32(cap), z32(cap), z64(cap)]),
                        ('f_seg_c', [z32(cap).cpu(), z32(cap), z32(cap)])):
        with pytest.raises(RuntimeError):
            split(**{name: wrong})
    rx = z8(64)

    def lists(**kw):
        a = dict(f_seg=z32(cap), sessions=z64(S), wslots=z32(S),
                 seg_state=z32(S), bad=z64(2), want=srv.list_want, rec_off=z64(cap), out=z8(4096))
        a.update(kw)
        _lib.tree_list_sessions(
            tree.tensors, rx, z64(cap), z32(cap), z64(1), cap,
            [a['f_seg'], a['sessions'], a['wslots'], a['seg_state'],
             a['bad']], 1 << 20, a['want'],
            srv.list_ws, a['out'], 4096, a['rec_off'], z64(1), z32(1))

    lists()
    for name, wrong in (('f_seg', z32(cap - 1)), ('f_seg', z64(cap)),
                        ('f_seg', z32(cap).cpu()), ('wslots', z64(S)),
                        ('wslots', z32(0)), ('wslots', z32(S).cpu()),
                        ('seg_state', z32(S - 1)), ('seg_state', z64(S)),
                        ('bad', z64(1)), ('bad', z32(2)),
                        ('bad', z64(2).cpu()), ('rec_off', z64(cap - 1)),
                        ('out', z8(4095)),
                        ('want', srv.list_want[:-1])):
        with pytest.raises(RuntimeError):
            lists(**{name: wrong})
    assert bool((srv.list_want == _lib.LIST_IDLE).all().item())

    def acls(**kw):
        a = dict(f_seg=z32(cap), sessions=z64(S), wslots=z32(S),
                 seg_state=z32(S), bad=z64(2), rec_off=z64(cap),
                 out=z8(4096), ws=srv._acl_workspace())
        a.update(kw)
        _lib.tree_acl_get_sessions(
            tree.tensors, tree.acl, rx, z64(cap), z32(cap), z64(1), cap,
            [a['f_seg'], a['sessions'], a['wslots'], a['seg_state'],
             a['bad']], a['ws'], a['out'], 4096,
            a['rec_off'], z64(1), z32(1))

    acls()
    for name, wrong in (('f_seg', z32(cap - 1)), ('f_seg', z64(cap)),
                        ('f_seg', z32(cap).cpu()), ('seg_state', z32(0)),
                        ('seg_state', z64(S)), ('seg_state', z32(S).cpu()),
                        ('bad', z64(1)), ('bad', z32(2)),
                        ('rec_off', z64(cap - 1)), ('out', z8(100)),
                        ('ws', srv._acl_workspace()[:-16])):
        with pytest.raises(RuntimeError):
            acls(**{name: wrong})
