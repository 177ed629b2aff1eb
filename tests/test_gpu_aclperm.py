"""GpuServer.serve_sessions_mixed(perms=...): the ACLs the tree keeps are
enforced (csrc/kernels/tree_aclperm.hip; the rule: csrc/kernels/zk_aclperm.h,
mirrored by tests/aclperm_model.py).

Every tree here has an ACL table and, under the static directory
/bench/d000000, nodes created with these vectors: the open ACL, READ only, all
but CREATE, all but DELETE, all but WRITE, all but READ, everything for
ip:10.1.2.0/24 alone; a second kind of tree has a store of two vectors, so the
third one's binding is lost.  time.time is frozen so twin trees' Stats compare
exactly.

The verdict's carrier: a denied frame's opcode word is overwritten with an
opcode of no request, which the serve answers BAD_ARGUMENTS, header only (as
it answers such an opcode sent by a client: test_gpu_sessions_mixed.py), and
the fix-up turns exactly the marked frames' BAD_ARGUMENTS into NO_AUTH."""

import struct
import time

import numpy as np
import pytest
import torch

import aclperm_model as A

from zkmi import jute
from zkmi.ops import _lib

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000.0
I64, I32, U8 = torch.int64, torch.int32, torch.uint8
D = '/bench/d000000'
NET, OUT, NONE = A.addr_of('10.1.2.9'), A.addr_of('10.1.3.9'), 0
NO_AUTH_FRAME = struct.Struct('>iiqi')


def world(perms):
    return [{'perms': perms, 'id': {'scheme': 'world', 'id': 'anyone'}}]


OPEN = world(A.ALL)
VEC = {
    'open': OPEN,
    'ro': world(A.READ),
    'nocreate': world(A.ALL & ~A.CREATE),
    'nodelete': world(A.ALL & ~A.DELETE),
    'nowrite': world(A.ALL & ~A.WRITE),
    'noread': world(A.ALL & ~A.READ),
    'ipnet': [{'perms': A.ALL, 'id': {'scheme': 'ip', 'id': '10.1.2.0/24'}}],
}


@pytest.fixture(autouse=True)
def _frozen_time(monkeypatch):
    monkeypatch.setattr(time, 'time', lambda: NOW)


def wire(acl):
    w = jute.JuteWriter()
    w.write_acl(acl)
    return bytes(w.getvalue())


def mk(path, acl=OPEN, flags=()):
    return {'opcode': 'CREATE', 'path': path, 'data': b'c', 'acl': acl,
            'flags': list(flags)}


def rd(path, watch=False, op='GET_DATA'):
    return {'opcode': op, 'path': path, 'watch': watch}


def wr(path, version=-1):
    return {'opcode': 'SET_DATA', 'path': path, 'data': b'w',
            'version': version}


def rm(path, version=-1):
    return {'opcode': 'DELETE', 'path': path, 'version': version}


def leaf(i):
    return '/bench/d%06d/n%09d' % (i // 10, i)


def _server(gpu, acl_cap=512, frames=1024):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(400, 16, fanout=10, device=gpu, spare=4.0,
                   ctime_ms=int(NOW * 1000), acl_cap=acl_cap, watch_cap=2048,
                   scratch=1 << 20)
    return GpuServer(tree, frames, 1 << 20, window=512)


def _dev(b, dev):
    a = np.frombuffer(bytes(b) if b else b'\0', np.uint8).copy()
    return torch.from_numpy(a).to(dev)


def _body(p):
    return p['raw'] if 'raw' in p else jute.encode_request(p)


class Batch(object):
    """One serve_sessions_mixed batch.  ``conns``: [(addr, watcher slot,
    [packet, ...])], a connection a segment; xids are the frames' indices.
    ``addrs`` None: ``perms=None``."""

    def __init__(self, srv, gpu, conns, enforce=True, sessions=None,
                 starts=None, **kw):
        from zkmi.server.engine import AclIdentity, SessionSegments
        self.flat = [p for _, _, pk in conns for p in pk]
        for x, p in enumerate(self.flat):
            p['xid'] = x
            if 'raw' in p and len(p['raw']) >= 4:
                p['raw'] = struct.pack('>i', x) + p['raw'][4:]
        parts = [b''.join(jute.frame(_body(p)) for p in pk)
                 for _, _, pk in conns]
        self.parts = parts
        rx = b''.join(parts)
        cuts = [0] + [int(x) for x in np.cumsum([len(b) for b in parts])]
        S = len(conns)
        segs = SessionSegments(
            torch.tensor(cuts if starts is None else starts, dtype=I64,
                         device=gpu),
            torch.tensor(sessions or [0x100 + s for s in range(S)],
                         dtype=I64, device=gpu),
            torch.tensor([w for _, w, _ in conns], dtype=I32, device=gpu))
        perms = AclIdentity(torch.tensor(
            [A.as_i32(a) for a, _, _ in conns], dtype=I32, device=gpu)) \
            if enforce else None
        self.zxid = int(srv.tree.counters[_lib.TC_ZXID].item())
        self.rx = _dev(rx, gpu)
        self.rx_sent = rx
        out, total, err, ft = srv.serve_sessions_mixed(
            self.rx, len(rx), segs, perms=perms, **kw)
        assert int(err.item()) == 0
        assert int(ft.count.item()) == len(self.flat)
        self.raw = bytes(out[:int(total.item())].cpu().numpy().tobytes())
        frames, used, bad = jute.scan_frames(self.raw)
        assert bad < 0 and used == len(self.raw)
        assert len(frames) == len(self.flat)
        self.frames = [self.raw[o - 4:o + ln] for o, ln in frames]
        self.reps = [jute.decode_response(
            f[4:], {p['xid']: p.get('opcode', 'PING')})
            for f, p in zip(self.frames, self.flat)]
        assert [r['xid'] for r in self.reps] == list(range(len(self.flat)))
        self.errs = [r['err'] for r in self.reps]
        self.rep_off = srv.seg.rep_off.cpu().tolist()

    def notes(self, srv):
        """{watcher slot: sorted [(type, path)]} of the batch's events."""
        buf, total, slots, count = srv.notif
        raw = bytes(buf[:int(total.item())].cpu().numpy().tobytes())
        off = srv.notif_slots[1].cpu().tolist()
        out = {}
        for w in range(64):
            part = raw[off[w]:off[w + 1]]
            got = []
            for o, ln in jute.scan_frames(part)[0]:
                pkt = jute.decode_response(part[o:o + ln], {})
                got.append((pkt['type'], pkt['path']))
            if got:
                out[w] = sorted(got)
        return out, raw


def _world(gpu, acl_cap=512, frames=1024):
    """A server whose tree holds D/<name> for every vector of VEC, each with a
    child ``kid`` (open ACL), made without enforcement."""
    srv = _server(gpu, acl_cap, frames)
    b = Batch(srv, gpu, [(0, -1, [mk('%s/%s' % (D, k), v)
                                  for k, v in VEC.items()])], enforce=False)
    assert b.errs == ['OK'] * len(VEC)
    b = Batch(srv, gpu, [(0, -1, [mk('%s/%s/kid' % (D, k)) for k in VEC])],
              enforce=False)
    assert b.errs == ['OK'] * len(VEC)
    assert srv.acl_stats()[2] == 0
    return srv


def _is_no_auth(b, i):
    """Frame i's reply is exactly be32(16), xid, zxid, be32(-102)."""
    return b.frames[i] == NO_AUTH_FRAME.pack(16, i, b.zxid, A.NO_AUTH)


# ---- (a) a batch that is permitted everything -------------------------------

def _permitted(n, S, gen):
    """n frames over S connections (addresses NET / OUT / none in turn), every
    one allowed by the ACL it meets.  No two frames of a batch touch one node
    with a writer among them (the unordered serve's batch is concurrent), and
    what generation 0 watches generation 1 writes."""
    addrs = [(NET, OUT, NONE)[s % 3] for s in range(S)]
    pks = [[] for _ in range(S)]
    for i in range(n):
        s = (i * S) // n if n >= S else i
        net = addrs[s] == NET
        k = (i + gen) % 11
        j = i // 11
        u = 'g%dn%d' % (gen, i)
        pks[s].append([
            rd(leaf(20 + i), watch=True) if j % 2 == 0 else
            rd(D + '/ro', watch=True),
            wr(leaf(20 + i)),
            mk('%s/open/%s' % (D, u)),
            mk('%s/%s/s-' % (D, 'ipnet' if net else 'nowrite'),
               flags=['SEQUENTIAL']),
            rm(leaf(330 + j + 30 * gen)),
            rd(D if not net else D + '/ipnet', op='GET_CHILDREN2'),
            {'opcode': 'GET_ACL', 'path': D + '/ro'},
            rd(D + '/nocreate', watch=True, op='EXISTS'),
            wr(D + '/noread') if j == 0 else wr(leaf(20 + i)),
            mk('%s/nodelete/%s' % (D, u), VEC['ro']),
            {'opcode': 'PING'}][k])
    return [(addrs[s], (5 * s) % 64, pks[s]) for s in range(S)]


@pytest.mark.parametrize('n,S', [(1, 1), (64, 3), (65, 70), (256, 3),
                                 (257, 70)])
def test_all_permitted_equals_unenforced(gpu, n, S):
    sx, sy = _world(gpu), _world(gpu)
    for gen in range(2):
        x = Batch(sx, gpu, _permitted(n, S, gen))
        y = Batch(sy, gpu, _permitted(n, S, gen), enforce=False)
        assert 'NO_AUTH' not in x.errs
        assert x.rx.cpu().numpy().tobytes()[:len(x.rx_sent)] == x.rx_sent
        for i, (fx, fy, p) in enumerate(zip(x.frames, y.frames, x.flat)):
            if p['opcode'] == 'GET_CHILDREN2':     # (the names' order is free)
                assert len(fx) == len(fy)
                assert sorted(x.reps[i]['children']) == \
                    sorted(y.reps[i]['children'])
            else:
                assert fx == fy, (gen, i, x.reps[i], y.reps[i])
        assert x.rep_off == y.rep_off
        (xn, xraw), (yn, yraw) = x.notes(sx), y.notes(sy)
        assert xn == yn and len(xraw) == len(yraw)
        assert bool(xn) == (gen == 1)
        assert sx.notif_slots[1].cpu().tolist() == \
            sy.notif_slots[1].cpu().tolist()
        assert sx.tree.digest() == sy.tree.digest()
        assert sx.tree.watch_census() == sy.tree.watch_census()
    st = sx.acl_enforce_stats()
    assert st['denied'] == 0 and st['denied_lost'] == 0
    assert st['checked'] > 0 or n == 1
    assert sy.acl_enforce_stats() == {'checked': 0, 'denied': 0,
                                      'denied_lost': 0}
    assert sx.acl_stats() == sy.acl_stats()


# ---- (b) denied frames ------------------------------------------------------

def _denied_writes():
    return [(OUT, 1, [wr(D + '/ro'), mk(D + '/nocreate/x'),
                      rm(D + '/nodelete/kid'), wr(D + '/ipnet'),
                      mk(D + '/ipnet/s-', flags=['SEQUENTIAL'])]),
            (NONE, 2, [wr(D + '/ipnet'), mk(D + '/ipnet/y'),
                       rm(D + '/ipnet/kid'), wr(D + '/nowrite', 0),
                       mk(D + '/ro/z', flags=['EPHEMERAL'])])]


def test_denied_writes_change_nothing(gpu):
    srv = _world(gpu)
    tree = srv.tree
    # watches a successful write of the batch below would fire
    arm = Batch(srv, gpu, [(NET, 9, [
        rd(D + '/ro', True), rd(D + '/ipnet', True), rd(D + '/nowrite', True),
        rd(D + '/nocreate/x', True, 'EXISTS'),
        rd(D + '/nodelete/kid', True), rd(D + '/ipnet/kid', True),
        rd(D + '/ipnet', True, 'GET_CHILDREN'),
        rd(D + '/nocreate', True, 'GET_CHILDREN2')])])
    assert set(arm.errs) <= {'OK', 'NO_NODE'} and arm.errs.count('OK') == 7
    dig, census = tree.digest(), tree.watch_census()
    before = srv.acl_enforce_stats()
    b = Batch(srv, gpu, _denied_writes())
    assert b.errs == ['NO_AUTH'] * 10
    for i in range(10):
        assert _is_no_auth(b, i), (i, b.frames[i])
    assert tree.digest() == dig
    assert tree.watch_census() == census
    assert srv.ev_total.cpu().tolist() == [0, 0]
    assert b.notes(srv) == ({}, b'')
    after = srv.acl_enforce_stats()
    assert after['checked'] - before['checked'] == 10
    assert after['denied'] - before['denied'] == 10
    assert after['denied_lost'] == 0
    # the denied frames' opcode words, and nothing else, were overwritten
    got = b.rx.cpu().numpy().tobytes()[:len(b.rx_sent)]
    want = bytearray(b.rx_sent)
    for o, _ in jute.scan_frames(b.rx_sent)[0]:
        want[o + 4:o + 8] = struct.pack('>i', -1000)
    assert got == bytes(want)
    # the same batch from inside the network: only the ip node opens up
    b = Batch(srv, gpu, [(NET, w, pk) for _, w, pk in _denied_writes()])
    assert b.errs == ['NO_AUTH', 'NO_AUTH', 'NO_AUTH', 'OK', 'OK',
                      'OK', 'OK', 'OK', 'NO_AUTH', 'NO_AUTH']
    assert b.reps[4]['path'].startswith(D + '/ipnet/s-')
    assert 9 in b.notes(srv)[0]


def test_denied_read_arms_nothing(gpu):
    srv = _world(gpu)
    census = srv.tree.watch_census()
    b = Batch(srv, gpu, [
        (NET, 5, [rd(D + '/noread', True),
                  rd(D + '/noread', True, 'GET_CHILDREN'),
                  rd(D + '/noread', True, 'GET_CHILDREN2')]),
        (OUT, 6, [rd(D + '/noread', True, 'EXISTS')])])
    assert b.errs == ['NO_AUTH'] * 3 + ['OK']
    assert all(_is_no_auth(b, i) for i in range(3))
    # (slot 6's EXISTS needs no permission: one watch was armed)
    assert srv.tree.watch_census()[1] == census[1] + 1
    b = Batch(srv, gpu, [(OUT, 7, [wr(D + '/noread')]),
                         (OUT, 8, [mk(D + '/noread/new')])])
    assert b.errs == ['OK', 'OK']
    notes = b.notes(srv)[0]
    assert 5 not in notes
    assert notes == {6: [('DATA_CHANGED', D + '/noread')]}


def test_lost_binding_denies(gpu):
    """A store of two vectors: the third distinct one's binding is lost, and
    a lost binding denies whoever asks, counted apart."""
    srv = _server(gpu, acl_cap=2)
    b = Batch(srv, gpu, [(0, -1, [mk(D + '/a', VEC['ro']),
                                  mk(D + '/b', VEC['nowrite'])])],
              enforce=False)
    assert b.errs == ['OK', 'OK']
    b = Batch(srv, gpu, [(0, -1, [mk(D + '/lost', VEC['ipnet'])])],
              enforce=False)
    assert b.errs == ['OK'] and srv.acl_stats()[2] == 1
    b = Batch(srv, gpu, [(NET, 3, [
        rd(D + '/lost', True), wr(D + '/lost'), mk(D + '/lost/c'),
        rd(D + '/lost', False, 'GET_CHILDREN'), rd(D + '/lost', True,
                                                   'EXISTS'),
        rd(D + '/a'), wr(D + '/a'), wr(leaf(3))])])
    assert b.errs == ['NO_AUTH'] * 4 + ['OK', 'OK', 'NO_AUTH', 'OK']
    assert srv.acl_enforce_stats() == {'checked': 7, 'denied': 5,
                                       'denied_lost': 4}


# ---- (c) where the verdict stands among the others --------------------------

def test_verdict_precedence(gpu):
    srv = _world(gpu)
    b = Batch(srv, gpu, [(OUT, -1, [
        mk(D + '/nocreate/kid'),            # exists, and no CREATE
        rm(D + '/nodelete/missing'),        # no node, under a no-DELETE parent
        wr(D + '/nowrite', version=99),     # bad version, and no WRITE
        rm(D + '/nodelete'),                # not empty; D allows the DELETE
        mk(D + '/open/kid'),                # exists, allowed
        wr(D + '/ro/nope'),                 # no node
        mk(D + '/nope/x'),                  # no parent
        wr(D + '/open', version=99),        # bad version, allowed
        rm(D + '/nodelete/kid', 99)])])     # bad version, and no DELETE
    assert b.errs == ['NO_AUTH', 'NO_NODE', 'NO_AUTH', 'NOT_EMPTY',
                      'NODE_EXISTS', 'NO_NODE', 'NO_NODE', 'BAD_VERSION',
                      'NO_AUTH']


# ---- (d) frames that get no verdict -----------------------------------------

def _no_verdict_conns():
    garbage = {'opcode': 'PING',
               'raw': struct.pack('>ii', 0, 9999) + b'\0' * 8}
    # a SET_DATA of a no-WRITE node cut short: parse_request rejects it
    cut = {'opcode': 'SET_DATA',
           'raw': jute.encode_request(dict(wr(D + '/ro'), xid=0))[:-3]}
    return garbage, [(OUT, 1, [wr(D + '/ro'), garbage, rd(leaf(1))]),
                     (OUT, 2, [wr(D + '/ro'), mk(D + '/nocreate/q'),
                               rd(D + '/noread', op='GET_CHILDREN')]),
                     (OUT, 3, [cut, rd(leaf(2))])]


def test_garbage_opcode_keeps_the_serves_answer(gpu):
    """An opcode of no request sent by the client: parse_request rejects it,
    so it gets no verdict and keeps what the serve answers without
    enforcement (BAD_ARGUMENTS, as test_gpu_sessions_mixed.py pins it), next
    to a denied frame whose carrier is that very code."""
    sx, sy = _world(gpu), _world(gpu)
    x = Batch(sx, gpu, _no_verdict_conns()[1])
    y = Batch(sy, gpu, _no_verdict_conns()[1], enforce=False)
    assert x.errs == ['NO_AUTH', 'BAD_ARGUMENTS', 'OK', 'NO_AUTH', 'NO_AUTH',
                      'NO_AUTH', 'BAD_ARGUMENTS', 'OK']
    assert y.errs == ['OK', 'BAD_ARGUMENTS', 'OK', 'OK', 'OK', 'OK',
                      'BAD_ARGUMENTS', 'OK']
    assert x.frames[1] == y.frames[1] and len(x.frames[1]) == 20
    assert sx.acl_enforce_stats() == {'checked': 6, 'denied': 4,
                                      'denied_lost': 0}


def test_dead_segment_and_unsound_table(gpu):
    from zkmi.server.sessions import GpuSessionTable
    srv = _world(gpu)
    tree = srv.tree
    tab = GpuSessionTable(tree, cap=64)
    sid = [tab.sid_of(k) for k in range(3)]
    for k in range(3):
        tab.sid[k] = sid[k]
        tab.state[k] = 1
    tab.next.fill_(3)
    tab.close(torch.tensor([sid[1]], dtype=I64, device=gpu))
    _, conns = _no_verdict_conns()
    conns[2][2].pop(0)
    b = Batch(srv, gpu, conns, sessions=sid, table=tab)
    assert b.errs == ['NO_AUTH', 'BAD_ARGUMENTS', 'OK'] + \
        ['SESSION_EXPIRED'] * 3 + ['OK']
    assert srv.acl_enforce_stats() == {'checked': 3, 'denied': 1,
                                       'denied_lost': 0}
    # an unsound table (a torn frame): SYSTEMERROR for all, no verdict, and
    # rx as it came
    _, conns = _no_verdict_conns()
    conns[2][2].pop(0)
    lens = [sum(len(jute.frame(_body(dict(p, xid=0)))) for p in pk)
            for _, _, pk in conns]
    starts = [0, lens[0] + 2, lens[0] + lens[1], sum(lens)]
    dig = tree.digest()
    b = Batch(srv, gpu, conns, starts=starts)
    assert b.errs == ['SYSTEM_ERROR'] * 7
    assert srv.session_stats()['bad'] > 0
    assert b.rx.cpu().numpy().tobytes()[:len(b.rx_sent)] == b.rx_sent
    assert tree.digest() == dig
    assert srv.acl_enforce_stats() == {'checked': 3, 'denied': 1,
                                       'denied_lost': 0}


def test_arguments(gpu):
    from zkmi.server.engine import (AclIdentity, GpuServer, SessionSegments)
    from zkmi.server.tree import GpuTree
    srv = _world(gpu)
    rx = _dev(jute.frame(jute.encode_request(dict(rd(leaf(1)), xid=1))), gpu)
    segs = SessionSegments(torch.tensor([0, rx.numel()], dtype=I64,
                                        device=gpu),
                           torch.zeros(1, dtype=I64, device=gpu),
                           torch.full((1,), -1, dtype=I32, device=gpu))
    two = AclIdentity(torch.zeros(2, dtype=I32, device=gpu))
    with pytest.raises(ValueError):
        srv.serve_sessions_mixed(rx, rx.numel(), segs, perms=two)
    with pytest.raises(ValueError):
        AclIdentity(torch.zeros(1, dtype=I64, device=gpu))
    bare = GpuServer(GpuTree(400, 16, fanout=10, device=gpu, watch_cap=64),
                     64, 1 << 16)
    one = AclIdentity(torch.zeros(1, dtype=I32, device=gpu))
    with pytest.raises(ValueError):
        bare.serve_sessions_mixed(rx, rx.numel(), segs, perms=one)
    # the op's own checks: a wrong dtype and a short table
    L = _lib.lib()
    srv.serve_sessions_mixed(rx, rx.numel(), segs, perms=one)
    ft = srv.result[3]
    tab = srv.seg.table(segs)
    good = (srv.tree.tensors, srv.tree.acl, rx, ft.off, ft.length, ft.count,
            srv.cap_frames, tab, one.addrs, srv.acl_deny, srv.acl_enf)
    for k, bad in ((8, one.addrs.to(I64)), (8, two.addrs),
                   (9, srv.acl_deny[:8]), (10, srv.acl_enf.to(I32)),
                   (2, rx.cpu())):
        args = list(good)
        args[k] = bad
        with pytest.raises(RuntimeError):
            L.aclperm_check(*args)
    with pytest.raises(RuntimeError):
        L.aclperm_fix(srv.acl_deny, srv.mix_cls.to(I64), srv.mix_sub,
                      ft.count, srv.cap_frames, srv.resp.err, srv.acl_enf)


# ---- (e) SEQUENTIAL numbering -----------------------------------------------

@pytest.mark.parametrize('ordered', [False, True])
def test_denied_sequential_creates_take_no_number(gpu, ordered):
    srv = _world(gpu)
    names = []
    for gen in range(2):
        conns = [((NET, OUT)[s % 2], -1,
                  [mk(D + '/ipnet/s-', flags=['SEQUENTIAL'])
                   for _ in range(3)]) for s in range(6)]
        b = Batch(srv, gpu, conns, ordered=ordered)
        for i, (e, r) in enumerate(zip(b.errs, b.reps)):
            if (i // 3) % 2 == 0:
                assert e == 'OK', (gen, i, e)
                names.append(r['path'])
            else:
                assert e == 'NO_AUTH' and _is_no_auth(b, i), (gen, i, e)
    assert len(names) == 18 and len(set(names)) == 18
    nums = sorted(int(p[len(D + '/ipnet/s-'):]) for p in names)
    # (the parent had one child before: its cversion was 1; no gap, so no
    # denied create took a number)
    assert nums == list(range(1, 19))


# ---- (f) ordered, with deferral ---------------------------------------------

def test_denied_frame_defers_nothing(gpu):
    """Connections 0 and 2 (inside the network) set D/ipnet: ranks 0, 1 and
    2, so with two passes connection 2's set is deferred.  Connection 1's set
    of the same node, between them in batch order, is denied: it has no rank,
    it is not deferred and it defers nothing — everything the deferral leaves
    is what it leaves with a PING of the same length in that frame's place."""
    from zkmi.server.engine import OrderDefer
    X = D + '/ipnet'

    def conns(denied):
        return [(NET, 1, [wr(X), wr(X)]),
                (OUT, 2, [denied, rd(leaf(5))]),
                (NET, 3, [wr(X), rd(leaf(6))])]
    n = len(jute.encode_request(dict(wr(X), xid=2)))
    ping = {'opcode': 'PING',
            'raw': struct.pack('>ii', 2, 11) + b'\0' * (n - 8)}
    sx, sy = _world(gpu), _world(gpu)
    dx, dy = OrderDefer(3, gpu), OrderDefer(3, gpu)
    x = Batch(sx, gpu, conns(wr(X)), ordered=True, passes=2, defer=dx)
    y = Batch(sy, gpu, conns(ping), enforce=False, ordered=True, passes=2,
              defer=dy)
    assert [len(p) for p in x.parts] == [len(p) for p in y.parts]
    assert x.errs[:4] == ['OK', 'OK', 'NO_AUTH', 'OK']
    assert y.errs[:4] == ['OK', 'OK', 'OK', 'OK']
    assert _is_no_auth(x, 2)
    for a, b in ((dx.clipf, dy.clipf), (dx.rep_end, dy.rep_end),
                 (dx.used, dy.used), (dx.deferred, dy.deferred)):
        assert a.cpu().tolist() == b.cpu().tolist()
    assert int(dx.deferred.item()) == 2
    assert dx.used.cpu().tolist() == [len(x.parts[0]), len(x.parts[1]), 0]
    assert x.rep_off == y.rep_off
    assert dx.rep_end.cpu().tolist() == [x.rep_off[1], x.rep_off[2],
                                         x.rep_off[2]]
    assert sx.order_stats() == sy.order_stats()
    assert sx.tree.digest() == sy.tree.digest()


# ---- (g) the oracle ---------------------------------------------------------

def _random_acl(rng):
    schemes = ['world', 'ip', 'digest', 'auth']
    ids = {'world': ['anyone', 'anyone', 'nobody', ''],
           'ip': ['10.1.2.0/24', '10.1.2.9', '10.1.3.9/32', '10.0.0.0/8',
                  '0.0.0.0/0', '10.1.2', '10.1.2.300/24', '10.1.3.0/33'],
           'digest': ['u:pw'], 'auth': ['']}
    out = []
    for _ in range(int(rng.integers(1, 4))):
        s = schemes[int(rng.integers(len(schemes)))]
        out.append({'perms': int(rng.integers(0, 32)),
                    'id': {'scheme': s,
                           'id': ids[s][int(rng.integers(len(ids[s])))]}})
    return out


def test_oracle_random_frames(gpu):
    """2 000 random frames against 40 random vectors: per frame the verdict
    is the mirror's, over the tree as the batch finds it, and the counters
    are the mirror's counts."""
    rng = np.random.default_rng(5)
    srv = _server(gpu)
    nodes = ['%s/v%02d' % (D, k) for k in range(40)]
    acls = [_random_acl(rng) for _ in nodes]
    b = Batch(srv, gpu, [(0, -1, [mk(p, a) for p, a in zip(nodes, acls)])],
              enforce=False)
    assert b.errs == ['OK'] * 40
    b = Batch(srv, gpu, [(0, -1, [mk(p + '/kid') for p in nodes])],
              enforce=False)
    assert b.errs == ['OK'] * 40 and srv.acl_stats()[2] == 0
    # what exists, and every node's vector in wire form (static ones: open)
    vec = {p: wire(a) for p, a in zip(nodes, acls)}
    open_w = wire(OPEN)
    for p in nodes:
        vec[p + '/kid'] = open_w
    vec[D] = vec['/bench'] = open_w
    for i in range(10):
        vec[leaf(i)] = open_w
    want = {'checked': 0, 'denied': 0, 'denied_lost': 0}
    fresh = 0
    for S, n in ((70, 1000), (3, 1000)):
        addrs = [(NET, OUT, NONE, A.addr_of('10.200.0.1'))[int(x)]
                 for x in rng.integers(0, 4, S)]
        pks, meta = [[] for _ in range(S)], [[] for _ in range(S)]
        for i in range(n):
            s = (i * S) // n
            base = nodes[int(rng.integers(40))]
            k = int(rng.integers(12))
            fresh += 1
            p, tgt = [
                (rd(base, bool(i % 2)), base),
                (rd(base, False, 'GET_CHILDREN'), base),
                (rd(base, bool(i % 2), 'GET_CHILDREN2'), base),
                (wr(base, 99), base),
                (wr(base), base),
                (mk('%s/f%d' % (base, fresh)), base),
                (mk(base + '/kid'), base),
                (rm(base + '/kid', 99), base),
                (rm(base + '/gone'), None),
                (rd(base, True, 'EXISTS'), None),
                ({'opcode': 'GET_ACL', 'path': base}, None),
                (wr(base + '/gone'), None)][k]
            pks[s].append(p)
            meta[s].append(tgt)
        conns = [(addrs[s], s % 64, pks[s]) for s in range(S)]
        b = Batch(srv, gpu, conns)
        i = 0
        for s in range(S):
            for p, tgt in zip(pks[s], meta[s]):
                code = A.OPS.get(p['opcode'])
                perm, _ = A.need(code)
                deny = False
                if tgt is not None:
                    want['checked'] += 1
                    deny = not A.permits(vec[tgt], perm, addrs[s])
                    want['denied'] += int(deny)
                assert (b.errs[i] == 'NO_AUTH') == deny, (i, p, addrs[s])
                if deny:
                    assert _is_no_auth(b, i)
                i += 1
        assert srv.acl_enforce_stats() == want
    assert 100 < want['denied'] < want['checked'] - 100


# ---- the launches -----------------------------------------------------------

class _Recorder(object):
    def __init__(self, ops, log):
        self._ops, self._log = ops, log

    def __getattr__(self, name):
        f = getattr(self._ops, name)

        def call(*a, **kw):
            self._log.append(name)
            return f(*a, **kw)
        return call


@pytest.mark.parametrize('kw', [{}, {'ordered': True, 'passes': 2},
                                {'resume': True, 'close': True}])
def test_perms_none_issues_the_launches_it_issued(gpu, monkeypatch, kw):
    """Every kernel is launched through an operator of torch.ops.zkmi, and no
    operator that existed was touched: the operators a call goes through are
    its launches.  Without ``perms`` no operator of the check is called; with
    it the sequence is the same one with the check behind the segment assign
    and the fix-up in front of the serve's reply encode."""
    srv = _world(gpu)
    conns = _denied_writes() + [
        (NET, 4, [rd(leaf(1)), rd(D, op='GET_CHILDREN'),
                  {'opcode': 'GET_ACL', 'path': D}])]
    Batch(srv, gpu, conns, **kw)                 # (every buffer allocated)
    Batch(srv, gpu, conns, enforce=False, **kw)
    log = []
    monkeypatch.setattr(_lib, '_ops', _Recorder(_lib.lib(), log))
    Batch(srv, gpu, conns, enforce=False, **kw)
    off = list(log)
    del log[:]
    Batch(srv, gpu, conns, **kw)
    on = list(log)
    assert not [x for x in off if x.startswith('aclperm')]
    assert [x for x in on if x.startswith('aclperm')] == ['aclperm_check',
                                                          'aclperm_fix']
    assert [x for x in on if not x.startswith('aclperm')] == off
    k = on.index('aclperm_check')
    assert on[k - 1] == 'sess_assign' and on[k + 1] == 'tree_mix_split'
    k = on.index('aclperm_fix')
    assert on[k + 1] == 'encode_responses'
    assert 'tree_acl_get_sessions' in on[k:]
