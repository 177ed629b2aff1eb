"""GpuServer.serve_sessions_mixed(perms=AclIdentity(addrs, auth=AuthTable)):
AUTH frames with the scheme ``digest`` give a connection identities, which
``digest`` ACL entries then match (csrc/kernels/tree_auth.hip; the rule:
csrc/kernels/zk_auth.h, mirrored by tests/auth_model.py; ``hashlib`` and
``base64`` are the reference for the identities).

Engine level: S = 8 segments, cap_frames 1024, the tree of
tests/test_gpu_aclperm.py with one node more, D/dg, whose ACL is
``digest:u:BvFa...`` with READ only.  time.time is frozen so twin trees' Stats
compare exactly."""

import struct
import time

import numpy as np
import pytest
import torch

import aclperm_model as A
import auth_model as M
import test_gpu_aclperm as T

from zkmi import jute
from zkmi.ops import _lib

pytestmark = pytest.mark.gpu

I64, I32, U8 = torch.int64, torch.int32, torch.uint8
S = 8
D, NET, OUT, NONE = T.D, T.NET, T.OUT, T.NONE
mk, rd, wr, rm, leaf = T.mk, T.rd, T.wr, T.rm, T.leaf
EDGES = (0, 1, 54, 55, 56, 57, 63, 64, 65, 118, 119)
U_ID = M.identity(b'u:pw')
SUPER_ID = M.identity(b'super:test')
DG = D + '/dg'
REPLY = struct.Struct('>iiqi')


@pytest.fixture(autouse=True)
def _frozen_time(monkeypatch):
    monkeypatch.setattr(time, 'time', lambda: T.NOW)


def digest_acl(perms, ident):
    return [{'perms': perms, 'id': {'scheme': 'digest',
                                    'id': ident.decode()}}]


def au(cred, scheme='digest', xid=None):
    """An AUTH packet; ``xid``: kept as given (else the frame's index)."""
    p = {'opcode': 'AUTH', 'type': 0, 'scheme': scheme, 'auth': cred}
    if xid is not None:
        p['xid'], p['keep_xid'] = xid, True
    return p


def _cred(n):
    rng = np.random.RandomState(n)
    raw = bytes(rng.randint(1, 256, size=n).astype(np.uint8).tolist())
    raw = raw.replace(b':', b';')
    return (b'usr:' + raw[4:]) if n >= 5 else raw


class Batch(object):
    """One serve_sessions_mixed batch of S segments.  ``conns``: [(addr,
    watcher slot, [packet, ...])], a connection a segment (missing ones are
    empty); xids are the frames' indices unless a packet keeps its own.
    ``auth``: the AuthTable (None: ``perms`` alone)."""

    def __init__(self, srv, gpu, conns, auth=None, sessions=None, starts=None,
                 **kw):
        from zkmi.server.engine import AclIdentity, SessionSegments
        conns = list(conns) + [(NONE, -1, [])] * (S - len(conns))
        assert len(conns) == S
        self.flat = [p for _, _, pk in conns for p in pk]
        for x, p in enumerate(self.flat):
            if not p.get('keep_xid'):
                p['xid'] = x
            if 'raw' in p and len(p['raw']) >= 4:
                p['raw'] = struct.pack('>i', p['xid']) + p['raw'][4:]
        self.parts = [b''.join(jute.frame(T._body(p)) for p in pk)
                      for _, _, pk in conns]
        rx = b''.join(self.parts)
        cuts = [0] + [int(x) for x in np.cumsum([len(b) for b in self.parts])]
        self.segs = segs = SessionSegments(
            torch.tensor(cuts if starts is None else starts, dtype=I64,
                         device=gpu),
            torch.tensor(sessions or [0x100 + s for s in range(S)],
                         dtype=I64, device=gpu),
            torch.tensor([w for _, w, _ in conns], dtype=I32, device=gpu))
        perms = AclIdentity(torch.tensor(
            [A.as_i32(a) for a, _, _ in conns], dtype=I32, device=gpu),
            auth=auth)
        self.zxid = int(srv.tree.counters[_lib.TC_ZXID].item())
        self.rx = T._dev(rx, gpu)
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
        # frame order kept
        assert [r['xid'] for r in self.reps] == [p['xid'] for p in self.flat]
        self.errs = [r['err'] for r in self.reps]
        self.rep_off = srv.seg.rep_off.cpu().tolist()
        self.deny = srv.acl_deny.cpu().tolist()[:len(self.flat)]


def _world(gpu):
    """test_gpu_aclperm's tree and D/dg (READ for the identity of u:pw) with
    a child."""
    srv = T._world(gpu)
    b = T.Batch(srv, gpu, [(0, -1, [mk(DG, digest_acl(A.READ, U_ID))])],
                enforce=False)
    assert b.errs == ['OK']
    b = T.Batch(srv, gpu, [(0, -1, [mk(DG + '/kid')])], enforce=False)
    assert b.errs == ['OK'] and srv.acl_stats()[2] == 0
    return srv


def _table(gpu):
    from zkmi.server.engine import AuthTable
    return AuthTable(S, gpu)


def _header(b, i, err):
    """Frame i's reply is exactly be32(16), its xid, zxid, be32(err)."""
    return b.frames[i] == REPLY.pack(16, b.flat[i]['xid'], b.zxid, err)


# ---- the identities ---------------------------------------------------------

def test_identity_edges(gpu):
    srv, tbl = _world(gpu), _table(gpu)
    creds = [_cred(n) for n in EDGES]
    b = Batch(srv, gpu, [(NONE, -1, [au(c)]) for c in creds[:S]], auth=tbl)
    assert b.errs == ['OK'] * S
    assert tbl.identities() == [[M.identity(c)] for c in creds[:S]]
    assert tbl.cnt.cpu().tolist() == [1] * S
    tbl.clear(torch.arange(S, dtype=I64, device=gpu))
    assert tbl.identities() == [[]] * S
    rest = creds[S:] + [b'x' * 120]
    b = Batch(srv, gpu, [(NONE, -1, [au(c)]) for c in rest], auth=tbl)
    assert b.errs == ['OK'] * (len(rest) - 1) + ['AUTH_FAILED']
    assert _header(b, len(rest) - 1, M.AUTH_FAILED)
    want = [[M.identity(c)] for c in creds[S:]]
    assert tbl.identities() == want + [[]] * (S - len(want))
    assert tbl.cnt.cpu().tolist() == [1] * len(want) + [0] * (S - len(want))
    st = srv.auth_stats()
    assert (st['ok'], st['failed'], st['full'], st['known']) == (11, 1, 0, 0)
    assert (st['answered_ok'], st['answered_failed']) == (11, 1)
    # the recorded vectors
    tbl.clear(torch.tensor([0, 1, 2], dtype=I64, device=gpu))
    Batch(srv, gpu, [(NONE, -1, [au(b'super:test')]),
                     (NONE, -1, [au(b'u:pw')]),
                     (NONE, -1, [au(b'y' * 119)])], auth=tbl)
    got = tbl.identities()
    assert got[:2] == [[b'super:D/InIHSb7yEEbrWz8b9l71RjZJU='],
                       [b'u:BvFaefuhWURhnvpD7ipe45CKTpk=']]
    # no ':' in 119 bytes: the longest identity there is
    assert got[2] == [M.identity(b'y' * 119)] and len(got[2][0]) == 148


def test_exact_replies(gpu):
    srv, tbl = _world(gpu), _table(gpu)
    trailing = {'opcode': 'AUTH', 'raw': M.body(0, b'digest', b'u:pw') + b'\0'}
    short = {'opcode': 'AUTH', 'raw': M.body(0, b'digest', b'u:pw')[:-1]}
    b = Batch(srv, gpu, [
        (NONE, -1, [au(b'u:pw', xid=-4), rd(leaf(1)), au(b'u:pw', 'ip'),
                    trailing]),
        (NONE, -1, [au(b'a:b', xid=0x7ffffff0), short,
                    au(b'x' * 500, xid=-4)])], auth=tbl)
    assert b.errs == ['OK', 'OK', 'AUTH_FAILED', 'AUTH_FAILED', 'OK',
                      'AUTH_FAILED', 'AUTH_FAILED']
    for i, e in ((0, 0), (2, -115), (3, -115), (4, 0), (5, -115), (6, -115)):
        assert _header(b, i, e), (i, b.frames[i])
        assert len(b.frames[i]) == 20
    assert b.flat[0]['xid'] == -4 and b.flat[4]['xid'] == 0x7ffffff0
    assert tbl.identities()[:2] == [[U_ID], [M.identity(b'a:b')]]
    # rx is as it came: an AUTH frame is answered without a mark in it
    assert b.rx.cpu().numpy().tobytes()[:len(b''.join(b.parts))] == \
        b''.join(b.parts)


# ---- enforcement ------------------------------------------------------------

def test_enforcement(gpu):
    srv, tbl = _world(gpu), _table(gpu)
    dig = srv.tree.digest()
    b = Batch(srv, gpu, [
        (NONE, -1, [au(b'u:pw'), rd(DG), wr(DG)]),
        (NONE, -1, [rd(DG)]),                       # anonymous, same batch
        (NET, -1, [rd(D + '/ipnet'), wr(D + '/ro')]),
        (OUT, -1, [rd(D + '/ipnet'), rd(D + '/ro')]),
        # the identity holds for the frames ahead of the AUTH frame too
        (NONE, -1, [rd(DG), au(b'u:pw')]),
        # a wrong password: AUTH itself is answered OK, the node stays shut
        (NONE, -1, [au(b'u:bad'), rd(DG), rd(DG, op='GET_CHILDREN')]),
        (NONE, -1, [au(b'super:test'), rd(DG)])], auth=tbl)
    assert b.errs == ['OK', 'OK', 'NO_AUTH',
                      'NO_AUTH',
                      'OK', 'NO_AUTH',
                      'NO_AUTH', 'OK',
                      'OK', 'OK',
                      'OK', 'NO_AUTH', 'NO_AUTH',
                      'OK', 'NO_AUTH']
    assert _header(b, 2, A.NO_AUTH) and _header(b, 3, A.NO_AUTH)
    assert srv.tree.digest() == dig
    # the next batch: the identity is the connection's still
    b = Batch(srv, gpu, [(NONE, -1, [rd(DG), rd(DG, op='GET_CHILDREN2'),
                                     mk(DG + '/x')]),
                         (NONE, -1, [rd(DG)])], auth=tbl)
    assert b.errs == ['OK', 'OK', 'NO_AUTH', 'NO_AUTH']
    # without the table the node opens to nobody, as before
    b = Batch(srv, gpu, [(NONE, -1, [au(b'u:pw'), rd(DG)])])
    assert b.errs == ['BAD_ARGUMENTS', 'NO_AUTH']


# ---- random frames ----------------------------------------------------------

POOL = [b'u:pw', b'super:test', b'x:y', b'nocolon']


def _random_acl(rng):
    schemes = ['world', 'ip', 'digest', 'digest', 'auth', 'sasl']
    ids = {'world': ['anyone', 'anyone', 'nobody'],
           'ip': ['10.1.2.0/24', '10.1.2.9', '10.1.3.9/32', '10.0.0.0/8',
                  '10.1.2.300/24'],
           'digest': [U_ID.decode(), SUPER_ID.decode(),
                      M.identity(b'x:y').decode(), 'u:pw', U_ID.decode()[:-1]],
           'auth': [''], 'sasl': [U_ID.decode()]}
    out = []
    for _ in range(int(rng.integers(1, 4))):
        s = schemes[int(rng.integers(len(schemes)))]
        out.append({'perms': int(rng.integers(0, 32)),
                    'id': {'scheme': s,
                           'id': ids[s][int(rng.integers(len(ids[s])))]}})
    return out


class Frames(object):
    """The random batches of the differential and the model check: 2 x 1 000
    frames over S connections against 40 nodes with random vectors, made
    once; with ``auths`` each connection's batch also carries AUTH frames at
    random places."""

    def __init__(self):
        rng = np.random.default_rng(17)
        self.nodes = ['%s/v%02d' % (D, k) for k in range(40)]
        self.acls = [_random_acl(rng) for _ in self.nodes]
        self.vec = {p: T.wire(a) for p, a in zip(self.nodes, self.acls)}
        self.addrs = [(NET, OUT, NONE, A.addr_of('10.200.0.1'))[int(x)]
                      for x in rng.integers(0, 4, S)]
        self.batches = []
        fresh = 0
        for gen in range(2):
            pks, meta = [[] for _ in range(S)], [[] for _ in range(S)]
            # the unordered serve's batch is concurrent: a node takes at
            # most one frame a batch that changes it, and then no frame
            # that reads it, so twin trees answer byte for byte the same
            written = set(int(x) for x in rng.choice(40, 12, replace=False))
            used = set()
            for i in range(1000):
                s = (i * S) // 1000
                v = int(rng.integers(40))
                base = self.nodes[v]
                fresh += 1
                quiet = [
                    (wr(base, 99), base),
                    (mk(base + '/kid'), base),
                    (rm(base + '/kid', 99), base),
                    (rm(base + '/gone'), None),
                    (wr(base + '/gone'), None)]
                if v in written and v not in used:
                    used.add(v)
                    p, tgt = [(wr(base), base),
                              (mk('%s/f%d' % (base, fresh)), base)][i % 2]
                elif v in written:
                    p, tgt = quiet[int(rng.integers(len(quiet)))]
                else:
                    reads = [
                        (rd(base, bool(i % 2)), base),
                        (rd(base, False, 'GET_CHILDREN'), base),
                        (rd(base, bool(i % 2), 'GET_CHILDREN2'), base),
                        (rd(base, True, 'EXISTS'), None),
                        ({'opcode': 'GET_ACL', 'path': base}, None)]
                    p, tgt = (reads + quiet)[int(rng.integers(10))]
                pks[s].append(p)
                meta[s].append(tgt)
            # the AUTH frames of connection s: distinct identities of POOL
            # (at most 4 a connection over both batches: no row fills up),
            # and frames that fail; (place, packet)
            auths = []
            for s in range(S):
                k = int(rng.integers(0, 4))
                pick = [POOL[int(j)] for j in
                        rng.choice(len(POOL), size=k, replace=False)]
                row = [au(c) for c in pick]
                if rng.integers(2):
                    row.append(au(b'u:pw', 'ip'))
                if rng.integers(3) == 0:
                    row.append(au(b'u:' + b'p' * 118))
                auths.append([(int(rng.integers(0, len(pks[s]) + 1)), p)
                              for p in row])
            self.batches.append((pks, meta, auths))

    def conns(self, gen, with_auth):
        pks, meta, auths = self.batches[gen]
        out, tags = [], []
        for s in range(S):
            row = [(dict(p), t) for p, t in zip(pks[s], meta[s])]
            if with_auth:
                for at, p in sorted(auths[s], key=lambda x: -x[0]):
                    row.insert(at, (dict(p), 'auth'))
            out.append((self.addrs[s], s, [p for p, _ in row]))
            tags.append([t for _, t in row])
        return out, tags


@pytest.fixture(scope='module')
def frames():
    return Frames()


def _random_world(gpu, fr):
    srv = T._server(gpu)
    b = T.Batch(srv, gpu, [(0, -1, [mk(p, a) for p, a in
                                    zip(fr.nodes, fr.acls)])], enforce=False)
    assert b.errs == ['OK'] * 40
    b = T.Batch(srv, gpu, [(0, -1, [mk(p + '/kid') for p in fr.nodes])],
                enforce=False)
    assert b.errs == ['OK'] * 40 and srv.acl_stats()[2] == 0
    return srv


def test_no_auth_frame_equals_perms_alone(gpu, frames):
    """2 000 random frames, none of them AUTH: with an AuthTable the reply
    stream, the ranges and the deny table are byte for byte those of ``perms``
    alone on a twin tree."""
    sx, sy = _random_world(gpu, frames), _random_world(gpu, frames)
    tbl = _table(gpu)
    denied = 0
    for gen in range(2):
        x = Batch(sx, gpu, frames.conns(gen, False)[0], auth=tbl)
        y = Batch(sy, gpu, frames.conns(gen, False)[0])
        assert len(x.flat) == 1000
        for i, (fx, fy, p) in enumerate(zip(x.frames, y.frames, x.flat)):
            if p['opcode'] in ('GET_CHILDREN', 'GET_CHILDREN2') and \
                    x.errs[i] == 'OK':             # (the names' order is free)
                assert len(fx) == len(fy) and sorted(
                    x.reps[i]['children']) == sorted(y.reps[i]['children'])
            else:
                assert fx == fy, (gen, i)
        assert len(x.raw) == len(y.raw)
        assert x.rep_off == y.rep_off
        assert x.deny == y.deny
        denied += sum(x.deny)
        assert sx.tree.digest() == sy.tree.digest()
    assert sx.acl_enforce_stats() == sy.acl_enforce_stats()
    assert 100 < denied
    assert tbl.identities() == [[]] * S
    assert set(sx.auth_stats().values()) == {0}


def test_model_random_frames_with_auth(gpu, frames):
    """The same frames with AUTH frames mixed in: per frame the answer is the
    mirror's — an identity holds for the whole batch that carries its AUTH
    frame and for the batches after it."""
    srv, tbl = _random_world(gpu, frames), _table(gpu)
    model = M.Table(S)
    open_w = T.wire(T.OPEN)
    want = {'checked': 0, 'denied': 0, 'denied_lost': 0}
    n_ok = n_failed = opened = 0
    for gen in range(2):
        conns, tags = frames.conns(gen, True)
        b = Batch(srv, gpu, conns, auth=tbl)
        codes = iter(model.batch(
            [(s, jute.encode_request(dict(p, xid=0)))
             for s, (_, _, pk) in enumerate(conns)
             for p, t in zip(pk, tags[s]) if t == 'auth']))
        i = 0
        for s, (addr, _, pk) in enumerate(conns):
            for p, tgt in zip(pk, tags[s]):
                if tgt == 'auth':
                    code = next(codes)
                    n_ok += code == 1
                    n_failed += code == 2
                    assert b.errs[i] == ('OK' if code == 1 else
                                         'AUTH_FAILED'), (gen, i, p)
                    assert _header(b, i, 0 if code == 1 else M.AUTH_FAILED)
                    assert b.deny[i] == 0
                else:
                    perm, _ = A.need(A.OPS.get(p['opcode']))
                    deny = False
                    if tgt is not None:
                        want['checked'] += 1
                        vec = frames.vec.get(tgt, open_w)
                        deny = not M.permits_auth(vec, perm, addr,
                                                  model.rows[s])
                        opened += deny != (not A.permits(vec, perm, addr))
                        want['denied'] += int(deny)
                    assert (b.errs[i] == 'NO_AUTH') == deny, (gen, i, p, addr)
                    assert b.deny[i] == int(deny)
                i += 1
        assert [sorted(r) for r in tbl.identities()] == \
            [sorted(r) for r in model.rows]
        assert srv.acl_enforce_stats() == want
    st = srv.auth_stats()
    assert (st['ok'], st['failed'], st['full']) == (n_ok, n_failed, 0)
    assert (st['answered_ok'], st['answered_failed']) == (n_ok, n_failed)
    assert n_ok > 10 and n_failed > 3 and st['known'] > 0
    # digest entries did open nodes that perms alone keeps shut
    assert opened > 20 and 100 < want['denied'] < want['checked'] - 100


# ---- the table's life -------------------------------------------------------

def test_table_life(gpu):
    srv, tbl = _world(gpu), _table(gpu)
    b = Batch(srv, gpu, [(NONE, -1, [rd(DG)]),
                         (NONE, -1, [au(b'u:pw')])], auth=tbl)
    assert b.errs == ['NO_AUTH', 'OK']
    # the next batch: the identity persists, the same AUTH takes no slot
    b = Batch(srv, gpu, [(NONE, -1, []),
                         (NONE, -1, [rd(DG), au(b'u:pw')])], auth=tbl)
    assert b.errs == ['OK', 'OK']
    assert tbl.cnt.cpu().tolist()[1] == 1 and srv.auth_stats()['known'] == 1
    b = Batch(srv, gpu, [(NONE, -1, []),
                         (NONE, -1, [au(b'a:1'), au(b'b:2'), au(b'c:3')])],
              auth=tbl)
    assert b.errs == ['OK'] * 3
    assert sorted(tbl.identities()[1]) == sorted(
        M.identity(c) for c in (b'u:pw', b'a:1', b'b:2', b'c:3'))
    # a fifth distinct identity: AUTH_FAILED, counted full; a known one: OK
    b = Batch(srv, gpu, [(NONE, -1, []),
                         (NONE, -1, [au(b'e:5'), au(b'b:2'), rd(DG)])],
              auth=tbl)
    assert b.errs == ['AUTH_FAILED', 'OK', 'OK']
    st = srv.auth_stats()
    assert st['full'] == 1 and st['failed'] == 1 and st['known'] == 2
    assert tbl.cnt.cpu().tolist()[1] == 4
    assert len(tbl.identities()[1]) == 4
    # another row is another connection
    b = Batch(srv, gpu, [(NONE, -1, [au(b'e:5'), rd(DG)])], auth=tbl)
    assert b.errs == ['OK', 'NO_AUTH']
    # clear: the row is forgotten, the others stay
    tbl.clear(torch.tensor([1], dtype=I64, device=gpu))
    assert tbl.identities()[:2] == [[M.identity(b'e:5')], []]
    b = Batch(srv, gpu, [(NONE, -1, []), (NONE, -1, [rd(DG)])], auth=tbl)
    assert b.errs == ['NO_AUTH']
    b = Batch(srv, gpu, [(NONE, -1, []), (NONE, -1, [au(b'u:pw'), rd(DG)])],
              auth=tbl)
    assert b.errs == ['OK', 'OK'] and tbl.identities()[1] == [U_ID]


def test_refused_segments_store_nothing(gpu):
    from zkmi.server.sessions import GpuSessionTable
    srv, tbl = _world(gpu), _table(gpu)
    tab = GpuSessionTable(srv.tree, cap=64)
    sid = [tab.sid_of(k) for k in range(S)]
    for k in range(S):
        tab.sid[k] = sid[k]
        tab.state[k] = 1
    tab.next.fill_(S)
    tab.close(torch.tensor([sid[1]], dtype=I64, device=gpu))
    conns = [(NONE, -1, [au(b'u:pw'), rd(DG)]),
             (NONE, -1, [au(b'u:pw'), rd(DG)]),
             (NONE, -1, [rd(DG)])]
    b = Batch(srv, gpu, conns, auth=tbl, sessions=sid, table=tab)
    assert b.errs == ['OK', 'OK', 'SESSION_EXPIRED', 'SESSION_EXPIRED',
                      'NO_AUTH']
    assert tbl.identities()[:3] == [[U_ID], [], []]
    assert tbl.cnt.cpu().tolist() == [1] + [0] * (S - 1)
    # an unsound table (a torn frame): SYSTEMERROR for all, nothing stored
    tbl.clear(torch.tensor([0], dtype=I64, device=gpu))
    lens = [sum(len(jute.frame(T._body(dict(p, xid=0)))) for p in pk)
            for _, _, pk in conns]
    starts = [0, lens[0] + 2, lens[0] + lens[1]] + [sum(lens)] * (S - 2)
    b = Batch(srv, gpu, conns, auth=tbl, starts=starts)
    assert b.errs == ['SYSTEM_ERROR'] * 5
    assert srv.session_stats()['bad'] > 0
    assert tbl.identities() == [[]] * S
    assert tbl.cnt.cpu().tolist() == [0] * S
    st = srv.auth_stats()
    assert (st['ok'], st['failed']) == (1, 0)


def test_deferred_auth_frame(gpu):
    """Two passes, three sets of one node: connection 2's set is deferred
    with the AUTH frame behind it.  Sent again in the next batch the frame
    finds its identity stored and is answered OK: one slot."""
    from zkmi.server.engine import OrderDefer
    X = D + '/ipnet'
    srv, tbl = _world(gpu), _table(gpu)
    df = OrderDefer(S, gpu)
    tail = [wr(X), au(b'u:pw', xid=-4), rd(DG)]
    b = Batch(srv, gpu, [(NET, 1, [wr(X), wr(X)]), (NONE, -1, []),
                         (NET, 3, [dict(p) for p in tail])],
              auth=tbl, ordered=True, passes=2, defer=df)
    assert int(df.deferred.item()) == 3
    assert df.used.cpu().tolist()[:3] == [len(b.parts[0]), 0, 0]
    assert b.errs == ['OK', 'OK', 'SYSTEM_ERROR', 'SYSTEM_ERROR',
                      'SYSTEM_ERROR']
    assert df.rep_end.cpu().tolist()[2] == b.rep_off[2]
    # (the AUTH pass runs before the deferral: the identity is stored already)
    assert tbl.identities()[2] == [U_ID]
    assert srv.auth_stats()['answered_ok'] == 0
    b = Batch(srv, gpu, [(NET, 1, []), (NONE, -1, []),
                         (NET, 3, [dict(p) for p in tail])],
              auth=tbl, ordered=True, passes=2, defer=df)
    assert int(df.deferred.item()) == 0
    assert b.errs == ['OK', 'OK', 'OK']
    assert _header(b, 1, 0) and b.flat[1]['xid'] == -4
    assert tbl.identities()[2] == [U_ID] and tbl.cnt.cpu().tolist()[2] == 1
    st = srv.auth_stats()
    assert st['answered_ok'] == 1 and st['known'] >= 1


def test_arguments(gpu):
    from zkmi.server.engine import AclIdentity, AuthTable
    addrs = torch.zeros(S, dtype=I32, device=gpu)
    with pytest.raises(ValueError):
        AclIdentity(addrs, auth=AuthTable(S - 1, gpu))
    with pytest.raises(ValueError):
        AclIdentity(addrs, auth=object())
    with pytest.raises(ValueError):
        AuthTable(0, gpu)
    assert AclIdentity(addrs, auth=AuthTable(S + 3, gpu)).auth.S == S + 3
    assert _lib.auth_row_bytes() == _lib.AUTH_K * _lib.AUTH_REC
    srv, tbl = _world(gpu), _table(gpu)
    b = Batch(srv, gpu, [(NONE, -1, [au(b'u:pw')])], auth=tbl)
    L = _lib.lib()
    ft = srv.result[3]
    # the op's own checks: a short record table, a wrong dtype
    with pytest.raises(RuntimeError):
        L.auth_frames(b.rx, ft.off, ft.length, ft.count, srv.cap_frames,
                      srv.seg.table(b.segs),
                      [tbl.recs[:S - 1], tbl.cnt, tbl.stats], srv.auth_res)
    with pytest.raises(RuntimeError):
        L.auth_fix(srv.auth_res.to(I64), srv.mix_cls, srv.mix_sub, ft.count,
                   srv.cap_frames, srv.resp.err, tbl.stats)


# ---- the launches -----------------------------------------------------------

@pytest.mark.parametrize('kw', [{}, {'ordered': True, 'passes': 2},
                                {'resume': True, 'close': True}])
def test_launches(gpu, monkeypatch, kw):
    """Every kernel is launched through an operator of torch.ops.zkmi.
    Without ``auth`` the call goes through the operators it went through
    before there was an AuthTable — the check, the fix-up and no operator of
    this file; with it the AUTH pass stands behind the segment assign, the
    check is the one that reads the table and the AUTH fix-up follows the
    check's, in front of the serve's reply encode."""
    srv, tbl = _world(gpu), _table(gpu)
    conns = T._denied_writes() + [
        (NET, 4, [rd(leaf(1)), rd(D, op='GET_CHILDREN'),
                  {'opcode': 'GET_ACL', 'path': D}, rd(DG)])]

    def fresh():
        return [(a, w, [dict(p) for p in pk]) for a, w, pk in conns]
    Batch(srv, gpu, fresh(), auth=tbl, **kw)      # (every buffer allocated)
    Batch(srv, gpu, fresh(), **kw)
    log = []
    monkeypatch.setattr(_lib, '_ops', T._Recorder(_lib.lib(), log))
    Batch(srv, gpu, fresh(), **kw)
    off = list(log)
    del log[:]
    Batch(srv, gpu, fresh(), auth=tbl, **kw)
    on = list(log)
    new = ('auth_frames', 'aclperm_check_auth', 'auth_fix')
    assert not [x for x in off if x in new or x == 'auth_row_bytes']
    assert [x for x in off if x.startswith('aclperm')] == ['aclperm_check',
                                                           'aclperm_fix']
    k = off.index('aclperm_check')
    assert off[k - 1] == 'sess_assign' and off[k + 1] == 'tree_mix_split'
    assert off[off.index('aclperm_fix') + 1] == 'encode_responses'
    # with the table: three operators in, one out, the rest as it was
    assert [x for x in on if x in new] == list(new)
    assert 'aclperm_check' not in on
    assert [x for x in on if x not in new] == \
        [x for x in off if x != 'aclperm_check']
    k = on.index('auth_frames')
    assert on[k - 1] == 'sess_assign' and on[k + 1] == 'aclperm_check_auth' \
        and on[k + 2] == 'tree_mix_split'
    k = on.index('auth_fix')
    assert on[k - 1] == 'aclperm_fix' and on[k + 1] == 'encode_responses'
