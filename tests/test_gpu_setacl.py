"""GpuServer.serve_sessions_mixed(setacl=True): SET_ACL frames are served by
a pass of the ACL engine's class (csrc/kernels/tree_setacl.hip; the rule:
csrc/kernels/zk_setacl.h, mirrored by tests/setacl_model.py).

A tree of 2 000 static nodes with ``acl_cap=64``; under /bench/d000000 a few
nodes with ACLs of their own.  The sequential model is fakezk's ZKDatabase
(``set_acl``) under the batch contract: ADMIN judged on the ACL the batch
finds, one SET_ACL a node a round, P rounds.  time.time is frozen so twin
trees' Stats compare exactly."""

import struct
import time

import numpy as np
import pytest
import torch

import aclperm_model as A
import auth_model as M
import setacl_model as S
import test_gpu_aclperm as T

from zkmi import jute
from zkmi.ops import _lib

pytestmark = pytest.mark.gpu

I64, I32 = torch.int64, torch.int32
D = T.D
NET, OUT, NONE = T.NET, T.OUT, T.NONE
HEAD = struct.Struct('>iiqi')
P = 4
U_ID = M.identity(b'u:pw')


class _Jute(object):
    """zkmi.jute for the Batch helpers of the neighbouring test modules,
    with the SET_ACL reply decoded (the oracle's default leaves it the
    unsupported opcode it is for the GPU reply decoders)."""

    def __getattr__(self, name):
        return getattr(jute, name)

    @staticmethod
    def decode_response(body, xid_map):
        return jute.decode_response(body, xid_map, set_acl=True)


@pytest.fixture(autouse=True)
def _frozen_time(monkeypatch):
    import test_gpu_auth as G
    monkeypatch.setattr(time, 'time', lambda: T.NOW)
    monkeypatch.setattr(T, 'jute', _Jute())
    monkeypatch.setattr(G, 'jute', _Jute())


def leaf(i):
    return '/bench/d%06d/n%09d' % (i // 100, i)


def ent(perms, scheme='world', who='anyone'):
    return {'perms': perms, 'id': {'scheme': scheme, 'id': who}}


OPEN = [ent(A.ALL)]
RO = [ent(A.READ)]
NOADMIN = [ent(A.ALL & ~A.ADMIN)]
NETADMIN = [ent(A.READ), ent(A.ALL, 'ip', '10.1.2.0/24')]
MINE = [ent(A.ALL, 'digest', U_ID.decode())]
THREE = [ent(A.READ), ent(A.ALL, 'digest', U_ID.decode()),
         ent(A.ADMIN, 'ip', '10.1.2.0/24')]
BIG = [ent(A.ALL, 'digest', 'x' * 278)]


def sa(path, acl, version=-1):
    return {'opcode': 'SET_ACL', 'path': path, 'acl': acl, 'version': version}


def ga(path):
    return {'opcode': 'GET_ACL', 'path': path}


def canon(acl):
    """``acl`` as a reply decodes: perm names."""
    return [{'perms': [k for k, m in
                       (('READ', 1), ('WRITE', 2), ('CREATE', 4),
                        ('DELETE', 8), ('ADMIN', 16))
                       if jute.perms_to_mask(a['perms']) & m],
             'id': dict(a['id'])} for a in acl]


def _server(gpu, frames=1024):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(n_nodes=2000, fanout=100, watch_cap=4096, acl_cap=64,
                   scratch=1 << 20, device=gpu, ctime_ms=int(T.NOW * 1000))
    return GpuServer(tree, frames, 1 << 20, window=512)


def batch(srv, gpu, conns, enforce=False, **kw):
    kw.setdefault('setacl', True)
    return T.Batch(srv, gpu, conns, enforce=enforce, **kw)


def one(srv, gpu, pkts, addr=NONE, **kw):
    return batch(srv, gpu, [(addr, -1, list(pkts))], **kw)


def _world(gpu, frames=1024):
    """D/ro, D/noadmin, D/net (ADMIN for 10.1.2.0/24), D/mine (a digest
    identity), made without SET_ACL."""
    srv = _server(gpu, frames)
    b = one(srv, gpu, [T.mk(D + '/ro', RO), T.mk(D + '/noadmin', NOADMIN),
                       T.mk(D + '/net', NETADMIN), T.mk(D + '/mine', MINE)],
            setacl=False)
    assert b.errs == ['OK'] * 4 and srv.acl_stats()[2] == 0
    return srv


def stat_of(srv, gpu, path):
    b = one(srv, gpu, [T.rd(path, op='EXISTS')], setacl=False)
    assert b.errs == ['OK']
    return b.reps[0]['stat']


def acl_of(srv, gpu, path):
    b = one(srv, gpu, [ga(path)], setacl=False)
    assert b.errs == ['OK']
    return b.reps[0]['acl'], b.reps[0]['stat']


# ---- without opcode 7 -------------------------------------------------------

@pytest.mark.parametrize('n,S_', [(1, 1), (65, 3), (257, 5)])
def test_without_set_acl_the_bytes_are_the_same(gpu, n, S_):
    sx, sy = _world(gpu), _world(gpu)

    def conns():
        pks = [[] for _ in range(S_)]
        for i in range(n):
            pks[i % S_].append([ga(leaf(i)), T.rd(leaf(i)), ga(D + '/mine'),
                                T.wr(leaf(500 + i)), ga('/nope'),
                                T.rd(leaf(i), op='EXISTS'),
                                T.mk('%s/k%d' % (D, i), RO)][i % 7])
        return [(NONE, -1, pk) for pk in pks]
    for _ in range(2):
        x = batch(sx, gpu, conns())
        y = batch(sy, gpu, conns(), setacl=False)
        assert x.raw == y.raw
        assert x.rep_off == y.rep_off
    assert sx.tree.digest() == sy.tree.digest()
    assert sx.acl_stats() == sy.acl_stats()
    assert sx.setacl_stats() == dict.fromkeys(_lib.SETACL_STATS, 0)
    assert int(sx.tree.counters[_lib.TC_ZXID].item()) == \
        int(sy.tree.counters[_lib.TC_ZXID].item())


def test_empty_class_and_arguments(gpu):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    srv = _world(gpu)
    b = one(srv, gpu, [T.rd(leaf(1)), {'opcode': 'PING'}])
    assert b.errs == ['OK', 'OK']
    b = batch(srv, gpu, [(NONE, -1, [])])
    assert b.raw == b''
    bare = GpuServer(GpuTree(n_nodes=2000, fanout=100, device=gpu), 64,
                     1 << 16, window=512)
    with pytest.raises(ValueError):
        one(bare, gpu, [T.rd(leaf(1))])
    # off, opcode 7 is the unknown request it was
    b = one(srv, gpu, [sa(leaf(1), RO)], setacl=False)
    assert b.errs == ['BAD_ARGUMENTS']
    assert acl_of(srv, gpu, leaf(1))[0] == canon(OPEN)


# ---- the replies ------------------------------------------------------------

def test_exact_frames_and_precedence(gpu):
    srv = _world(gpu)
    st0 = stat_of(srv, gpu, leaf(3))
    empty = []
    whole = jute.encode_request(dict(sa(leaf(5), RO), xid=0))
    pk = [sa(leaf(3), RO, -1),                      # 0 OK
          sa('/nope', empty, 7),                    # 1 INVALID_ACL first
          sa(D + '/noadmin', empty, 7),             # 2 ... before NO_AUTH
          sa('/nope', RO, 7),                       # 3 NO_NODE before
          sa(D + '/noadmin', RO, 7),                # 4 NO_AUTH before
          sa(leaf(4), RO, 7),                       # 5 BAD_VERSION
          {'opcode': 'SET_ACL', 'raw': whole[:-1]},        # 6 truncated
          {'opcode': 'SET_ACL', 'raw': whole + b'\0'},     # 7 trailing
          sa('/', RO, -1),                          # 8 "/" has no node here
          sa(leaf(6), RO, 0)]                       # 9 OK, an explicit version
    b = one(srv, gpu, pk, enforce=True)
    assert b.errs == ['OK', 'INVALID_ACL', 'INVALID_ACL', 'NO_NODE',
                      'NO_AUTH', 'BAD_VERSION', 'BAD_ARGUMENTS',
                      'BAD_ARGUMENTS', 'NO_NODE', 'OK']
    # zxids: the frames that reached the version check, in frame order
    zx = {0: b.zxid + 1, 5: b.zxid + 2, 9: b.zxid + 3}
    want = jute.Stat(*st0.as_tuple())
    want.aversion = 1
    assert len(b.frames[0]) == 88
    assert b.frames[0] == HEAD.pack(84, 0, zx[0], 0) + want.to_bytes()
    for i, e in ((1, S.INVALID_ACL), (2, S.INVALID_ACL), (3, S.NO_NODE),
                 (4, S.NO_AUTH), (5, S.BAD_VERSION), (6, S.BAD_ARGUMENTS),
                 (7, S.BAD_ARGUMENTS), (8, S.NO_NODE)):
        assert b.frames[i] == HEAD.pack(16, i, zx.get(i, b.zxid), e), i
    assert b.reps[9]['zxid'] == zx[9] and b.reps[9]['stat'].aversion == 1
    assert int(srv.tree.counters[_lib.TC_ZXID].item()) == b.zxid + 3
    assert srv.setacl_stats() == {
        'applied': 2, 'bad_version': 1, 'denied': 1, 'invalid': 2,
        'unreached': 0, 'store_full': 0}
    assert acl_of(srv, gpu, leaf(3)) == (canon(RO), want)
    assert acl_of(srv, gpu, leaf(4))[0] == canon(OPEN)
    assert acl_of(srv, gpu, D + '/noadmin')[0] == canon(NOADMIN)
    # without perms nothing is checked
    b = one(srv, gpu, [sa(D + '/noadmin', RO, 0)])
    assert b.errs == ['OK'] and acl_of(srv, gpu, D + '/noadmin')[0] == \
        canon(RO)


def test_admin_by_address_and_identity(gpu):
    import test_gpu_auth as G
    srv = _world(gpu)
    b = batch(srv, gpu, [(OUT, -1, [sa(D + '/net', RO)]),
                         (NONE, -1, [sa(D + '/net', RO)]),
                         (NET, -1, [sa(D + '/mine', RO)]),
                         (NET, -1, [sa(D + '/net', NETADMIN + RO)])],
              enforce=True)
    assert b.errs == ['NO_AUTH', 'NO_AUTH', 'NO_AUTH', 'OK']
    # a digest identity: the AUTH frame of the batch counts
    tbl = G._table(gpu)
    b = G.Batch(srv, gpu, [(NONE, -1, [sa(D + '/mine', MINE + RO)]),
                           (NONE, -1, [G.au(b'u:pw'),
                                       sa(D + '/mine', MINE + RO)]),
                           (NONE, -1, [G.au(b'u:bad'),
                                       sa(D + '/mine', RO)])],
                auth=tbl, setacl=True)
    assert b.errs == ['NO_AUTH', 'OK', 'OK', 'OK', 'NO_AUTH']
    assert acl_of(srv, gpu, D + '/mine')[0] == canon(MINE + RO)


def test_denied_frames_leave_the_store_alone(gpu):
    srv = _world(gpu)
    before = srv.acl_stats()
    top = int(srv.tree.acl[4][_lib.AC_TOP].item())
    fresh = [[ent(A.ALL, 'digest', 'new%d:x' % i)] for i in range(40)]
    b = one(srv, gpu, [sa(D + '/noadmin', v) for v in fresh] +
            [sa('/nope', v) for v in fresh] +
            [{'opcode': 'SET_ACL',
              'raw': jute.encode_request(dict(sa(leaf(1), fresh[0]),
                                              xid=0))[:-3]}],
            enforce=True)
    assert b.errs == ['NO_AUTH'] * 40 + ['NO_NODE'] * 40 + ['BAD_ARGUMENTS']
    assert srv.acl_stats() == before
    assert int(srv.tree.acl[4][_lib.AC_TOP].item()) == top
    # a BAD_VERSION frame has interned its vector (documented)
    b = one(srv, gpu, [sa(leaf(1), fresh[0], 5)], enforce=True)
    assert b.errs == ['BAD_VERSION']
    assert srv.acl_stats()[0] == before[0] + 1


# ---- the batch contract -----------------------------------------------------

def test_get_acl_of_the_batch_sees_the_new_acl(gpu):
    srv = _world(gpu)
    new = D + '/fresh'
    b = batch(srv, gpu, [
        (NONE, -1, [ga(leaf(7)), sa(leaf(7), THREE), ga(leaf(7))]),
        (NONE, -1, [T.mk(new, RO), sa(new, BIG), ga(new)])])
    assert b.errs == ['OK'] * 6
    assert b.reps[0]['acl'] == b.reps[2]['acl'] == canon(THREE)
    assert b.reps[2]['stat'].aversion == 1
    # the create of the batch was bound before the pass ran
    assert b.reps[5]['acl'] == canon(BIG)
    assert b.reps[4]['stat'].aversion == 1
    assert len(T.wire(BIG)) == 300
    assert acl_of(srv, gpu, new)[0] == canon(BIG)


def _serial(frames, aver, p=P):
    """The model of one node: frames [(index, version)] in frame order, one
    a round, ``p`` rounds -> {index: (err, aversion produced)}."""
    out = {}
    for r, (i, v) in enumerate(frames):
        if r >= p:
            out[i] = ('SYSTEM_ERROR', None)
        elif v != -1 and v != aver:
            out[i] = ('BAD_VERSION', None)
        else:
            aver += 1
            out[i] = ('OK', aver)
    return out


def test_one_node_in_frame_order(gpu):
    srv = _world(gpu)
    vec = [[ent(A.ALL, 'digest', 'v%d:x' % i)] for i in range(8)]
    # two of one wave; the same explicit version twice: exactly the first
    b = batch(srv, gpu, [(NONE, -1, [sa(leaf(10), vec[0]),
                                     sa(leaf(11), vec[2], 0)]),
                         (NONE, -1, [sa(leaf(10), vec[1]),
                                     sa(leaf(11), vec[3], 0)])])
    assert b.errs == ['OK', 'OK', 'OK', 'BAD_VERSION']
    assert [b.reps[i]['stat'].aversion for i in (0, 2)] == [1, 2]
    assert acl_of(srv, gpu, leaf(10))[0] == canon(vec[1])
    assert acl_of(srv, gpu, leaf(11))[0] == canon(vec[2])
    # frames 0, 64 and 256 of the class: a wave edge and a block edge
    pk = [sa(leaf(100 + i), RO) for i in range(257)]
    for k, i in enumerate((0, 64, 256)):
        pk[i] = sa(leaf(12), vec[k], k)
    b = one(srv, gpu, pk)
    assert b.errs == ['OK'] * 257
    assert [b.reps[i]['stat'].aversion for i in (0, 64, 256)] == [1, 2, 3]
    assert [b.reps[i]['zxid'] - b.zxid for i in (0, 64, 256)] == [1, 65, 257]
    assert acl_of(srv, gpu, leaf(12))[0] == canon(vec[2])
    # P + 1 on one node: the last is refused without effect, and counted
    un0 = srv.setacl_stats()['unreached']
    pk = [sa(leaf(13), vec[i], (-1, 0, 1, 9, -1)[i]) for i in range(P + 1)]
    b = one(srv, gpu, pk)
    want = _serial([(i, p['version']) for i, p in enumerate(pk)], 0)
    assert b.errs == [want[i][0] for i in range(P + 1)]
    assert b.errs == ['OK', 'BAD_VERSION', 'OK', 'BAD_VERSION',
                      'SYSTEM_ERROR']
    assert [b.reps[i]['stat'].aversion for i in (0, 2)] == [1, 2]
    assert b.frames[4] == HEAD.pack(16, 4, b.zxid, -1)
    assert srv.setacl_stats()['unreached'] == un0 + 1
    a, st = acl_of(srv, gpu, leaf(13))
    assert a == canon(vec[2]) and st.aversion == 2
    # the claim words are idle again
    assert bool((srv.setacl_claim == _lib.SETACL_IDLE).all().item())
    # more rounds reach it
    b = one(srv, gpu, [sa(leaf(14), vec[i]) for i in range(P + 1)],
            setacl_passes=P + 1)
    assert b.errs == ['OK'] * (P + 1)
    assert b.reps[P]['stat'].aversion == P + 1


def test_vector_alignments_and_one_entry_for_equal_vectors(gpu):
    srv = _world(gpu)
    ent0 = srv.acl_stats()[0]
    # a padded PING in front of each frame puts its vector at every
    # alignment of rx in turn
    rel = S.parse(jute.encode_request(dict(sa(leaf(40), THREE), xid=0)))[5]
    pk, o = [], 0
    for k in range(16):
        pad = (k - (o + 12 + 4 + rel)) % 16
        pk.append({'opcode': 'PING',
                   'raw': struct.pack('>ii', 0, 11) + b'\0' * pad})
        o += 12 + pad
        p = sa(leaf(40 + k), THREE, 0)
        assert (o + 4 + rel) % 16 == k
        o += 4 + len(jute.encode_request(dict(p, xid=0)))
        pk.append(p)
    b = one(srv, gpu, pk)
    assert b.errs == ['OK'] * 32
    assert srv.acl_stats()[0] == ent0 + 1
    for k in range(16):
        a, st = acl_of(srv, gpu, leaf(40 + k))
        assert a == canon(THREE) and st.aversion == 1
    # the same new vector from 65 frames on 65 nodes: one entry
    b = one(srv, gpu, [sa(leaf(200 + i), BIG) for i in range(65)])
    assert b.errs == ['OK'] * 65
    assert srv.acl_stats()[0] == ent0 + 2 and srv.acl_stats()[2] == 0
    assert acl_of(srv, gpu, leaf(264))[0] == canon(BIG)


def test_refused_dead_and_deferred_frames_do_nothing(gpu):
    from zkmi.server.engine import OrderDefer
    from zkmi.server.sessions import GpuSessionTable
    srv = _world(gpu)
    tab = GpuSessionTable(srv.tree, cap=64)
    sid = [tab.sid_of(k) for k in range(2)]
    for k in range(2):
        tab.sid[k] = sid[k]
        tab.state[k] = 1
    tab.next.fill_(2)
    tab.close(torch.tensor([sid[1]], dtype=I64, device=gpu))
    b = batch(srv, gpu, [(NONE, -1, [sa(leaf(20), RO)]),
                         (NONE, -1, [sa(leaf(21), RO), ga(leaf(21))])],
              sessions=sid, table=tab)
    assert b.errs == ['OK', 'SESSION_EXPIRED', 'SESSION_EXPIRED']
    assert acl_of(srv, gpu, leaf(21)) [0] == canon(OPEN)
    # an unsound table: every frame SYSTEMERROR, nothing applied
    conns = [(NONE, -1, [sa(leaf(22), RO)]), (NONE, -1, [sa(leaf(23), RO)])]
    n0 = len(jute.frame(jute.encode_request(dict(sa(leaf(22), RO), xid=0))))
    b = batch(srv, gpu, conns, starts=[0, n0 + 2, 2 * n0])
    assert b.errs == ['SYSTEM_ERROR'] * 2
    assert acl_of(srv, gpu, leaf(22))[0] == canon(OPEN)
    # a deferred frame: the segment's third write on one path is past the
    # two passes, and so is the SET_ACL behind it
    d = OrderDefer(1, gpu)
    z = srv.setacl_stats()
    b = one(srv, gpu, [T.wr(leaf(24)), T.wr(leaf(24)), T.wr(leaf(24)),
                       sa(leaf(25), RO)], ordered=True, passes=2, defer=d)
    assert b.errs == ['OK', 'OK', 'SYSTEM_ERROR', 'SYSTEM_ERROR']
    assert int(d.deferred.item()) == 2
    assert srv.setacl_stats() == z
    assert acl_of(srv, gpu, leaf(25))[0] == canon(OPEN)
    assert stat_of(srv, gpu, leaf(25)).aversion == 0


# ---- random frames against the sequential model -----------------------------

def test_random_frames_against_fakezk(gpu):
    from zkmi.server import FakeZKServer
    srv = _world(gpu)
    rng = np.random.RandomState(5)
    nodes = [leaf(300 + i) for i in range(40)] + \
        [D + '/ro', D + '/noadmin', D + '/net', D + '/mine']
    vecs = [OPEN, RO, NOADMIN, NETADMIN, MINE, THREE, BIG,
            [ent(A.ADMIN)], [ent(A.ADMIN, 'ip', '10.1.3.9')], []]
    addrs = [NET, OUT, NONE, NET]
    zk = FakeZKServer()
    try:
        db = zk.db
        zk.run(lambda: [db.create(p, b'', canon(OPEN), [], None)
                        for p in ('/bench', D, '/bench/d000003')])
        stats = {}
        for p in nodes:
            a, st = acl_of(srv, gpu, p)
            zk.run(lambda p=p, a=a: db.create(p, b'', a, [], None))
            stats[p] = st
        total = 0
        for rnd in range(8):
            n = 250
            frames = []
            for i in range(n):
                r = rng.randint(0, 20)
                path = '/nope%d' % i if r == 0 else \
                    nodes[int(rng.randint(len(nodes)))]
                frames.append((int(rng.randint(4)), sa(
                    path, vecs[int(rng.randint(len(vecs)))],
                    int(rng.randint(-1, 4)))))
            conns = [(addrs[s], -1, [p for c, p in frames if c == s])
                     for s in range(4)]
            flat = [(s, p) for s in range(4) for c, p in frames if c == s]
            start = {p: zk.run(lambda p=p: list(db.nodes[p].acl))
                     for p in nodes}
            rounds = {}
            want, reached = [], []
            for s, p in flat:
                path, acl, ver = p['path'], p['acl'], p['version']
                ok = path in start and S.admin(
                    S.SA_VECTOR, T.wire(start[path]), addrs[s]) if acl else 0
                if not acl:
                    want.append(('INVALID_ACL', None))
                elif path not in start:
                    want.append(('NO_NODE', None))
                elif not ok:
                    want.append(('NO_AUTH', None))
                elif rounds.get(path, 0) >= P:
                    want.append(('SYSTEM_ERROR', None))
                else:
                    rounds[path] = rounds.get(path, 0) + 1
                    reached.append(len(want))
                    try:
                        st = zk.run(lambda: db.set_acl(path, canon(acl), ver))
                        want.append(('OK', st.aversion))
                    except Exception as e:
                        want.append((e.code, None))
            b = batch(srv, gpu, conns, enforce=True)
            total += n
            zxs = {i: b.zxid + k + 1 for k, i in enumerate(reached)}
            for i, ((s, p), (err, av)) in enumerate(zip(flat, want)):
                if err == 'OK':
                    st = jute.Stat(*stats[p['path']].as_tuple())
                    st.aversion = av
                    exp = HEAD.pack(84, i, zxs[i], 0) + st.to_bytes()
                else:
                    code = {'SYSTEM_ERROR': -1}.get(err) or \
                        jute.consts.ERR_CODES[err]
                    exp = HEAD.pack(16, i, zxs.get(i, b.zxid), code)
                assert b.frames[i] == exp, (rnd, i, p, err)
        assert total == 2000
        # what the batches left: every node's ACL and Stat
        for p in nodes:
            a, st = acl_of(srv, gpu, p)
            node = zk.run(lambda p=p: (list(db.nodes[p].acl),
                                       db.nodes[p].stat.aversion))
            assert a == node[0], p
            want_st = jute.Stat(*stats[p].as_tuple())
            want_st.aversion = node[1]
            assert st == want_st, p
        z = srv.setacl_stats()
        assert z['applied'] > 100 and z['denied'] > 100 and \
            z['bad_version'] > 100 and z['unreached'] > 0 and \
            z['invalid'] > 100 and z['store_full'] == 0
    finally:
        zk.shutdown()


def test_snapshot_keeps_the_acl_and_the_aversion(gpu):
    from zkmi.server.tree import GpuTree
    srv = _world(gpu)
    b = one(srv, gpu, [sa(leaf(30), THREE), sa(leaf(30), MINE + RO)])
    assert b.errs == ['OK', 'OK']
    image = srv.tree.snapshot()
    tree2 = GpuTree.load(image, device=gpu, watch_cap=4096, acl_cap=64,
                         scratch=1 << 20)
    from zkmi.server.engine import GpuServer
    srv2 = GpuServer(tree2, 1024, 1 << 20, window=512)
    a, st = acl_of(srv2, gpu, leaf(30))
    assert a == canon(MINE + RO) and st.aversion == 2
    assert (a, st) == acl_of(srv, gpu, leaf(30))
