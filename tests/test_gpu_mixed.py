"""GpuServer.serve_mixed: a batch of any op mix served into one reply stream
in request order (csrc/kernels/tree_mix.hip around the three serve engines).

Two identical trees: X serves the mixed batch; Y serves the same requests
split on the host by the class rule, through the three existing entry points
in the engines' order — serve, serve_acl, serve_list.  The replies, decoded
with the jute oracle (children sorted), must be equal request by request, the
non-list replies byte for byte, and the trees' digests equal afterwards.
time.time is frozen so the Stats' times compare exactly."""

import struct
import time

import numpy as np
import pytest
import torch

from zkmi import consts, jute

pytestmark = pytest.mark.gpu

A, C, L = 0, 1, 2
NOW = 1_700_000_000.0
ACL2 = [{'perms': 0x1f, 'id': {'scheme': 'digest',
                               'id': 'bench:kQq8nOxk1NC8y2GdzFjp0v4ZbVY='}},
        {'perms': 0x01, 'id': {'scheme': 'ip', 'id': '10.0.0.7'}}]
LEAVES = {10: 400, 300: 900}


@pytest.fixture(autouse=True)
def _frozen_time(monkeypatch):
    monkeypatch.setattr(time, 'time', lambda: NOW)


def _dev_bytes(b, dev):
    a = np.frombuffer(bytes(b) if b else b'\0', np.uint8).copy()
    return torch.from_numpy(a).to(dev)


def _body(p):
    """A packet's request body: 'raw' bytes as they are, else the oracle's
    encoding less 'cut' bytes (a truncated request)."""
    if 'raw' in p:
        return p['raw']
    body = jute.encode_request(p)
    return body[:len(body) - p.get('cut', 0)]


def _stream(pk):
    return b''.join(jute.frame(_body(p)) for p in pk)


def _class(body, has_acl=True):
    """The class rule on the host (the split of tree Y's batches)."""
    if len(body) < 8:
        return A
    op = struct.unpack_from('>i', body, 4)[0]
    if op in (consts.OP_CODES['GET_CHILDREN'],
              consts.OP_CODES['GET_CHILDREN2']):
        return L
    if op == consts.OP_CODES['GET_ACL'] and has_acl:
        return C
    return A


def _replies(out, total, pk):
    """[(frame bytes, decoded reply)] of a reply stream; scan_frames must
    consume all of it."""
    raw = bytes(out[:int(total.item())].cpu().numpy().tobytes())
    frames, used, bad = jute.scan_frames(raw)
    assert bad < 0 and used == len(raw), (used, len(raw), bad)
    xmap = {p['xid']: p.get('opcode', 'PING') for p in pk}
    return [(raw[o - 4:o + ln], jute.decode_response(raw[o:o + ln], xmap))
            for o, ln in frames]


def _norm(rep):
    r = dict(rep)
    if 'children' in r:
        r['children'] = sorted(r['children'])
    if 'stat' in r:
        r['stat'] = r['stat'].as_tuple()
    return r


def _mixed(srv, pk, gpu, **kw):
    s = _stream(pk)
    out, total, err, ft = srv.serve_mixed(_dev_bytes(s, gpu), len(s), **kw)
    assert int(err.item()) == 0
    assert int(ft.count.item()) == len(pk)
    reps = _replies(out, total, pk)
    # in request order, with the request xids
    assert [r['xid'] for _, r in reps] == [p['xid'] for p in pk]
    rec = srv.last_rec_off[:len(pk)].cpu().tolist()
    assert rec == list(np.cumsum([0] + [len(f) for f, _ in reps])[:-1])
    return reps


def _homogeneous(srv, pk, gpu, session=0, wslot=-1, max_frame=None):
    """The same requests through serve, serve_acl, serve_list, in that order,
    on the host-split streams; the replies back in request order."""
    has_acl = srv.tree.acl is not None
    cls = [_class(_body(p), has_acl) for p in pk]
    part = {c: [p for p, k in zip(pk, cls) if k == c] for c in (A, C, L)}
    got = {A: [], C: [], L: []}
    notes = []
    if part[A]:
        s = _stream(part[A])
        out, total, err, _ = srv.serve(_dev_bytes(s, gpu), len(s),
                                       session=session, wslot=wslot)
        assert int(err.item()) == 0
        got[A] = _replies(out, total, part[A])
        if srv.tree.watch is not None:
            notes = _notes(srv)
    if part[C]:
        s = _stream(part[C])
        out, total, err, _ = srv.serve_acl(_dev_bytes(s, gpu), len(s))
        assert int(err.item()) == 0
        got[C] = _replies(out, total, part[C])
    if part[L]:
        s = _stream(part[L])
        out, total, err, _ = srv.serve_list(_dev_bytes(s, gpu), len(s),
                                            wslot=wslot, max_frame=max_frame)
        assert int(err.item()) == 0
        got[L] = _replies(out, total, part[L])
    its = {c: iter(got[c]) for c in got}
    return [next(its[c]) for c in cls], cls, notes


def _notes(srv):
    buf, total, slots, count = srv.notif
    n = int(count.item())
    raw = bytes(buf[:int(total.item())].cpu().numpy().tobytes())
    frames, _, bad = jute.scan_frames(raw)
    assert bad < 0 and len(frames) == n
    return [(s, pkt['type'], pkt['path']) for s, pkt in
            ((s, jute.decode_response(raw[o:o + ln], {}))
             for (o, ln), s in zip(frames, slots[:n].cpu().tolist()))]


def _compare(x, y, cls):
    assert len(x) == len(y) == len(cls)
    for k, ((fx, rx), (fy, ry), c) in enumerate(zip(x, y, cls)):
        assert _norm(rx) == _norm(ry), (k, rx, ry)
        if c != L:
            assert fx == fy, (k, fx.hex(), fy.hex())
        else:
            assert len(fx) == len(fy)


def _pair(gpu, fanout, frames=1024, acl=True, watch=True):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    out = []
    for _ in range(2):
        tree = GpuTree(LEAVES[fanout], 16, fanout=fanout, device=gpu,
                       spare=4.0, ctime_ms=int(NOW * 1000),
                       acl_cap=512 if acl else 0,
                       watch_cap=256 if watch else 0)
        out.append(GpuServer(tree, frames, 1 << 20, window=512))
    return out


def _leaf(fanout, i):
    return '/bench/d%06d/n%09d' % (i // fanout, i)


def _patterns(n):
    rng = np.random.default_rng(99 + n)
    i = np.arange(n)
    pats = [('rotation', np.array([A, L, C])[i % 3]),
            ('runs70', np.array([A, C, L])[(i // 70) % 3]),
            ('random', rng.integers(0, 3, n))]
    pats += [('only%d' % c, np.full(n, c)) for c in (A, C, L)]
    pats += [('pair%d%d' % (a, b),
              np.where(rng.integers(0, 2, n) == 0, a, b))
             for a, b in ((A, C), (A, L), (C, L))]
    return pats


def _batch(classes, fanout, gen):
    """Requests of the given classes, xids 1000.. in request order.  No two
    requests of a batch touch one path when one of them writes it (a batch's
    writes are concurrent): gets read leaves 0..99, sets write leaves
    100..249, creates make fresh names of generation `gen`, deletes take
    leaves from 250 on (15 a generation) and then the names generation
    `gen - 1` made (NO_NODE where it made none).  Lists and
    GET_ACLs see the batch's writes on both trees alike."""
    ndirs = LEAVES[fanout] // fanout
    pk = []
    na = 0
    for k, c in enumerate(classes):
        x = 1000 + k
        if c == L:
            op = 'GET_CHILDREN2' if k % 2 else 'GET_CHILDREN'
            path = ('/bench/d%06d' % (k % ndirs), _leaf(fanout, k % 100),
                    '/bench', '/bench/nope%d' % k)[(k // 2) % 4]
            pk.append({'xid': x, 'opcode': op, 'path': path, 'watch': False})
        elif c == C:
            path = (_leaf(fanout, k % 100), '/bench/d%06d' % (k % ndirs),
                    '/bench/d000000/c%d_%d' % (gen - 1, k - 1),
                    '/bench/nope%d' % k)[k % 4]
            pk.append({'xid': x, 'opcode': 'GET_ACL', 'path': path})
        else:
            kind, j = na % 7, na // 7
            na += 1
            d = '/bench/d%06d' % (k % ndirs)
            if kind == 0:
                p = {'opcode': 'GET_DATA', 'path': _leaf(fanout, k % 100),
                     'watch': False}
            elif kind == 1:
                p = {'opcode': 'EXISTS', 'watch': False, 'path':
                     _leaf(fanout, k % 100) if j % 2 else d + '/nope'}
            elif kind == 2:
                p = {'opcode': 'SET_DATA', 'path': _leaf(fanout, 100 + j),
                     'data': b'set-%d-%d' % (gen, k), 'version': -1}
            elif kind == 3:
                p = {'opcode': 'CREATE', 'path': '%s/c%d_%d' % (d, gen, k),
                     'data': b'c%d' % k, 'acl': jute.DEFAULT_ACL,
                     'flags': []}
            elif kind == 4:
                p = {'opcode': 'CREATE', 'path':
                     '/bench/d000000/c%d_%d' % (gen, k),
                     'data': b'', 'acl': ACL2, 'flags': []}
            elif kind == 5:
                p = {'opcode': 'DELETE', 'version': -1, 'path':
                     _leaf(fanout, 250 + 15 * gen + j) if j < 15 else
                     '/bench/d000000/c%d_%d' % (gen - 1, k - 1)}
            else:
                p = {'opcode': 'SYNC', 'path': d}
            pk.append(dict(p, xid=x))
    return pk


@pytest.mark.parametrize('fanout', [10, 300])
@pytest.mark.parametrize('n', [1, 64, 65, 257, 600])
def test_mixed_equals_the_three_entry_points(gpu, fanout, n):
    """Every interleaving (rotation, runs of 70, random, each class alone,
    each pair) of GET_DATA, EXISTS, SET_DATA, CREATE with and without an ACL
    of its own, DELETE, SYNC, both list ops and GET_ACL: decoded replies
    equal request by request, non-list replies byte-equal, the whole stream
    framed, xids in request order, the two trees' digests equal."""
    sx, sy = _pair(gpu, fanout)
    for gen, (name, classes) in enumerate(_patterns(n)):
        pk = _batch(classes, fanout, gen)
        x = _mixed(sx, pk, gpu)
        y, cls, _ = _homogeneous(sy, pk, gpu)
        assert cls == [int(c) for c in classes], name
        _compare(x, y, cls)
        assert sx.tree.digest() == sy.tree.digest(), name
    assert sx.acl_stats() == sy.acl_stats()


def test_same_batch_visibility(gpu):
    """The batch contract: a list and a GET_ACL see the tree after the
    batch's writes — the created child is listed, the deleted one is not,
    the GET_ACL of a node created in the batch returns its ACL."""
    sx, sy = _pair(gpu, 10)
    d0, d1 = '/bench/d000000', '/bench/d000001'
    gone = _leaf(10, 13)
    pk = [{'xid': 1, 'opcode': 'GET_CHILDREN2', 'path': d0},
          {'xid': 2, 'opcode': 'GET_ACL', 'path': d0 + '/new'},
          {'xid': 3, 'opcode': 'GET_CHILDREN', 'path': d1},
          {'xid': 4, 'opcode': 'CREATE', 'path': d0 + '/new', 'data': b'x',
           'acl': ACL2, 'flags': []},
          {'xid': 5, 'opcode': 'DELETE', 'path': gone, 'version': -1},
          {'xid': 6, 'opcode': 'GET_CHILDREN2', 'path': d1}]
    xf = _mixed(sx, pk, gpu)
    x = [r for _, r in xf]
    assert [r['err'] for r in x] == ['OK'] * 6
    assert 'new' in x[0]['children'] and len(x[0]['children']) == 11
    assert x[0]['stat'].numChildren == 11
    wire = jute.decode_request(jute.encode_request(pk[3]))['acl']
    assert x[1]['acl'] == wire
    name = gone.rpartition('/')[2]
    assert name not in x[2]['children'] and len(x[2]['children']) == 9
    assert sorted(x[5]['children']) == sorted(x[2]['children'])
    assert x[5]['stat'].numChildren == 9
    y, cls, _ = _homogeneous(sy, pk, gpu)
    _compare(xf, y, cls)
    assert sx.tree.digest() == sy.tree.digest()


def test_watches(gpu):
    """A watch=1 list of a mixed batch arms the child watch of slot wslot
    after the batch's writes: a create of the same batch does not fire it,
    a create of the next (mixed) batch does, and that batch's srv.notif
    carries the event — with the data watch a GET_DATA of the first batch
    armed — as the homogeneous path reports them."""
    sx, sy = _pair(gpu, 10)
    d0 = '/bench/d000000'
    leaf = _leaf(10, 3)
    first = [{'xid': 1, 'opcode': 'CREATE', 'path': d0 + '/kidA',
              'data': b'', 'acl': jute.DEFAULT_ACL, 'flags': []},
             {'xid': 2, 'opcode': 'GET_CHILDREN2', 'path': d0,
              'watch': True},
             {'xid': 3, 'opcode': 'GET_DATA', 'path': leaf, 'watch': True},
             {'xid': 4, 'opcode': 'GET_ACL', 'path': d0},
             {'xid': 5, 'opcode': 'GET_CHILDREN', 'path': d0 + '/nope',
              'watch': True}]
    x = _mixed(sx, first, gpu, wslot=3)
    assert _notes(sx) == []                    # the same batch: not fired
    y, cls, ynotes = _homogeneous(sy, first, gpu, wslot=3)
    _compare(x, y, cls)
    assert ynotes == []
    assert 'kidA' in x[1][1]['children']
    second = [{'xid': 6, 'opcode': 'GET_CHILDREN', 'path': d0},
              {'xid': 7, 'opcode': 'CREATE', 'path': d0 + '/kidB',
               'data': b'', 'acl': ACL2, 'flags': []},
              {'xid': 8, 'opcode': 'GET_ACL', 'path': leaf},
              {'xid': 9, 'opcode': 'SET_DATA', 'path': leaf, 'data': b'w',
               'version': -1},
              {'xid': 10, 'opcode': 'CREATE', 'path': d0 + '/nope',
               'data': b'', 'acl': jute.DEFAULT_ACL, 'flags': []}]
    x = _mixed(sx, second, gpu, wslot=3)
    xnotes = _notes(sx)
    y, cls, ynotes = _homogeneous(sy, second, gpu, wslot=3)
    _compare(x, y, cls)
    assert xnotes == ynotes
    # one child event on d0 (one-shot: kidB fired it, /nope found it gone;
    # the missing path's list armed nothing), one data event on the leaf
    assert sorted(xnotes) == sorted([(3, 'CHILDREN_CHANGED', d0),
                                     (3, 'DATA_CHANGED', leaf)])
    third = [{'xid': 11, 'opcode': 'CREATE', 'path': d0 + '/kidC',
              'data': b'', 'acl': jute.DEFAULT_ACL, 'flags': []},
             {'xid': 12, 'opcode': 'GET_CHILDREN', 'path': d0}]
    _mixed(sx, third, gpu, wslot=3)
    assert _notes(sx) == []
    assert sx.tree.digest()[0] != 0


def _malformed(x0):
    ls = jute.encode_request({'xid': x0, 'opcode': 'GET_CHILDREN2',
                              'path': '/bench/d000001', 'watch': False})
    ga = jute.encode_request({'xid': x0 + 1, 'opcode': 'GET_ACL',
                              'path': '/bench/d000001'})
    gd = jute.encode_request({'xid': x0 + 3, 'opcode': 'GET_DATA',
                              'path': '/bench/d000001', 'watch': False})
    return [
        {'xid': x0, 'opcode': 'GET_CHILDREN2', 'raw': ls[:-1]},
        {'xid': x0 + 1, 'opcode': 'GET_ACL', 'raw': ga[:-1]},
        # six bytes: no opcode word; the reply carries xid 0
        {'xid': 0, 'opcode': 'PING', 'raw': struct.pack('>i', x0 + 2) + b'\0\0'},
        {'xid': x0 + 3, 'opcode': 'GET_DATA',
         'raw': gd[:4] + struct.pack('>i', 9999) + gd[8:]},
        {'xid': x0 + 4, 'opcode': 'GET_CHILDREN', 'raw':
         struct.pack('>ii', x0 + 4, 8) + ls[8:11]},  # cut inside the length
        {'xid': x0 + 5, 'opcode': 'GET_ACL',
         'raw': struct.pack('>ii', x0 + 5, 6)},
    ]


def test_malformed_frames(gpu):
    """A truncated list frame, a truncated GET_ACL frame, a 6-byte frame and
    an unknown opcode between well-formed requests: the answers of the
    homogeneous paths (BAD_ARGUMENTS, from the frame's own engine), header
    only."""
    sx, sy = _pair(gpu, 10)
    good = _batch(np.array([A, L, C] * 4), 10, 0)
    bad = _malformed(5000)
    pk = good[:5] + bad[:3] + good[5:9] + bad[3:] + good[9:]
    x = _mixed(sx, pk, gpu)
    y, cls, _ = _homogeneous(sy, pk, gpu)
    _compare(x, y, cls)
    by = {r['xid']: (r['err'], len(f)) for f, r in x}
    assert by[5000] == ('BAD_ARGUMENTS', 20)
    assert by[5001] == ('BAD_ARGUMENTS', 20)
    assert by[0] == ('BAD_ARGUMENTS', 20)
    assert by[5003] == ('BAD_ARGUMENTS', 20)
    assert by[5004] == ('BAD_ARGUMENTS', 20)
    assert by[5005] == ('BAD_ARGUMENTS', 20)
    assert [cls[5], cls[6], cls[7], cls[12], cls[13], cls[14]] == \
        [L, C, A, A, L, C]
    assert sx.tree.digest() == sy.tree.digest()


def test_tree_without_acl_table(gpu):
    """No ACL table: GET_ACL is the serve's and answered UNIMPLEMENTED; the
    rest of the batch is served."""
    sx, sy = _pair(gpu, 10, acl=False)
    pk = _batch(np.array([A, C, L] * 30), 10, 0)
    x = _mixed(sx, pk, gpu)
    y, cls, _ = _homogeneous(sy, pk, gpu)
    assert C not in cls
    _compare(x, y, cls)
    for p, (_, r) in zip(pk, x):
        if p['opcode'] == 'GET_ACL':
            assert r['err'] == 'UNIMPLEMENTED'
    assert sum(r['err'] == 'OK' for _, r in x) > 40
    assert sx.tree.digest() == sy.tree.digest()


def _read_only(fanout, n):
    pk = []
    for k in range(n):
        x = 100 + k
        kind = k % 4
        if kind == 0:
            pk.append({'xid': x, 'opcode': 'GET_DATA', 'watch': False,
                       'path': _leaf(fanout, k)})
        elif kind == 1:
            pk.append({'xid': x, 'opcode': 'GET_CHILDREN2', 'watch': False,
                       'path': '/bench/d%06d' % (k % 3)})
        elif kind == 2:
            pk.append({'xid': x, 'opcode': 'GET_ACL',
                       'path': _leaf(fanout, k)})
        else:
            pk.append({'xid': x, 'opcode': 'GET_CHILDREN', 'watch': False,
                       'path': _leaf(fanout, k)})
    return pk


def test_overflow_and_max_frame(gpu):
    """out one byte short of the merged stream: err 2, total 0, not a byte
    written; exactly enough: the whole stream.  max_frame demotes the large
    list replies to SYSTEMERROR headers as serve_list does, the replies
    around them whole."""
    sx, sy = _pair(gpu, 300)
    pk = _read_only(300, 40)
    s = _stream(pk)
    rx = _dev_bytes(s, gpu)
    _, total, err, _ = sx.serve_mixed(rx, len(s))
    T = int(total.item())
    assert int(err.item()) == 0 and T > 10 * 300 * 14
    out = torch.full((T - 1,), 0xAB, dtype=torch.uint8, device=gpu)
    o, total, err, _ = sx.serve_mixed(rx, len(s), out=out)
    assert o is out and int(err.item()) == 2 and int(total.item()) == 0
    assert bool((out == 0xAB).all().item())
    out = torch.full((T,), 0xAB, dtype=torch.uint8, device=gpu)
    o, total, err, _ = sx.serve_mixed(rx, len(s), out=out, terminate=True)
    assert int(err.item()) == 0 and int(total.item()) == T
    whole = _replies(out, total, pk)
    # (every served batch moves the zxid on: a fresh pair for the comparison)
    sx, sy = _pair(gpu, 300)
    x = _mixed(sx, pk, gpu, max_frame=256)
    y, cls, _ = _homogeneous(sy, pk, gpu, max_frame=256)
    _compare(x, y, cls)
    for p, (f, r), (fw, rw) in zip(pk, x, whole):
        if p['opcode'] == 'GET_CHILDREN2':
            assert r['err'] == 'SYSTEM_ERROR' and len(f) == 20
            assert len(rw['children']) == 300
        else:
            assert r['err'] == 'OK' and len(f) == len(fw)
            assert dict(_norm(r), zxid=0) == dict(_norm(rw), zxid=0)


def test_empty_batch_with_terminator(gpu):
    sx, _ = _pair(gpu, 10)
    rx = torch.zeros(64, dtype=torch.uint8, device=gpu)
    out, total, err, ft = sx.serve_mixed(rx, 0, terminate=True)
    assert int(total.item()) == 0 and int(err.item()) == 0
    assert int(ft.count.item()) == 0
    assert out[:4].cpu().tolist() == [0xFF] * 4
    # and after a batch that left rows in every table
    _mixed(sx, _batch(np.array([A, C, L] * 5), 10, 0), gpu)
    out, total, err, _ = sx.serve_mixed(rx, 0, terminate=True)
    assert int(total.item()) == 0 and int(err.item()) == 0
    assert out[:4].cpu().tolist() == [0xFF] * 4


def test_refusals(gpu):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    rx = torch.zeros(64, dtype=torch.uint8, device=gpu)
    tree = GpuTree(100, 16, fanout=10, device=gpu)
    srv = GpuServer(tree, 64, 1 << 16, seq_order=False, fused_rows=True)
    with pytest.raises(ValueError, match='fused_rows'):
        srv.serve_mixed(rx, 0)
    tree = GpuTree(100, 16, fanout=10, device=gpu, shard=(0, 2))
    srv = GpuServer(tree, 64, 1 << 16)
    with pytest.raises(ValueError, match='sharded'):
        srv.serve_mixed(rx, 0)


def test_capture_replay(gpu):
    """After a warm-up call a read-only mixed batch is captured on one stream
    and replayed three times: the decoded replies of every replay equal the
    eager ones.  The header's zxid is the one field that moves: the serve
    advances the tree's zxid by its requests every batch, reads included, so
    it is compared apart — every replay's is the one before plus the batch's
    25 serve-class requests (capturing itself runs nothing)."""
    sx, _ = _pair(gpu, 10)
    pk = _read_only(10, 97)
    s = _stream(pk)
    rx = _dev_bytes(s, gpu)
    n_serve = sum(p['opcode'] == 'GET_DATA' for p in pk)
    first = [_norm(r) for _, r in _mixed(sx, pk, gpu, terminate=True)]
    eager = [dict(r, zxid=0) for r in first]
    zxid = first[0]['zxid']
    torch.cuda.synchronize(gpu)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        out, total, err, _ = sx.serve_mixed(rx, len(s), terminate=True)
    for _ in range(3):
        out.fill_(0)
        g.replay()
        torch.cuda.synchronize(gpu)
        assert int(err.item()) == 0
        got = [_norm(r) for _, r in _replies(out, total, pk)]
        zxid += n_serve
        # (the serve's replies carry the batch's base, the two engines
        # behind it the zxid the serve left)
        assert [r['zxid'] for r in got] == [
            zxid if p['opcode'] == 'GET_DATA' else zxid + n_serve
            for p in pk]
        assert [dict(r, zxid=0) for r in got] == eager
        T = int(total.item())
        assert out[T:T + 4].cpu().tolist() == [0xFF] * 4
