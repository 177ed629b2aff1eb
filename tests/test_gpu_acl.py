"""The GPU server's ACL path (csrc/kernels/tree_acl.hip): the ACL table
beside the HBM tree, the pass that records every CREATE's ACL after a serve,
and GpuServer.serve_acl answering GET_ACL batches.  Replies are decoded with
the jute oracle; the expected ACLs come from a model the test keeps with
fakezk's create / get_acl rules (a successful create stores the request's
ACL, pre-made nodes carry the open ACL).
Reference: lib/zk-buffer.js (GET_ACL request and reply); lib/client.js
getACL()."""

import types

import numpy as np
import pytest
import torch

from zkmi import jute
from zkmi.ops import _lib

pytestmark = pytest.mark.gpu

OPEN = jute.decode_request(jute.encode_request(
    {'xid': 0, 'opcode': 'CREATE', 'path': '/x', 'data': b'',
     'acl': jute.DEFAULT_ACL, 'flags': []}))['acl']
OPEN_FRAME = 16 + 27 + 68


def _dev_bytes(b, dev):
    a = np.frombuffer(bytes(b) if b else b'\0', np.uint8).copy()
    return torch.from_numpy(a).to(dev)


def _ga(x, path):
    return {'xid': x, 'opcode': 'GET_ACL', 'path': path}


def _create(x, path, acl, flags=()):
    return {'xid': x, 'opcode': 'CREATE', 'path': path, 'data': b'c',
            'acl': acl, 'flags': list(flags)}


def _wire_acl(p):
    """The oracle's decode of the request's own bytes."""
    return jute.decode_request(jute.encode_request(p))['acl']


def _acl_len(acl):
    w = jute.JuteWriter()
    w.write_acl(acl)
    return len(w.getvalue())


def _frames(pk):
    out = []
    for p in pk:
        body = jute.encode_request(p)
        out.append(jute.frame(body[:len(body) - p.get('cut', 0)]))
    return b''.join(out)


def _decode(out, total, pk):
    raw = bytes(out[:int(total.item())].cpu().numpy().tobytes())
    frames, used, bad = jute.scan_frames(raw)
    assert bad < 0 and used == len(raw), (used, len(raw), bad)
    xmap = {p['xid']: p['opcode'] for p in pk}
    reps = [jute.decode_response(raw[o:o + ln], xmap) for o, ln in frames]
    for (o, ln), r in zip(frames, reps):
        r['_len'] = ln
    return reps


def _get(srv, pk, gpu, **kw):
    s = _frames(pk)
    out, total, err, _ = srv.serve_acl(_dev_bytes(s, gpu), len(s), **kw)
    assert int(err.item()) == 0
    reps = _decode(out, total, pk)
    assert [r['xid'] for r in reps] == [p['xid'] for p in pk]
    return reps


def _get_paths(srv, paths, gpu, x0=50_000, chunk=None):
    chunk = chunk or srv.cap_frames
    reps = []
    for k in range(0, len(paths), chunk):
        reps += _get(srv, [_ga(x0 + k + j, p)
                           for j, p in enumerate(paths[k:k + chunk])], gpu)
    return reps


def _serve(srv, pk, gpu, session=0, **kw):
    s = _frames(pk)
    out, total, _, _ = srv.serve(_dev_bytes(s, gpu), len(s), session=session,
                                 **kw)
    return _decode(out, total, pk)


def _check_ok(rep, acl):
    assert rep['err'] == 'OK', rep
    assert rep['acl'] == acl
    assert rep['_len'] == 16 + _acl_len(acl) + 68
    assert rep['stat'].aversion == 0


def _ident(scheme, ident):
    return {'scheme': scheme, 'id': ident}


def _acl_vectors(k):
    """k distinct ACL vectors of 1 to 4 entries: byte lengths that are no
    multiples of 4 or 16 among them, an empty id string, a digest id of 40
    bytes, and vectors 0 and 1 differing only in their last perms byte."""
    digest = 'bench:' + 'kQq8nOxk1NC8y2GdzFjp0v4ZbVY=' + 'abcdef'
    assert len(digest) == 40
    base = [
        [{'perms': 0x1f, 'id': _ident('digest', digest)},
         {'perms': 0x01, 'id': _ident('ip', '10.0.0.7')}],
        [{'perms': 0x1f, 'id': _ident('digest', digest)},
         {'perms': 0x03, 'id': _ident('ip', '10.0.0.7')}],
        [{'perms': 0x05, 'id': _ident('world', '')}],
        [{'perms': 0x09, 'id': _ident('world', 'anyone')},
         {'perms': 0x11, 'id': _ident('auth', '')},
         {'perms': 0x02, 'id': _ident('ip', '192.168.1.13/24')},
         {'perms': 0x1f, 'id': _ident('digest', digest)}],
        [{'perms': 0x07, 'id': _ident('sasl', 'bob')},
         {'perms': 0x1b, 'id': _ident('x509', 'CN=a,O=b')},
         {'perms': 0x04, 'id': _ident('ip', '::1')}],
    ]
    out = base[:k]
    j = 0
    while len(out) < k:
        n = 1 + j % 4
        out.append([{'perms': 1 + (j + e) % 31,
                     'id': _ident('ip', 'h%d.%s' % (j, 'x' * ((j + e) % 7)))}
                    for e in range(n)])
        j += 1
    lens = {_acl_len(a) for a in out}
    if k >= 5:
        assert any(ln % 4 for ln in lens) and any(ln % 16 for ln in lens)
    assert len({repr(a) for a in out}) == k
    return out


def _setup(gpu, n=300, fanout=100, frames=1024, **kw):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    kw.setdefault('acl_cap', 512)
    kw.setdefault('spare', 4.0)
    tree = GpuTree(n, 16, fanout=fanout, device=gpu, **kw)
    srv = GpuServer(tree, frames, 1 << 20, window=512)
    return tree, srv


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_static_tree(gpu, n):
    """Batches of 1 / 63 / 64 / 65 / 257 requests (wave and block edges) over
    static nodes: every reply is the open ACL in a 115-byte frame with the
    Stat EXISTS returns, in request order with the request xids and the
    zxid of the EXISTS batch; a missing path and / (NO_NODE), a GET_DATA
    frame (UNIMPLEMENTED) and a frame cut by one byte (BAD_ARGUMENTS) in the
    same batch are answered header only."""
    tree, srv = _setup(gpu)
    paths = ['/bench', '/bench/d000001'] + \
        ['/bench/d%06d/n%09d' % (i // 100, i) for i in range(300)]
    paths = [paths[(7 * k) % len(paths)] for k in range(n)]
    pk = [_ga(100 + k, p) for k, p in enumerate(paths)]
    x = 100 + n
    pk += [_ga(x, '/bench/nope'), _ga(x + 1, '/'),
           {'xid': x + 2, 'opcode': 'GET_DATA', 'path': paths[0],
            'watch': False},
           dict(_ga(x + 3, paths[0]), cut=1)]
    reps = _get(srv, pk, gpu)
    assert len(reps) == len(pk)
    for r in reps[:n]:
        _check_ok(r, OPEN)
        assert r['_len'] == OPEN_FRAME == 115 - 4
    assert [r['err'] for r in reps[n:]] == [
        'NO_NODE', 'NO_NODE', 'UNIMPLEMENTED', 'BAD_ARGUMENTS']
    assert all(r['_len'] == 16 for r in reps[n:])
    ex = _serve(srv, [{'xid': p['xid'], 'opcode': 'EXISTS',
                       'path': p['path'], 'watch': False} for p in pk[:n]],
                gpu)
    for e, r in zip(ex, reps):
        assert e['err'] == 'OK' and e['xid'] == r['xid']
        assert e['stat'].as_tuple() == r['stat'].as_tuple()
    assert all(r['zxid'] == ex[0]['zxid'] for r in reps)
    assert tree.acl_host(0) == OPEN
    assert srv.acl_stats() == (1, 27, 0)


@pytest.mark.parametrize('k', [1, 2, 65, 300])
def test_creates_bind_their_acl(gpu, k):
    """600 creates whose ACLs cycle over k distinct vectors (one, a few, more
    than 64 per wave): every created path answers the ACL it was created
    with, byte for byte; the table holds k entries beside the open ACL and
    lost nothing; a second batch with the same ACLs adds no entry and no
    arena byte."""
    tree, srv = _setup(gpu)
    acls = _acl_vectors(k)
    pk = [_create(1000 + i, '/bench/d%06d/c%04d' % (i % 3, i), acls[i % k])
          for i in range(600)]
    reps = _serve(srv, pk, gpu)
    assert [r['err'] for r in reps] == ['OK'] * 600
    got = _get_paths(srv, [p['path'] for p in pk], gpu)
    for p, r in zip(pk, got):
        _check_ok(r, _wire_acl(p))
    ent, used, lost = srv.acl_stats()
    assert (ent, lost) == (k + 1, 0)
    assert used == 27 + sum(_acl_len(a) for a in acls)
    v = tree.find_host(pk[1]['path'])
    assert tree.acl_host(v) == _wire_acl(pk[1])
    pk2 = [_create(3000 + i, '/bench/d%06d/e%04d' % (i % 3, i),
                   acls[(i + 1) % k]) for i in range(600)]
    reps = _serve(srv, pk2, gpu)
    assert [r['err'] for r in reps] == ['OK'] * 600
    assert srv.acl_stats() == (ent, used, 0)
    got = _get_paths(srv, [p['path'] for p in pk2], gpu)
    for p, r in zip(pk2, got):
        _check_ok(r, _wire_acl(p))
    # the open ACL is interned from the start: a create with it adds nothing
    r = _serve(srv, [_create(9000, '/bench/d000000/open', jute.DEFAULT_ACL)],
               gpu)
    assert r[0]['err'] == 'OK' and srv.acl_stats() == (ent, used, 0)
    _check_ok(_get(srv, [_ga(9001, '/bench/d000000/open')], gpu)[0], OPEN)


def test_what_must_not_bind(gpu):
    """Failed creates (NODE_EXISTS with another ACL, a missing parent, an
    empty ACL) bind nothing and intern nothing; SEQUENTIAL and EPHEMERAL
    creates answer under the returned name, and after the session's expiry
    the ephemeral paths answer NO_NODE."""
    tree, srv = _setup(gpu)
    a, b, c, d = _acl_vectors(4)
    base = '/bench/d000001'
    r = _serve(srv, [_create(1, base + '/keep', a)], gpu)
    assert r[0]['err'] == 'OK'
    ent0 = srv.acl_stats()[0]
    assert ent0 == 2
    r = _serve(srv, [_create(2, base + '/keep', b),
                     _create(3, '/bench/missing/kid', c),
                     _create(4, base + '/empty', []),
                     _create(5, base + '/n000000100', d)], gpu)
    assert [x['err'] for x in r] == ['NODE_EXISTS', 'NO_NODE', 'INVALID_ACL',
                                     'NODE_EXISTS']
    assert srv.acl_stats() == (ent0, 27 + _acl_len(a), 0)
    got = _get(srv, [_ga(6, base + '/keep'), _ga(7, base + '/n000000100'),
                     _ga(8, base + '/empty'), _ga(9, '/bench/missing/kid')],
               gpu)
    _check_ok(got[0], _wire_acl(_create(0, '/', a)))
    _check_ok(got[1], OPEN)
    assert [x['err'] for x in got[2:]] == ['NO_NODE', 'NO_NODE']
    # SEQUENTIAL and EPHEMERAL creates, under the names the replies give
    pk = [_create(20 + i, base + '/seq-', b if i % 2 else c, ['SEQUENTIAL'])
          for i in range(10)]
    pk += [_create(40 + i, base + '/eph%02d' % i, d, ['EPHEMERAL'])
           for i in range(10)]
    r = _serve(srv, pk, gpu, session=0x77)
    assert [x['err'] for x in r] == ['OK'] * 20
    names = [x['path'] for x in r]
    assert len(set(names)) == 20 and all(len(nm) == len(base) + 15
                                         for nm in names[:10])
    got = _get_paths(srv, names, gpu)
    for p, g in zip(pk, got):
        _check_ok(g, _wire_acl(p))
    assert srv.acl_stats()[::2] == (ent0 + 3, 0)
    assert int(tree.expire(0x77).item()) == 10
    got = _get_paths(srv, names, gpu)
    assert [g['err'] for g in got] == ['OK'] * 10 + ['NO_NODE'] * 10
    assert all(g['_len'] == 16 for g in got[10:])


def test_recycled_nodes(gpu):
    """20 created nodes deleted, 20 others created under another parent
    with another ACL on the freed node slots: the new paths show the new
    ACL, the deleted paths answer NO_NODE."""
    tree, srv = _setup(gpu, spare=2.0)
    a, b = _acl_vectors(2)
    old = ['/bench/d000000/old%02d' % i for i in range(20)]
    new = ['/bench/d000002/new%02d' % i for i in range(20)]
    r = _serve(srv, [_create(100 + i, p, a) for i, p in enumerate(old)], gpu)
    assert [x['err'] for x in r] == ['OK'] * 20
    nodes = {tree.find_host(p) for p in old}
    r = _serve(srv, [{'xid': 200 + i, 'opcode': 'DELETE', 'path': p,
                      'version': -1} for i, p in enumerate(old)], gpu)
    assert [x['err'] for x in r] == ['OK'] * 20
    hw = int(tree.counters[_lib.TC_NODES].item())
    r = _serve(srv, [_create(300 + i, p, b) for i, p in enumerate(new)], gpu)
    assert [x['err'] for x in r] == ['OK'] * 20
    assert int(tree.counters[_lib.TC_NODES].item()) == hw     # recycled
    assert {tree.find_host(p) for p in new} == nodes
    got = _get_paths(srv, new + old, gpu)
    for g in got[:20]:
        _check_ok(g, _wire_acl(_create(0, '/', b)))
    assert [g['err'] for g in got[20:]] == ['NO_NODE'] * 20
    assert srv.acl_stats()[::2] == (3, 0)


def test_ordered_serve(gpu):
    """serve(ordered=True): create -> set -> get on one path in one batch,
    and a create -> delete pair: the surviving node answers its ACL, the
    deleted one NO_NODE."""
    tree, srv = _setup(gpu, scratch=1 << 16)
    a, b = _acl_vectors(2)
    p, q = '/bench/d000001/stay', '/bench/d000001/gone'
    pk = [_create(1, p, a),
          {'xid': 2, 'opcode': 'SET_DATA', 'path': p, 'data': b'zz',
           'version': -1},
          {'xid': 3, 'opcode': 'GET_DATA', 'path': p, 'watch': False},
          _create(4, q, b),
          {'xid': 5, 'opcode': 'DELETE', 'path': q, 'version': -1}]
    r = _serve(srv, pk, gpu, ordered=True, passes=4)
    assert [x['err'] for x in r] == ['OK'] * 5
    assert r[2]['data'] == b'zz'
    got = _get(srv, [_ga(6, p), _ga(7, q)], gpu)
    _check_ok(got[0], _wire_acl(pk[0]))
    assert got[1]['err'] == 'NO_NODE' and got[1]['_len'] == 16
    assert srv.acl_stats()[::2] == (3, 0)


@pytest.mark.parametrize('kind', ['entries', 'arena'])
def test_full_store(gpu, kind):
    """A table with room for 4 ACLs, and one whose arena holds the open ACL
    plus 100 bytes, the arena a view into a larger 0xAB-filled tensor: ten
    creates with ten distinct ACLs, one per batch, all answer OK; those
    whose ACL found room answer it, the rest SYSTEMERROR header only;
    ``lost`` counts them and no byte past the arena changed."""
    if kind == 'entries':
        tree, srv = _setup(gpu, acl_cap=4)
    else:
        tree, srv = _setup(gpu, acl_cap=64, acl_arena_bytes=127)
    acap = tree.acl[1].numel()
    big = torch.full((acap + 4096,), 0xAB, dtype=torch.uint8, device=gpu)
    big[:acap] = tree.acl[1]
    tree.acl[1] = big[:acap]
    acls = _acl_vectors(10)
    acls = [acls[2], acls[4]] + acls[5:] + [acls[0], acls[1], acls[3]]
    pk = [_create(10 + i, '/bench/d000000/f%02d' % i, acls[i])
          for i in range(10)]
    for p in pk:
        r = _serve(srv, [p], gpu)
        assert r[0]['err'] == 'OK'
    got = _get_paths(srv, [p['path'] for p in pk], gpu)
    # the model: one create per batch, so the vectors arrive in order.  The
    # entry limit refuses the fifth and later ones; the arena is a bump
    # allocator, so a vector that does not fit still moves its top and the
    # arena then counts as full
    fits, top = [], 27
    for a in acls:
        if kind == 'entries':
            ok = sum(fits) < 4
            top += _acl_len(a) if ok else 0
        else:
            ok = top + _acl_len(a) <= acap
            top += _acl_len(a)
        fits.append(ok)
    assert sum(fits) == (4 if kind == 'entries' else 2)
    assert 0 < sum(fits) < 10
    for p, g, ok in zip(pk, got, fits):
        if ok:
            _check_ok(g, _wire_acl(p))
        else:
            assert g['err'] == 'SYSTEM_ERROR' and g['_len'] == 16
            assert tree.acl_host(tree.find_host(p['path'])) is None
    ent, used, lost = srv.acl_stats()
    assert ent == 1 + sum(fits) and lost == 10 - sum(fits)
    assert used == min(top, acap)
    assert bool((big[acap:] == 0xAB).all().item())
    # the other nodes' bindings and the created nodes' data are untouched
    _check_ok(_get(srv, [_ga(99, '/bench/d000000/n000000001')], gpu)[0], OPEN)
    r = _serve(srv, [{'xid': 98, 'opcode': 'GET_DATA',
                      'path': pk[9]['path'], 'watch': False}], gpu)
    assert r[0]['err'] == 'OK' and r[0]['data'] == b'c'


def test_output_limits(gpu):
    """An output one byte short of the stream: error flag 2, total 0 and not
    a byte written; exactly enough room: the whole stream and nothing past
    it; an empty batch with and without the terminator; the terminator
    after one reply."""
    tree, srv = _setup(gpu)
    a = _acl_vectors(4)[3]
    r = _serve(srv, [_create(1, '/bench/d000000/x', a)], gpu)
    assert r[0]['err'] == 'OK'
    pk = [_ga(10 + k, '/bench/d000000/x' if k % 3 == 0 else
              '/bench/d000001/n%09d' % (100 + k)) for k in range(70)]
    s = _frames(pk)
    rx = _dev_bytes(s, gpu)
    _, total, err, ft = srv.serve_acl(rx, len(s))
    T = int(total.item())
    assert T > 70 * 115 and int(err.item()) == 0
    out = torch.full((T + 256,), 0xAB, dtype=torch.uint8, device=gpu)
    tot = torch.full((1,), -1, dtype=torch.int64, device=gpu)
    er = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    _lib.tree_acl_get(tree.tensors, tree.acl, rx, ft.off, ft.length, ft.count,
                      srv.cap_frames, srv.acl_ws, out, T - 1, srv.acl_rec_off,
                      tot, er)
    assert int(er.item()) == 2 and int(tot.item()) == 0
    assert bool((out == 0xAB).all().item())
    _lib.tree_acl_get(tree.tensors, tree.acl, rx, ft.off, ft.length, ft.count,
                      srv.cap_frames, srv.acl_ws, out, T, srv.acl_rec_off,
                      tot, er)
    assert int(er.item()) == 0 and int(tot.item()) == T
    assert bool((out[T:] == 0xAB).all().item())
    reps = _decode(out, tot, pk)
    for k, g in enumerate(reps):
        _check_ok(g, _wire_acl(_create(0, '/', a)) if k % 3 == 0 else OPEN)
    # empty batches and the terminator
    z = torch.zeros(64, dtype=torch.uint8, device=gpu)
    out, total, err, _ = srv.serve_acl(z, 0)
    assert int(total.item()) == 0 and int(err.item()) == 0
    out, total, err, _ = srv.serve_acl(z, 0, terminate=True)
    assert int(total.item()) == 0 and int(err.item()) == 0
    assert out[:4].cpu().tolist() == [255] * 4
    one = [_ga(1, '/bench/d000001')]
    s = _frames(one)
    out, total, err, _ = srv.serve_acl(_dev_bytes(s, gpu), len(s),
                                       terminate=True)
    T = int(total.item())
    assert T == 115 and out[T:T + 4].cpu().tolist() == [255] * 4
    _check_ok(_decode(out, total, one)[0], OPEN)


def test_replicas(gpu, monkeypatch):
    """Two trees with a fixed clock get the same create batches (the second
    after its table interned another ACL first, so its arena offsets
    differ): their GET_ACL reply streams for all created paths are
    byte-equal."""
    import time
    from zkmi.server import engine as S
    monkeypatch.setattr(S, 'time', types.SimpleNamespace(
        time=lambda: 1.7e9, perf_counter=time.perf_counter,
        sleep=time.sleep))
    acls = _acl_vectors(9)
    pk1 = [_create(100 + i, '/bench/d000000/r%03d' % i, acls[i % 7])
           for i in range(200)]
    pk2 = [_create(400 + i, '/bench/d000001/s%03d' % i, acls[(3 * i) % 9])
           for i in range(200)]
    streams, words = [], []
    for rep in range(2):
        tree, srv = _setup(gpu, ctime_ms=1600000000000)
        if rep == 1:
            # this replica's table has seen another ACL before (recorded
            # straight through the op for a node slot no create reaches), so
            # its arena offsets differ while its tree does not
            pre = _frames([_create(7, '/x', acls[8])])
            prx = _dev_bytes(pre, gpu)
            ft = srv.scanner.scan(prx, len(pre))
            cap = srv.cap_frames
            _lib.tree_acl_record(
                tree.acl, prx, ft.off, ft.length, ft.count, cap,
                torch.ones(cap, dtype=torch.int32, device=gpu),
                torch.zeros(cap, dtype=torch.int32, device=gpu),
                torch.full((cap,), tree.cap - 1, dtype=torch.int64,
                           device=gpu), srv._acl_workspace())
            assert srv.acl_stats() == (2, 27 + _acl_len(acls[8]), 0)
        for pk in (pk1, pk2):
            r = _serve(srv, pk, gpu)
            assert [x['err'] for x in r] == ['OK'] * 200
        gets = [_ga(1000 + i, p['path']) for i, p in enumerate(pk1 + pk2)]
        s = _frames(gets)
        out, total, err, _ = srv.serve_acl(_dev_bytes(s, gpu), len(s))
        assert int(err.item()) == 0
        streams.append(bytes(out[:int(total.item())].cpu().numpy()
                             .tobytes()))
        words.append(tree.acl[0][:tree.cap - 1].cpu().numpy().copy())
        for p, g in zip(pk1 + pk2, _decode(out, total, gets)):
            _check_ok(g, _wire_acl(p))
        assert srv.acl_stats()[::2] == (8 + rep, 0)   # 7 ACLs + the open one
    assert not np.array_equal(words[0], words[1])      # other offsets
    assert len(streams[0]) > 400 * 100
    assert streams[0] == streams[1]


def test_op_argument_checks(gpu):
    """tree_acl_get / tree_acl_record check every tensor before a pointer
    reaches a kernel."""
    tree, srv = _setup(gpu)
    s = _frames([_ga(1, '/bench/d000000')])
    rx = _dev_bytes(s, gpu)
    _, _, _, ft = srv.serve_acl(rx, len(s))
    out = torch.empty(1 << 12, dtype=torch.uint8, device=gpu)
    tot = torch.zeros(1, dtype=torch.int64, device=gpu)
    er = torch.zeros(1, dtype=torch.int32, device=gpu)

    def call(**kw):
        a = dict(acl=tree.acl, ws=srv.acl_ws, out=out,
                 rec_off=srv.acl_rec_off, total=tot, err=er, foff=ft.off,
                 out_cap=out.numel())
        a.update(kw)
        _lib.tree_acl_get(tree.tensors, a['acl'], rx, a['foff'], ft.length,
                          ft.count, srv.cap_frames, a['ws'], a['out'],
                          a['out_cap'], a['rec_off'], a['total'], a['err'])

    def acl_with(k, t):
        v = list(tree.acl)
        v[k] = t
        return v

    with pytest.raises(RuntimeError, match='node_acl must be Long'):
        call(acl=acl_with(0, tree.acl[0].to(torch.int32)))
    with pytest.raises(RuntimeError, match='frame_off must be Long'):
        call(foff=ft.off.to(torch.int32))
    with pytest.raises(RuntimeError, match='must be a GPU tensor'):
        call(out=out.cpu())
    with pytest.raises(RuntimeError, match='acl workspace has'):
        call(ws=srv.acl_ws[:srv.acl_ws.numel() - 16])
    with pytest.raises(RuntimeError, match='node_acl has'):
        call(acl=acl_with(0, tree.acl[0][:tree.cap - 1]))
    with pytest.raises(RuntimeError, match='contiguous'):
        call(acl=acl_with(0, torch.zeros(2 * tree.cap, dtype=torch.int64,
                                         device=gpu)[::2]))
    with pytest.raises(RuntimeError, match='out has'):
        call(out_cap=out.numel() + 1)
    with pytest.raises(RuntimeError, match='power of two'):
        call(acl=acl_with(2, tree.acl[2][:3]))
    with pytest.raises(RuntimeError, match='acl table needs 5'):
        call(acl=tree.acl[:4])
    r = srv.resp
    with pytest.raises(RuntimeError, match='r.node must be Long'):
        _lib.tree_acl_record(tree.acl, rx, ft.off, ft.length, ft.count,
                             srv.cap_frames, r.opcode, r.err,
                             r.node.to(torch.int32), srv.acl_ws)
    with pytest.raises(RuntimeError, match='r.err has'):
        _lib.tree_acl_record(tree.acl, rx, ft.off, ft.length, ft.count,
                             srv.cap_frames, r.opcode, r.err[:5], r.node,
                             srv.acl_ws)
    assert _lib.tree_acl_workspace(srv.cap_frames) == srv.acl_ws.numel()
    call()                                        # and the good call runs
    assert int(er.item()) == 0 and int(tot.item()) == 115


def test_no_acl_table(gpu):
    """A tree without an ACL table: serve_acl raises, and serve() answers a
    create batch as a tree with one does."""
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    a, b = _acl_vectors(2)
    pk = [_create(10 + i, '/bench/d000000/p%02d' % i, a if i % 2 else b)
          for i in range(40)]
    pk += [_create(91, '/nope/x', a)]
    again = [_create(90, '/bench/d000000/p00', a)]     # (its own batch)
    got = []
    for cap in (0, 64):
        tree = GpuTree(300, 16, fanout=100, device=gpu, acl_cap=cap)
        assert (tree.acl is None) == (cap == 0)
        srv = GpuServer(tree, 256, 1 << 18, window=512)
        reps = _serve(srv, pk, gpu) + _serve(srv, again, gpu)
        got.append([(r['xid'], r['err'], r.get('path')) for r in reps])
        if cap == 0:
            s = _frames([_ga(1, '/bench')])
            with pytest.raises(ValueError, match='ACL table'):
                srv.serve_acl(_dev_bytes(s, gpu), len(s))
            assert not hasattr(srv, 'acl_ws')
    assert got[0] == got[1]
    assert [e for _, e, _ in got[0]] == ['OK'] * 40 + ['NO_NODE',
                                                      'NODE_EXISTS']


def test_acl_pipeline_capture_replay(gpu):
    """AclPipeline on a 20k-node tree, batch 512, after 200 of the nodes were
    re-created with a second ACL: an eager step, then the captured step
    replayed three times; the device check stays clean and the first
    replay's replies decode to the same (xid, acl) list as the eager
    step's."""
    from zkmi.bench.synthetic import AclPipeline, MIX_ACLS
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(20_000, 16, fanout=100, device=gpu, acl_cap=16)
    srv = GpuServer(tree, 256, 1 << 18, window=512)
    second = MIX_ACLS[1]
    paths = ['/bench/d%06d/n%09d' % (i // 100, i)
             for i in range(0, 20_000, 100)]
    assert len(paths) == 200
    r = _serve(srv, [{'xid': i, 'opcode': 'DELETE', 'path': p, 'version': -1}
                     for i, p in enumerate(paths)], gpu)
    assert [x['err'] for x in r] == ['OK'] * 200
    r = _serve(srv, [_create(500 + i, p, second)
                     for i, p in enumerate(paths)], gpu)
    assert [x['err'] for x in r] == ['OK'] * 200
    # seed chosen so that the draw holds re-created nodes
    pipe = AclPipeline(tree, 512, seed=1)
    want = _wire_acl(_create(0, '/', second))

    def acls():
        rep, rx, ft, total = pipe.last
        raw = bytes(rx[:int(total.item())].cpu().numpy().tobytes())
        frames, used, bad = jute.scan_frames(raw)
        assert bad < 0 and used == len(raw) and len(frames) == 512
        xmap = {k: 'GET_ACL' for k in range(512)}
        out = []
        for o, ln in frames:
            g = jute.decode_response(raw[o:o + ln], xmap)
            assert g['err'] == 'OK' and g['acl'] in (OPEN, want)
            out.append((g['xid'], repr(g['acl'])))
        return out

    acc = pipe.step()
    torch.cuda.synchronize()
    assert int(acc.item()) == 512 and int(pipe.bad.item()) == 0, \
        pipe.diagnose()
    eager = acls()
    assert [x for x, _ in eager] == list(range(512))
    assert int(pipe.want_cnt.max().item()) == 2       # both ACLs are asked
    assert int(pipe.want_cnt.min().item()) == 1
    acc = torch.zeros(1, dtype=torch.int64, device=gpu)
    g = pipe.capture(acc)
    g.replay()
    torch.cuda.synchronize()
    assert acls() == eager
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert int(acc.item()) == 3 * 512 and int(pipe.bad.item()) == 0, \
        pipe.diagnose()
    n = int(pipe.nrows.item())
    assert n == pipe.want_entries == int(pipe.want_cnt.sum().item())
