"""The GPU tree's image (csrc/kernels/tree_snap.hip, zk_snap.h):
GpuTree.snapshot after a churned history, GpuTree.load into trees of other
capacities, the ACL table through both, a host-made image served by the GPU
server, the reject side on the mutation corpus of tests/image_corpus.py, the
fixed-buffer snapshot and the ops' argument checks.  All comparisons are
exact."""

import pytest
import torch

import image_corpus as C
from treemodel import (TreeModel, _Loop, create, delete, dev_bytes, exists,
                       get, hash_twin, set_data)
from zkmi import jute
from zkmi.ops import _lib
from zkmi.server.fakezk import ZKDatabase
from zkmi.utils import treeimage as TI

pytestmark = pytest.mark.gpu

W, S, E, LONG = '/bench/w', '/bench/s', '/bench/e', '/bench/long'
NW = 560


def _name(k):
    """Name k under W: path lengths 15..80, every residue mod 16."""
    total = 15 + k % 66
    return '%s/%04d%s' % (W, k, 'x' * (total - len(W) - 5))


def _dl(k):
    """Data length of name k: 0..2048, every residue mod 16, both sides of
    256, the ends and the neighbours of 256 among the first few."""
    return (0, 255, 256, 257, 2048, 1, 15, 16, 17)[k] if k < 9 else \
        (k * 37) % 2049


def _bytes(k, n):
    return bytes((k * 7 + j * 13) & 0xff for j in range(n))


def _stream(pk):
    return b''.join(jute.frame(jute.encode_request(p)) for p in pk)


def _raw(serve, pk, dev, x0=1 << 20):
    """The reply stream's bytes for the requests ``pk`` (xids from x0)."""
    for j, p in enumerate(pk):
        p['xid'] = x0 + j
    s = _stream(pk)
    out, total, err, _ = serve(dev_bytes(s, dev), len(s))
    assert int(err.item()) == 0
    return bytes(out[:int(total.item())].cpu().numpy().tobytes())


def _raw_chunks(srv, serve, pk, dev):
    return b''.join(_raw(serve, pk[o:o + srv.cap_frames], dev)
                    for o in range(0, len(pk), srv.cap_frames))


def _replies(raw, pk):
    frames, used, bad = jute.scan_frames(raw)
    assert bad < 0 and used == len(raw) and len(frames) == len(pk)
    return [jute.decode_response(raw[o:o + ln], {p['xid']: p['opcode']})
            for (o, ln), p in zip(frames, pk)]


def _server(tree, frames=1024):
    from zkmi.server.engine import GpuServer
    return GpuServer(tree, frames, 4 << 20)


@pytest.fixture(scope='module')
def churned(gpu):
    """The source tree after its history, its image, and what the source
    answers for every path that ever lived (taken before anything else
    runs)."""
    from zkmi.server.tree import GpuTree
    tree = GpuTree(10, 2048, fanout=10, device=gpu, spare=6.0)
    assert 1100 <= tree.cap <= 1110
    m = TreeModel(tree, _server(tree), gpu)
    sid = m.session()
    names = [_name(k) for k in range(NW)]
    assert {len(p) % 16 for p in names} == set(range(16))
    assert {len(p) for p in names} == set(range(15, 81))
    assert {_dl(k) % 16 for k in range(NW)} == set(range(16))
    a = LONG + '/' + 'T' * 44
    twin = hash_twin(a, 5)
    assert len(a) == 56 and twin != a
    m.serve([create(p) for p in (W, S, E, LONG)], audit=False)
    for lo in range(0, NW, 140):
        m.serve([create(names[k], _bytes(k, _dl(k)))
                 for k in range(lo, lo + 140)], audit=False)
    # (the twins in two batches: two creates of one hash key in one batch
    # race for the index entry)
    m.serve([create(a, b'one')] +
            [create('%s/e%d' % (E, j), _bytes(j, 40 * j), ['EPHEMERAL'])
             for j in range(5)] +
            [create(S + '/q-', _bytes(j, j), ['SEQUENTIAL'])
             for j in range(6)], sid=sid, audit=False)
    # holes: every third name goes; half of those come back on recycled
    # nodes (longer and shorter data than the node had), the rest never do
    m.serve([delete(names[k]) for k in range(0, NW, 3)] +
            [create(twin, b'two')], audit=False)
    m.serve([create(names[k], _bytes(k + 1, _dl((k * 5 + 3) % NW)))
             for k in range(0, NW, 6)] +
            [create('%s/r%04d%s' % (W, j, 'y' * (j % 50)), _bytes(j, 3 * j))
             for j in range(40)], audit=False)
    # version CAS: right, wrong and unconditional
    m.serve([set_data(names[k], _bytes(k, k % 129),
                      0 if k % 10 == 1 else (3 if k % 10 == 6 else -1))
             for k in range(1, NW, 5) if k % 3], audit=False)
    m.serve([set_data(names[k], _bytes(k + 2, (k * 3) % 129), 1)
             for k in range(1, NW, 10) if k % 3], audit=False)
    m.audit()
    # what the old slot capacity refuses (and a loaded tree's larger one takes)
    small = names[8]
    assert _dl(8) == 17
    _, want = m.serve([set_data(small, b'z' * 1000)], audit=False)
    assert want[0][1] == 'BAD_ARGUMENTS'
    live = sorted(m.live())
    dead = sorted(m.dead)
    assert len(live) > 500 and len(dead) > 90
    assert names[3] in dead and names[6] in live
    img = tree.snapshot()
    torch.cuda.synchronize()
    # (taken now: every served batch, reads too, moves the zxid counter on,
    # and a reply's header carries it)
    zxid = int(tree.counters[_lib.TC_ZXID].item())
    digest = tree.digest()
    pk = [get(p) for p in live] + [exists(p) for p in dead]
    return {'tree': tree, 'model': m, 'srv': m.srv,
            'node_of': dict(m.node_of), 'sid': sid, 'names': names,
            'small': small, 'live': live, 'dead': dead, 'img': img,
            'bytes': bytes(img.cpu().numpy().tobytes()),
            'gets': _raw_chunks(m.srv, m.srv.serve, pk, gpu),
            'digest': digest, 'zxid': zxid}


# ---- 1. round trip after churn ----------------------------------------------

def test_snapshot_after_churn(churned, gpu):
    c = churned
    hd, recs = TI.unpack(c['bytes'])
    assert TI.check(c['bytes']) == (TI.OK, -1)
    assert sorted(r['path'] for r in recs) == c['live']
    assert hd['n'] == len(c['live']) > 2 * 256
    # holes and recycled nodes: record index != node index
    order = [c['node_of'][r['path']] for r in recs]
    assert order == sorted(order) and order != list(range(len(order)))
    pk = [get(r['path']) for r in recs]
    raw = _raw_chunks(c['model'].srv, c['srv'].serve, pk, gpu)
    open_acl = TI.unpack(TI.pack([C.rec('/o')], 0))[1][0]['acl']
    for r, rep in zip(recs, _replies(raw, pk)):
        assert rep['err'] == 'OK', r['path']
        assert bytes(rep['data'] or b'') == r['data'], r['path']
        # all 11 fields, ctime and mtime among them
        assert rep['stat'].as_tuple() == r['stat'].as_tuple(), r['path']
        assert r['acl'] == open_acl
    assert hd['zxid'] == c['zxid']
    assert hd['digest'] == TI.digest(recs) == c['digest'][0]
    assert hd['max_data'] == max(len(r['data']) for r in recs) == 2048
    assert hd['path16'] == sum((len(r['path']) + 15) & ~15 for r in recs)
    # the source's znodes did not move: a second snapshot is the same image
    # but for the zxid counter, which the reads above moved on
    again = c['tree'].snapshot()
    assert torch.equal(again[:32], c['img'][:32])
    assert torch.equal(again[40:], c['img'][40:])


# ---- 2. load and carry on ---------------------------------------------------

def test_load_and_carry_on(churned, gpu):
    from zkmi.server.tree import GpuTree
    c = churned
    m = c['model']
    t = GpuTree.load(c['img'], device=gpu, spare=0.5, hash_factor=4,
                     data_cap=4096)
    torch.cuda.synchronize()
    n = len(c['live'])
    assert t.cap == int(n * 1.5) + 1024 and t.cap != c['tree'].cap
    assert t.hcap == 8192 and t.leaf0 is None and t.n_leaves is None
    d = t.digest()
    assert d[:2] == c['digest'][:2]
    assert d[2] == n and d[3] == 0          # entries in use, tombstones
    cnt = t.counters.cpu().tolist()
    assert cnt[_lib.TC_NODES] == n and cnt[_lib.TC_ZXID] == c['zxid']
    assert cnt[_lib.TC_FREE_HEAD] == cnt[_lib.TC_FREE_TAIL] == \
        cnt[_lib.TC_FREE_PUB] == 0 and cnt[_lib.TC_DIRTY] == 0
    assert cnt[_lib.TC_PATH_TOP] == TI.header(c['bytes'])['path16']
    # compaction: the arenas hold the live znodes and nothing else
    src = c['tree'].counters.cpu().tolist()
    assert cnt[_lib.TC_PATH_TOP] < src[_lib.TC_PATH_TOP]
    # snapshot(load(img)) is img
    assert torch.equal(t.snapshot(), c['img'])
    # the same replies, byte for byte
    srv = _server(t)
    pk = [get(p) for p in c['live']] + [exists(p) for p in c['dead']]
    assert _raw_chunks(srv, srv.serve, pk, gpu) == c['gets']
    # the model over the loaded tree: everything the audit reads
    m.tree, m.srv = t, srv
    m.touched = {W, S, E, LONG, '/bench', '/bench/d000000'}
    m.audit()
    assert int(m.slot_cap.min()) == 4096
    # the history goes on
    names, sid = c['names'], c['sid']
    base = m.counter(_lib.TC_ZXID)
    assert base > c['zxid']
    reps, _ = m.serve([create(S + '/q-', b'next', ['SEQUENTIAL']),
                       create(W + '/newkid', b'k' * 300),
                       delete(names[7]),
                       set_data(c['small'], b'z' * 1000),
                       create(E + '/late', b'', ['EPHEMERAL'])], sid=sid)
    assert reps[0]['path'] == S + '/q-0000000006'
    assert reps[0]['zxid'] == base + 1
    m.serve([create(names[7], b'back' * 100), get(c['small']),
             create(names[3], _bytes(3, 700))])
    eph = sorted(p for p in m.live() if p.startswith(E + '/'))
    assert len(eph) == 6
    assert m.expire(sid) == 6
    assert not [p for p in m.live() if p.startswith(E + '/')]
    # and its image loads again, into the smallest tree that takes it
    img2 = t.snapshot()
    h2 = TI.header(bytes(img2[:64].cpu().numpy().tobytes()))
    t2 = GpuTree.load(img2, device=gpu, nodes=h2['n'], data_cap=0,
                      path_bytes=h2['path16'])
    assert t2.digest()[:2] == t.digest()[:2]
    assert torch.equal(t2.snapshot(), img2)


# ---- 3. ACLs ----------------------------------------------------------------

def _acl_create(path, acl):
    return {'opcode': 'CREATE', 'path': path, 'data': path.encode(),
            'acl': acl, 'flags': []}


def test_acls_through_image(gpu):
    from zkmi.server.tree import GpuTree
    src = GpuTree(10, 16, fanout=10, device=gpu, spare=0.0, acl_cap=3)
    srv = _server(src)
    vec = [C.DIGEST_ACL,
           [{'perms': ['READ'], 'id': {'scheme': 'world', 'id': ''}}],
           [{'perms': ['ADMIN'], 'id': {'scheme': 'ip', 'id': '::1'}},
            {'perms': ['READ'], 'id': {'scheme': 'sasl', 'id': 'bob'}}],
           [{'perms': ['WRITE'], 'id': {'scheme': 'x509', 'id': 'CN=a'}}]]
    pk = [_acl_create('/bench/a%d' % j, vec[j % 3]) for j in range(9)] + \
        [_acl_create('/bench/o%d' % j, jute.DEFAULT_ACL) for j in range(3)]
    reps = _replies(_raw(srv.serve, pk, gpu), pk)
    assert {r['err'] for r in reps} == {'OK'}
    # a fourth vector on a table for three: the binding is lost
    pk2 = [_acl_create('/bench/lost', vec[3])]
    assert _replies(_raw(srv.serve, pk2, gpu), pk2)[0]['err'] == 'OK'
    assert srv.acl_stats()[0] == 4 and srv.acl_stats()[2] == 1
    paths = ['/bench', '/bench/d000000', '/bench/d000000/n000000003',
             '/bench/lost', '/bench/none'] + [p['path'] for p in pk]
    ga = [{'opcode': 'GET_ACL', 'path': p} for p in paths]
    gets = [get(p) for p in paths]
    img = src.snapshot()
    # (a reply's header carries the zxid counter, which every served batch
    # moves on: the loaded trees below are asked in this order too)
    want_get = _raw(srv.serve, gets, gpu)
    want_acl = _raw(srv.serve_acl, ga, gpu)
    reps = _replies(want_acl, ga)
    assert reps[3]['err'] == 'SYSTEM_ERROR' and reps[4]['err'] == 'NO_NODE'
    assert reps[5]['acl'] == jute.decode_request(jute.encode_request(
        dict(pk[0], xid=0)))['acl']
    recs = TI.unpack(bytes(img.cpu().numpy().tobytes()))[1]
    assert [r['path'] for r in recs if r['acl'] is None] == ['/bench/lost']
    # with a table
    t = GpuTree.load(img, device=gpu, acl_cap=8)
    ts = _server(t)
    assert torch.equal(t.snapshot(), img)
    assert _raw(ts.serve, gets, gpu) == want_get
    assert _raw(ts.serve_acl, ga, gpu) == want_acl
    ent, used, lost = ts.acl_stats()
    assert (ent, lost) == (4, 1)
    assert used == sum(len(_acl_wire(v)) for v in vec[:3]) + 27
    # a CREATE after the load: a loaded vector adds no entry, a new one does
    more = [_acl_create('/bench/again', vec[1])]
    assert _replies(_raw(ts.serve, more, gpu), more)[0]['err'] == 'OK'
    assert ts.acl_stats()[0] == 4
    more = [_acl_create('/bench/fresh', vec[3])]
    assert _replies(_raw(ts.serve, more, gpu), more)[0]['err'] == 'OK'
    assert ts.acl_stats() == (5, used + len(_acl_wire(vec[3])), 1)
    ga2 = [{'opcode': 'GET_ACL', 'path': p}
           for p in ('/bench/again', '/bench/fresh', '/bench/a1')]
    r2 = _replies(_raw(ts.serve_acl, ga2, gpu), ga2)
    assert r2[0]['acl'] == r2[2]['acl'] != r2[1]['acl']
    assert [r['err'] for r in r2] == ['OK'] * 3
    # without a table: the vectors are dropped, the data reads are the same
    t0 = GpuTree.load(img, device=gpu)
    assert t0.acl is None
    assert _raw(_server(t0).serve, gets, gpu) == want_get
    assert t0.digest()[:2] == src.digest()[:2]


def _acl_wire(acl):
    w = jute.JuteWriter()
    w.write_acl(acl)
    return w.getvalue()


# ---- 4. a host-made image ---------------------------------------------------

def _host_db():
    db = ZKDatabase(_Loop())
    world = [db._world()]
    sid = db.new_session(30000).sid
    for top in ('/app', '/cfg', '/x'):
        db.create(top, top.encode(), world, [], None)
    for k in range(20):
        db.create('/app/n%02d' % k, _bytes(k, k * 23), world, [], None)
    db.create('/app/n03/deep', b'', world, [], None)
    db.create('/app/n03/deep/er', _bytes(1, 300), world, [], None)
    db.create('/app/n03/deep/est', b'4', world, [], None)
    db.create('/cfg/eph', b'e', world, ['EPHEMERAL'], sid)
    for _ in range(3):
        db.create('/cfg/seq-', b's', world, ['SEQUENTIAL'], None)
    db.set_data('/app/n05', b'changed', 0)
    for k in (1, 4, 7):
        db.delete('/app/n%02d' % k, -1, None)
    return db


def test_host_made_image(gpu):
    from zkmi.server.tree import GpuTree
    db = _host_db()
    recs = [{'path': p, 'stat': n.stat, 'data': bytes(n.data or b''),
             'acl': n.acl} for p, n in sorted(db.nodes.items()) if p != '/']
    assert max(r['path'].count('/') for r in recs) == 4
    t = GpuTree.load(TI.pack(recs, db.zxid), device=gpu)
    assert int(t.counters[_lib.TC_ZXID].item()) == db.zxid
    srv = _server(t)
    paths = [r['path'] for r in recs] + ['/app/n01', '/nope', '/app/n03/x']
    for op, serve in (('GET_DATA', srv.serve), ('EXISTS', srv.serve),
                      ('GET_CHILDREN2', srv.serve_list)):
        pk = [{'opcode': op, 'path': p, 'watch': False} for p in paths]
        for rep, p in zip(_replies(_raw(serve, pk, gpu), pk), pk):
            want = db.handle(dict(p), None)
            assert rep['err'] == want['err'], (op, p['path'])
            if want['err'] != 'OK':
                continue
            assert rep['stat'].as_tuple() == want['stat'].as_tuple()
            if op == 'GET_DATA':
                assert bytes(rep['data'] or b'') == bytes(want['data'] or b'')
            if op == 'GET_CHILDREN2':
                assert sorted(rep['children']) == want['children']
    assert t.digest()[0] == TI.digest(recs)


@pytest.mark.parametrize('n', [0, 1])
def test_tiny_images(gpu, n):
    from zkmi.server.tree import GpuTree
    recs = [C.rec('/only', b'1', z=4)][:n]
    t = GpuTree.load(TI.pack(recs, 9), device=gpu)
    assert t.digest()[:2] == (TI.digest(recs), n)
    srv = _server(t)
    pk = [get('/only'), get('/other'), create('/made', b'm')]
    reps = _replies(_raw(srv.serve, pk, gpu), pk)
    assert [r['err'] for r in reps] == [('OK' if n else 'NO_NODE'),
                                        'NO_NODE', 'OK']
    assert reps[2]['zxid'] == 9 + 3
    if n:
        assert reps[0]['data'] == b'1' and reps[0]['stat'].czxid == 4
    assert TI.unpack(bytes(t.snapshot().cpu().numpy().tobytes()))[0]['n'] == \
        n + 1


# ---- 5. the reject side -----------------------------------------------------

def _load_outcome(img, gpu, **kw):
    from zkmi.server.tree import GpuTree
    try:
        GpuTree.load(img, device=gpu, **kw)
        out = (TI.OK, -1)
    except TI.TreeImageError as e:
        out = (e.code, e.index)
    torch.cuda.synchronize()              # no HIP error behind a refusal
    return out


def test_loader_refuses_what_the_host_check_refuses(gpu):
    wrong = []
    for name, img, want in C.corpus():
        got = _load_outcome(img, gpu)
        chk = TI.check(img)
        assert chk[0] == want[0]
        ok = got == chk or (chk[0] == TI.DUP_PATH and got[0] == TI.DUP_PATH
                            and got[1] in (1, 5))
        if not ok:
            wrong.append((name, got, chk))
    assert not wrong, wrong
    # the same images as device tensors and CPU tensors
    img = C.base_image()
    cpu = torch.frombuffer(bytearray(img), dtype=torch.uint8)
    assert _load_outcome(cpu, gpu) == (TI.OK, -1)
    assert _load_outcome(cpu.to(gpu), gpu) == (TI.OK, -1)


def test_colliding_keys_in_one_wave(gpu):
    """Three distinct paths of one 64-bit hash key at adjacent record
    indices: one wave inserts them, the second and third behind the first's
    unpublished entry (the index build's second launch).  They are no
    duplicates: the image loads and every one answers its own data."""
    from zkmi.server.tree import GpuTree
    twins = C.twin_paths()
    assert len({_lib.acl_hash(p.encode()) for p in twins}) == 1
    img = dict((c[0], c[1]) for c in C.corpus())['twins3']
    recs = TI.unpack(img)[1]
    assert [r['path'] for r in recs[-3:]] == list(twins)
    # (an ACL table: the base records hold a lost binding, which only a
    # tree with a table writes back as it was)
    t = GpuTree.load(img, device=gpu, acl_cap=4)
    assert t.digest()[:4] == (TI.digest(recs), len(recs), len(recs), 0)
    assert bytes(t.snapshot().cpu().numpy().tobytes()) == img
    srv = _server(t)
    pk = [get(p) for p in twins]
    reps = _replies(_raw(srv.serve, pk, gpu), pk)
    assert [r['err'] for r in reps] == ['OK'] * 3
    assert [r['data'] for r in reps] == [p[-9:].encode() for p in twins]
    # a true duplicate among them is still found
    dup = TI.pack(recs + [C.rec(twins[1], b'again', 30)], 77)
    assert TI.check(dup) == (TI.DUP_PATH, len(recs))
    got = _load_outcome(dup, gpu)
    assert got[0] == TI.DUP_PATH and got[1] in (len(recs) - 2, len(recs))


def test_lying_size_hints_stay_bounded(gpu):
    """The loader sizes the tree from the header before the device has
    checked anything: hints far past what the image can hold must not size
    the tree past a few times the image."""
    from zkmi.server.tree import GpuTree
    img = dict((c[0], c[1]) for c in C.corpus())['hint-huge']
    t = GpuTree.load(img, device=gpu)
    assert t.slab_cap < (1 << 22) and t.path_cap < (1 << 22)
    assert t.digest()[:2] == (TI.digest(C.base_records()), 5)


def test_no_room(gpu):
    img = C.base_image()
    recs = C.base_records()
    n = len(recs)
    p16 = TI.header(img)['path16']
    slab = sum(_lib.SLOT_DATA + ((max(128, len(r['data'])) + 15) & ~15) + 4
               for r in recs)
    fit = dict(nodes=n, path_bytes=p16, slab_bytes=slab)
    assert _load_outcome(img, gpu, **fit) == (TI.OK, -1)
    for k, v in (('nodes', n - 1), ('path_bytes', p16 - 16),
                 ('slab_bytes', slab - 16)):
        assert _load_outcome(img, gpu, **dict(fit, **{k: v})) == \
            (TI.NO_ROOM, -1), k


# ---- 6. a fixed buffer ------------------------------------------------------

def test_snapshot_into_fixed_buffer(churned, gpu):
    tree = churned['tree']
    img = tree.snapshot()                 # the allocating call
    L = img.numel()
    assert L == churned['img'].numel()
    buf = torch.full((L + 64,), 0xAB, dtype=torch.uint8, device=gpu)
    out, total, status = tree.snapshot(out=buf[:L - 1])
    assert status.cpu().tolist() == [TI.NO_ROOM, -1]
    assert total.cpu().tolist() == [L, len(churned['live'])]
    assert bool((buf == 0xAB).all())
    out, total, status = tree.snapshot(out=buf[:L])
    assert status.cpu().tolist() == [TI.OK, -1]
    assert torch.equal(buf[:L], img)
    assert bool((buf[L:] == 0xAB).all())
    big = torch.zeros(L + 4096, dtype=torch.uint8, device=gpu)
    out, total, status = tree.snapshot(out=big)
    assert torch.equal(big[:int(total[0].item())], img)


# ---- 7. the ops' argument checks --------------------------------------------

def test_op_argument_checks(gpu):
    from zkmi.server.tree import GpuTree
    t = GpuTree(10, 16, fanout=10, device=gpu, spare=0.0)
    ops = _lib.lib()
    U8, I64 = torch.uint8, torch.int64
    ws = torch.empty(ops.tree_snap_workspace(t.cap), dtype=U8, device=gpu)
    total = torch.zeros(2, dtype=I64, device=gpu)
    status = torch.zeros(2, dtype=I64, device=gpu)
    out = torch.empty(1 << 16, dtype=U8, device=gpu)
    ops.tree_snap_size(t.tensors, [], ws, total)
    with pytest.raises(RuntimeError, match='image workspace has'):
        ops.tree_snap_size(t.tensors, [], ws[:-16], total)
    with pytest.raises(RuntimeError, match='image workspace must be Byte'):
        ops.tree_snap_size(t.tensors, [], ws.view(I64), total)
    with pytest.raises(RuntimeError, match='total must be Long'):
        ops.tree_snap_size(t.tensors, [], ws, total.int())
    with pytest.raises(RuntimeError, match='must be a GPU tensor'):
        ops.tree_snap_size(t.tensors, [], ws, total.cpu())
    with pytest.raises(RuntimeError, match='acl table needs 5'):
        ops.tree_snap_size(t.tensors, [ws], ws, total)
    with pytest.raises(RuntimeError, match='out has'):
        ops.tree_snap_write(t.tensors, [], ws, out, out.numel() + 1, status)
    with pytest.raises(RuntimeError, match='16-byte aligned'):
        ops.tree_snap_write(t.tensors, [], ws, out[8:], 4096, status)
    with pytest.raises(RuntimeError, match='must be a GPU tensor'):
        ops.tree_snap_write(t.tensors, [], ws, out.cpu(), 4096, status)
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.tree_snap_write(t.tensors, [], ws, out[::2], 4096, status)
    img = dev_bytes(C.base_image(), gpu)
    n = len(C.base_records())
    lws = torch.empty(ops.tree_load_workspace(n), dtype=U8, device=gpu)
    with pytest.raises(RuntimeError, match='does not fit the image'):
        ops.tree_load(t.tensors, [], img, 64 + 8 * n, n, 128, lws, status)
    with pytest.raises(RuntimeError, match='image has'):
        ops.tree_load(t.tensors, [], img, img.numel() + 1, n, 128, lws,
                      status)
    with pytest.raises(RuntimeError, match='image workspace has'):
        ops.tree_load(t.tensors, [], img, img.numel(), n, 128, lws[:-16],
                      status)
    with pytest.raises(RuntimeError, match='image must be Byte'):
        ops.tree_load(t.tensors, [], img.view(torch.int8), img.numel(), n,
                      128, lws, status)
    with pytest.raises(RuntimeError, match='must be a GPU tensor'):
        ops.tree_load(t.tensors, [], img.cpu(), img.numel(), n, 128, lws,
                      status)
    with pytest.raises(RuntimeError, match='status has'):
        ops.tree_load(t.tensors, [], img, img.numel(), n, 128, lws,
                      status[:1])
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        GpuTree.load(torch.zeros(8, dtype=I64), device=gpu)
