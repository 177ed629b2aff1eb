"""The GPU server's list path (csrc/kernels/tree_list.hip,
GpuServer.serve_list): GET_CHILDREN / GET_CHILDREN2 batches answered from
the HBM tree by a join of the requested parents against a sweep of the node
table.  Replies are decoded with the jute oracle and compared, as sorted
lists, with a path model the test keeps.
Reference: lib/zk-buffer.js:64-70 (request), :300-306 (reply);
lib/client.js list()."""

import numpy as np
import pytest
import torch

from zkmi import jute
from zkmi.ops import _lib

pytestmark = pytest.mark.gpu


def _dev_bytes(b, dev):
    a = np.frombuffer(bytes(b) if b else b'\0', np.uint8).copy()
    return torch.from_numpy(a).to(dev)


def _ls(x, path, op=12, watch=False):
    return {'xid': x, 'opcode': 'GET_CHILDREN2' if op == 12
            else 'GET_CHILDREN', 'path': path, 'watch': watch}


def _frames(pk):
    """The request stream of ``pk``; a packet with 'cut' loses that many
    bytes of its body (the frame length says so: a truncated request)."""
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


def _list(srv, pk, gpu, **kw):
    s = _frames(pk)
    out, total, err, _ = srv.serve_list(_dev_bytes(s, gpu), len(s), **kw)
    assert int(err.item()) == 0
    reps = _decode(out, total, pk)
    assert [r['xid'] for r in reps] == [p['xid'] for p in pk]
    return reps


def _serve(srv, pk, gpu, session=0):
    s = _frames(pk)
    out, total, _, _ = srv.serve(_dev_bytes(s, gpu), len(s), session=session)
    return _decode(out, total, pk)


def _path_model(tree):
    """{parent path: sorted child names} from the tree's path table read
    back to the host (node_path_off / node_path_len of the live nodes) —
    grouped by the paths' text, not by the parent links the kernels use."""
    n = int(tree.counters[_lib.TC_NODES].item())
    po = tree.node_path_off[:n].cpu().numpy()
    pl = tree.node_path_len[:n].cpu().numpy()
    live = tree.node_parent[:n].cpu().numpy() != -2
    arena = tree.path_arena.cpu().numpy().tobytes()
    model = {}
    for v in np.nonzero(live)[0]:
        p = arena[po[v]:po[v] + pl[v]].decode()
        model.setdefault(p, [])
        d, _, name = p.rpartition('/')
        if d:
            model.setdefault(d, []).append(name)
    return {k: sorted(v) for k, v in model.items()}


def _check_ok(rep, names):
    assert rep['err'] == 'OK', rep
    assert sorted(rep['children']) == names
    body = 16 + 4 + sum(4 + len(c.encode()) for c in rep['children'])
    if rep['opcode'] == 'GET_CHILDREN2':
        assert rep['stat'].numChildren == len(names)
        body += 68
    assert rep['_len'] == body            # (GET_CHILDREN carries no Stat)


@pytest.mark.parametrize('fanout', [1, 10, 63, 64, 65, 300])
def test_static_tree_lists(gpu, fanout):
    """Directories of 1 child, several directories per wave (10), the wave
    edge (63 / 64 / 65) and one spanning two 256-thread blocks (300), the
    last directory partly filled; with a leaf (empty vector), /bench (node
    0), a missing path and / (NO_NODE: the tree has no root node), a
    GET_DATA frame (UNIMPLEMENTED) and a truncated frame (BAD_ARGUMENTS) in
    the same batch.  Replies come in request order with the request xids."""
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    n = max(5 * fanout + 3, 40)
    tree = GpuTree(n, 16, fanout=fanout, device=gpu)
    srv = GpuServer(tree, 256, 1 << 20, window=256)
    ndirs = (n + fanout - 1) // fanout
    dirs = ['/bench/d%06d' % d for d in range(ndirs)]
    want = {d: [] for d in dirs}
    for i in range(n):
        want[dirs[i // fanout]].append('n%09d' % i)
    want['/bench'] = ['d%06d' % d for d in range(ndirs)]
    leaf = '/bench/d000000/n000000000'
    pk = [_ls(100 + k, d, op=12 if k % 2 else 8) for k, d in enumerate(dirs)]
    x = 100 + ndirs
    pk += [_ls(x, leaf), _ls(x + 1, '/bench'), _ls(x + 2, '/bench/nope', 8),
           {'xid': x + 3, 'opcode': 'GET_DATA', 'path': dirs[0],
            'watch': False},
           dict(_ls(x + 4, dirs[0]), cut=1), _ls(x + 5, '/'),
           _ls(x + 6, '/bench', 8)]
    reps = _list(srv, pk, gpu)
    assert len(reps) == len(pk)
    for k, d in enumerate(dirs):
        _check_ok(reps[k], want[d])
    tail = reps[ndirs:]
    _check_ok(tail[0], [])
    _check_ok(tail[1], want['/bench'])
    assert [r['err'] for r in tail[2:6]] == [
        'NO_NODE', 'UNIMPLEMENTED', 'BAD_ARGUMENTS', 'NO_NODE']
    assert all(r['_len'] == 16 for r in tail[2:6])
    _check_ok(tail[6], want['/bench'])
    # the Stat of a GET_CHILDREN2 is the one EXISTS returns from serve()
    asked = [p for p in pk if p['opcode'] == 'GET_CHILDREN2' and
             not p.get('cut') and p['path'] != '/']
    ex = _serve(srv, [{'xid': p['xid'], 'opcode': 'EXISTS',
                       'path': p['path'], 'watch': False} for p in asked],
                gpu)
    by_xid = {r['xid']: r for r in reps}
    for e in ex:
        assert e['stat'].as_tuple() == by_xid[e['xid']]['stat'].as_tuple()
    assert all(r['zxid'] == ex[0]['zxid'] for r in reps)


def test_unaligned_names(gpu):
    """Names of 10..47 bytes (name_pad): every child of 20 directories byte
    for byte, and the reply stream frames exactly (checked in _decode)."""
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(20 * 37, 16, fanout=37, device=gpu, name_pad=(0, 37))
    srv = GpuServer(tree, 64, 1 << 20, window=256)
    model = _path_model(tree)
    dirs = ['/bench/d%06d' % d for d in range(20)]
    lens = {len(c) for d in dirs for c in model[d]}
    assert len(lens) > 20                      # really a mix of lengths
    reps = _list(srv, [_ls(k, d, op=8 if k % 3 else 12)
                       for k, d in enumerate(dirs)], gpu)
    for d, r in zip(dirs, reps):
        assert len(model[d]) == 37
        _check_ok(r, model[d])


def test_duplicate_parents(gpu):
    """One parent asked five times in a batch (opcodes 8 and 12 in turn)
    between other parents: every copy is complete, the per-node claim words
    are idle again afterwards, and the next batch is right."""
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(2000, 16, fanout=100, device=gpu)
    srv = GpuServer(tree, 64, 1 << 20, window=256)
    model = _path_model(tree)
    d = ['/bench/d%06d' % k for k in range(20)]
    order = [d[3], d[0], d[3], d[1], d[1], d[3], d[2], d[3], d[19], d[3]]
    pk = [_ls(10 + k, p, op=8 if k % 2 else 12)
          for k, p in enumerate(order)]
    reps = _list(srv, pk, gpu)
    for p, r in zip(order, reps):
        assert len(model[p]) == 100
        _check_ok(r, model[p])
    assert bool((srv.list_want == _lib.LIST_IDLE).all().item())
    order = [d[7], d[8], d[7], '/bench', d[9]]
    reps = _list(srv, [_ls(50 + k, p) for k, p in enumerate(order)], gpu)
    for p, r in zip(order, reps):
        _check_ok(r, model[p])
    assert bool((srv.list_want == _lib.LIST_IDLE).all().item())


def _create(x, path, flags=()):
    return {'xid': x, 'opcode': 'CREATE', 'path': path, 'data': b'c',
            'acl': jute.DEFAULT_ACL, 'flags': list(flags)}


def test_lists_follow_writes(gpu):
    """Creates (plain and SEQUENTIAL, paths past the 40 bytes a hash entry
    holds), deletes, creates that recycle the freed nodes under another
    parent, EPHEMERAL children and their session's expiry, all through
    serve(): after each stage every touched parent lists its model, agrees
    with its numChildren and with GpuTree.children_host, and no freed node
    shows."""
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(200, 16, fanout=20, device=gpu, spare=2.0)
    srv = GpuServer(tree, 256, 1 << 20, window=512)
    model = _path_model(tree)
    a, b, c = '/bench/d000001', '/bench/d000004', '/bench/d000009'
    xid = [1000]

    def write(pk):
        reps = _serve(srv, pk, gpu, session=0x51)
        assert [r['err'] for r in reps] == ['OK'] * len(pk), reps
        return reps

    def nx():
        xid[0] += 1
        return xid[0]

    def check(parents):
        reps = _list(srv, [_ls(nx(), p, op=12 if k % 2 else 8)
                           for k, p in enumerate(parents)], gpu)
        for p, r in zip(parents, reps):
            _check_ok(r, sorted(model[p]))
            assert tree.children_host(p) == sorted(model[p])
        # a deleted path lists NO_NODE and has no host children either
        return reps

    long_name = 'k' * 45
    # 1. plain and SEQUENTIAL creates with long names
    pk = [_create(nx(), '%s/%s-%02d' % (a, long_name, k)) for k in range(30)]
    pk += [_create(nx(), '%s/%s-' % (b, long_name), ['SEQUENTIAL'])
           for _ in range(30)]
    for p, r in zip(pk, write(pk)):
        d, _, name = r['path'].rpartition('/')
        assert len(r['path']) > 40
        model[d].append(name)
    check([a, b, c, '/bench'])
    # 2. delete some of the new and some of the static children
    gone = sorted(model[a])[5:25] + sorted(model[a])[-4:]
    write([{'xid': nx(), 'opcode': 'DELETE', 'path': a + '/' + g,
            'version': -1} for g in gone])
    model[a] = [x for x in model[a] if x not in gone]
    reps = check([a, b])
    ls_gone = _list(srv, [_ls(nx(), a + '/' + gone[0])], gpu)
    assert ls_gone[0]['err'] == 'NO_NODE'
    assert tree.children_host(a + '/' + gone[0]) is None
    # 3. create again: the freed nodes come back under another parent
    hw = int(tree.counters[_lib.TC_NODES].item())
    pk = [_create(nx(), '%s/re-%02d' % (c, k)) for k in range(len(gone))]
    write(pk)
    model[c] += ['re-%02d' % k for k in range(len(gone))]
    assert int(tree.counters[_lib.TC_NODES].item()) == hw     # recycled
    check([a, b, c])
    # 4. EPHEMERAL children of one session, then its expiry
    pk = [_create(nx(), '%s/eph-%02d' % (p, k), ['EPHEMERAL'])
          for k in range(12) for p in (a, c)]
    write(pk)
    keep = {p: list(model[p]) for p in (a, c)}
    for p in (a, c):
        model[p] += ['eph-%02d' % k for k in range(12)]
    check([a, b, c])
    assert int(tree.expire(0x51).item()) == 24
    model.update(keep)
    check([a, b, c, '/bench'])


def _notes(srv):
    buf, total, slots, count = srv.notif
    n = int(count.item())
    raw = bytes(buf[:int(total.item())].cpu().numpy().tobytes())
    frames, _, bad = jute.scan_frames(raw)
    assert bad < 0 and len(frames) == n
    out = []
    for (o, ln), s in zip(frames, slots[:n].cpu().tolist()):
        pkt = jute.decode_response(raw[o:o + ln], {})
        out.append((s, pkt['type'], pkt['path']))
    return out


def test_list_arms_child_watch(gpu):
    """A list with watch=1 arms the one-shot child watch of the caller's
    watcher slot: the next create under the directory notifies slot 3 once,
    a second create nothing; a listed missing path arms nothing."""
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(300, 16, fanout=100, device=gpu, watch_cap=256)
    srv = GpuServer(tree, 64, 1 << 18, window=256)
    d0, d1 = '/bench/d000000', '/bench/d000001'
    reps = _list(srv, [_ls(1, d0, watch=True),
                       _ls(2, d1 + '/nope', op=8, watch=True),
                       _ls(3, d1, watch=False)], gpu, wslot=3)
    assert [r['err'] for r in reps] == ['OK', 'NO_NODE', 'OK']
    r = _serve(srv, [_create(4, d0 + '/kid1')], gpu)
    assert r[0]['err'] == 'OK'
    assert _notes(srv) == [(3, 'CHILDREN_CHANGED', d0)]
    r = _serve(srv, [_create(5, d0 + '/kid2')], gpu)
    assert r[0]['err'] == 'OK' and _notes(srv) == []
    # nothing was armed on d1 (watch=0) or on the missing path
    r = _serve(srv, [_create(6, d1 + '/nope')], gpu)
    assert r[0]['err'] == 'OK' and _notes(srv) == []
    r = _serve(srv, [_create(7, d1 + '/nope/kid')], gpu)
    assert r[0]['err'] == 'OK' and _notes(srv) == []
    names = _list(srv, [_ls(8, d0)], gpu)[0]['children']
    assert 'kid1' in names and 'kid2' in names and len(names) == 102


def _limit_setup(gpu):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(250, 16, fanout=100, device=gpu)
    srv = GpuServer(tree, 64, 1 << 18, window=256)
    return tree, srv


def test_output_overflow(gpu):
    """An output one byte short of the stream: error flag 2, total 0, and
    not a byte written — the guard bytes past the capacity included."""
    tree, srv = _limit_setup(gpu)
    pk = [_ls(k, '/bench/d%06d' % (k % 3), op=8 if k % 2 else 12)
          for k in range(7)]
    s = _frames(pk)
    rx = _dev_bytes(s, gpu)
    _, total, err, ft = srv.serve_list(rx, len(s))
    T = int(total.item())
    assert T > 1000 and int(err.item()) == 0
    out = torch.full((T + 256,), 0xAB, dtype=torch.uint8, device=gpu)
    tot = torch.full((1,), -1, dtype=torch.int64, device=gpu)
    er = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    _lib.tree_list(tree.tensors, rx, ft.off, ft.length, ft.count,
                   srv.cap_frames, -1, 1 << 24, srv.list_want, srv.list_ws,
                   out, T - 1, srv.list_rec_off, tot, er)
    assert int(er.item()) == 2 and int(tot.item()) == 0
    assert bool((out == 0xAB).all().item())
    assert bool((srv.list_want == _lib.LIST_IDLE).all().item())
    # exactly enough room: the whole stream, nothing past it
    _lib.tree_list(tree.tensors, rx, ft.off, ft.length, ft.count,
                   srv.cap_frames, -1, 1 << 24, srv.list_want, srv.list_ws,
                   out, T, srv.list_rec_off, tot, er)
    assert int(er.item()) == 0 and int(tot.item()) == T
    assert bool((out[T:] == 0xAB).all().item())
    reps = _decode(out, tot, pk)
    assert all(len(r['children']) in (100, 50) for r in reps)


def test_max_frame_demotes_large_replies(gpu):
    """max_frame=256: the big directories are answered SYSTEMERROR with a
    header only — their GET_CHILDREN2 and GET_CHILDREN copies alike — and
    the small replies around them are whole."""
    tree, srv = _limit_setup(gpu)
    leaf = '/bench/d000000/n000000007'
    pk = [_ls(1, leaf), _ls(2, '/bench/d000000'), _ls(3, '/bench'),
          _ls(4, '/bench/d000002', 8), _ls(5, '/bench/d000000', 8),
          _ls(6, leaf, 8)]
    reps = _list(srv, pk, gpu, max_frame=256)
    assert [r['err'] for r in reps] == ['OK', 'SYSTEM_ERROR', 'OK',
                                        'SYSTEM_ERROR', 'SYSTEM_ERROR', 'OK']
    assert all(r['_len'] == 16 for r in reps if r['err'] != 'OK')
    _check_ok(reps[0], [])
    _check_ok(reps[2], ['d000000', 'd000001', 'd000002'])
    _check_ok(reps[5], [])
    # a limit between the two frame sizes of one parent: GET_CHILDREN fits,
    # GET_CHILDREN2 (68 bytes of Stat more) does not; the copy that fits is
    # whole although the parent's first request was demoted
    size8 = 4 + 16 + 4 + 50 * 14
    pk = [_ls(7, '/bench/d000002', 12), _ls(8, '/bench/d000002', 8),
          _ls(9, '/bench/d000002', 8)]
    reps = _list(srv, pk, gpu, max_frame=size8)
    assert [r['err'] for r in reps] == ['SYSTEM_ERROR', 'OK', 'OK']
    want = ['n%09d' % i for i in range(200, 250)]
    _check_ok(reps[1], want)
    _check_ok(reps[2], want)


def test_empty_batch_and_terminator(gpu):
    tree, srv = _limit_setup(gpu)
    rx = torch.zeros(64, dtype=torch.uint8, device=gpu)
    out, total, err, _ = srv.serve_list(rx, 0)
    assert int(total.item()) == 0 and int(err.item()) == 0
    out, total, err, _ = srv.serve_list(rx, 0, terminate=True)
    assert int(total.item()) == 0 and int(err.item()) == 0
    assert out[:4].cpu().tolist() == [255] * 4
    pk = [_ls(1, '/bench/d000001')]
    s = _frames(pk)
    out, total, err, _ = srv.serve_list(_dev_bytes(s, gpu), len(s),
                                        terminate=True)
    T = int(total.item())
    assert out[T:T + 4].cpu().tolist() == [255] * 4
    _check_ok(_decode(out, total, pk)[0],
              ['n%09d' % i for i in range(100, 200)])


def test_sharded_tree_refused(gpu):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(200, 16, fanout=100, device=gpu, shard=(0, 2))
    srv = GpuServer(tree, 64, 1 << 16, window=256)
    s = _frames([_ls(1, '/bench/d000000')])
    with pytest.raises(ValueError, match='sharded'):
        srv.serve_list(_dev_bytes(s, gpu), len(s))


def test_op_argument_checks(gpu):
    """tree_list checks every tensor before a pointer reaches a kernel."""
    tree, srv = _limit_setup(gpu)
    s = _frames([_ls(1, '/bench/d000000')])
    rx = _dev_bytes(s, gpu)
    _, _, _, ft = srv.serve_list(rx, len(s))
    out = torch.empty(1 << 12, dtype=torch.uint8, device=gpu)
    tot = torch.zeros(1, dtype=torch.int64, device=gpu)
    er = torch.zeros(1, dtype=torch.int32, device=gpu)

    def call(**kw):
        a = dict(want=srv.list_want, ws=srv.list_ws, out=out,
                 rec_off=srv.list_rec_off, total=tot, err=er, wslot=-1,
                 foff=ft.off, out_cap=out.numel())
        a.update(kw)
        _lib.tree_list(tree.tensors, rx, a['foff'], ft.length, ft.count,
                       srv.cap_frames, a['wslot'], 1 << 24, a['want'],
                       a['ws'], a['out'], a['out_cap'], a['rec_off'],
                       a['total'], a['err'])

    with pytest.raises(RuntimeError, match='want must be Int'):
        call(want=srv.list_want.to(torch.int64))
    with pytest.raises(RuntimeError, match='frame_off must be Long'):
        call(foff=ft.off.to(torch.int32))
    with pytest.raises(RuntimeError, match='must be a GPU tensor'):
        call(out=out.cpu())
    with pytest.raises(RuntimeError, match='want has'):
        call(want=srv.list_want[:tree.cap - 1])
    with pytest.raises(RuntimeError, match='list workspace has'):
        call(ws=srv.list_ws[:srv.list_ws.numel() - 16])
    with pytest.raises(RuntimeError, match='rec_off has'):
        call(rec_off=srv.list_rec_off[:srv.cap_frames - 1])
    with pytest.raises(RuntimeError, match='out has'):
        call(out_cap=out.numel() + 1)
    with pytest.raises(RuntimeError, match='contiguous'):
        call(want=torch.full((2 * tree.cap,), _lib.LIST_IDLE,
                             dtype=torch.int32, device=gpu)[::2])
    with pytest.raises(RuntimeError, match='watcher slot'):
        call(wslot=64)
    assert _lib.tree_list_workspace(64) == srv.list_ws.numel()
    call()                                        # and the good call runs
    assert int(er.item()) == 0 and int(tot.item()) > 1000


def test_list_pipeline_capture_replay(gpu):
    """ListPipeline on a 20k-node tree: an eager step, then the captured
    step replayed three times; the device check stays clean and the first
    replay's replies decode to the same children as the eager step's."""
    from zkmi.bench.synthetic import ListPipeline
    from zkmi.server.tree import GpuTree
    tree = GpuTree(20_000, 16, fanout=100, device=gpu)
    pipe = ListPipeline(tree, 512)            # 200 directories, duplicates

    def children():
        rep, rx, ft, total = pipe.last
        raw = bytes(rx[:int(total.item())].cpu().numpy().tobytes())
        frames, used, bad = jute.scan_frames(raw)
        assert bad < 0 and used == len(raw) and len(frames) == 512
        xmap = {k: 'GET_CHILDREN2' for k in range(512)}
        out = []
        for o, ln in frames:
            r = jute.decode_response(raw[o:o + ln], xmap)
            assert r['err'] == 'OK' and r['stat'].numChildren == 100
            out.append((r['xid'], tuple(sorted(r['children']))))
        return out

    acc = pipe.step()
    torch.cuda.synchronize()
    assert int(acc.item()) == 512 and int(pipe.bad.item()) == 0, \
        pipe.diagnose()
    eager = children()
    assert eager[0][1] == tuple('n%09d' % i for i in range(100))
    assert eager[200] == (200, eager[0][1])   # request 200: directory 0 again
    acc = torch.zeros(1, dtype=torch.int64, device=gpu)
    g = pipe.capture(acc)
    g.replay()
    torch.cuda.synchronize()
    assert children() == eager
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert int(acc.item()) == 3 * 512 and int(pipe.bad.item()) == 0, \
        pipe.diagnose()
    # the expanded name table: one row per child, inside the reply stream
    n = int(pipe.nstr.item())
    assert n == 512 * 100 == pipe.want_children
    assert bool((pipe.slen[:n] == 10).all().item())
