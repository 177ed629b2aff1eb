"""The GPU server's data path at payload sizes from 0 bytes to 1 MB, model
checked (tests/treemodel.py): znodes of every length of the ladder in
tests/sizeladder.py are created, read at every start residue mod 16, set,
recycled, served in order, served through the mixed entry points, imaged and
loaded again, and sent over the socket; the uniform reply writer runs at a
reply size of 4192 bytes.  Every reply is compared with the fake server's
database, every audit reads every live znode's bytes and Stat.  All
comparisons are exact."""

import copy
import os
import random
import struct
import threading

import pytest
import torch

from sizeladder import (BIG, BIG_HOLE, ENC_T, GET_REG_DATA, HOLE_TRIP,
                        LADDER_DIR, ReplyCoverage, create_ladder, ladder,
                        ladder_tree, rand_bytes, read_batch)
from treemodel import (_decode, _stream, create, delete, dev_bytes, get,
                       set_data)

from zkmi import consts, jute
from zkmi.ops import _lib
from zkmi.utils import treeimage as TI

pytestmark = pytest.mark.gpu

D0 = '/bench/d000000'
STATIC = D0 + '/n%09d'
PAD = LADDER_DIR + '/pad%02d'


@pytest.fixture(scope='module')
def lad(gpu):
    """Stage 1's tree: one znode of random data per ladder size (each
    CREATE compared with the model, one audit at the end) and 16 pad nodes
    of 0..15 bytes.  (model, {size: path})."""
    m = ladder_tree(gpu, acl_cap=8)
    paths = create_ladder(m, ladder(big=True))
    rng = random.Random(3)
    m.serve([create(PAD % r, rand_bytes(rng, r)) for r in range(16)],
            audit=False)
    return m, paths


def _raw_serve(m, pk, serve=None, **kw):
    """The reply stream's bytes and frame starts for ``pk`` (xids from the
    model's counter; the model is not told: reads only)."""
    for p in pk:
        p['xid'] = m.xid
        m.xid += 1
    s = _stream(pk)
    out, total, err, _ = (serve or m.srv.serve)(dev_bytes(s, m.dev), len(s),
                                                **kw)
    assert int(err.item()) == 0
    raw = bytes(out[:int(total.item())].cpu().numpy().tobytes())
    frames, used, bad = jute.scan_frames(raw)
    assert bad < 0 and used == len(raw) and len(frames) == len(pk)
    return raw, [o - 4 for o, _ in frames]


# ---- 1. create, read back ---------------------------------------------------

def test_create_and_read_back(lad):
    """Every ladder znode answers its bytes and Stat to GET_DATA and EXISTS
    in one batch, the 1 000 000-byte one among them."""
    m, paths = lad
    assert sorted(paths) == sorted(ladder(big=True))
    reps, _ = m.serve(read_batch(paths), audit=False)
    got = {len(r['data'] or b'') for r in reps if r['opcode'] == 'GET_DATA'}
    assert got == set(paths)
    cap = m.slot_cap
    for dl, p in paths.items():
        assert int(cap[m.node_of[p]]) == max(dl, 128), dl


# ---- 2. start residues ------------------------------------------------------

def test_read_at_every_start_residue(lad):
    """The read batch 16 times, led by a GET of a pad node of 0..15 bytes:
    every reply starts at every residue mod 16.  Through the host mirror of
    resp_write's rules: at every residue replies lie on both sides of the
    register path's bound, of the hole rule and of copy_hole_q's 1 KiB trip;
    some block holds a number of holes that is no multiple of 4 and some
    block more than 4."""
    m, paths = lad
    small = {dl: p for dl, p in paths.items() if dl != BIG}
    cov = ReplyCoverage()
    seen = [set() for _ in range(16)]
    for r in range(16):
        pk = read_batch(small, lead=get(PAD % r))
        reps, _ = m.serve(pk, audit=False)
        rec = m.srv.last_rec_off[:len(pk)].cpu().tolist()
        dls, offs, o = [], [], 0
        for p, rep in zip(pk, reps):
            assert rep['err'] == 'OK'
            offs.append(o)
            if p['opcode'] == 'GET_DATA':
                dl = len(rep['data'] or b'')
                dls.append(dl)
                o += 92 + dl
            else:
                dls.append(None)
                o += 88
        assert rec == offs
        cov.add(offs, dls)
        for o, dl in zip(offs[1:], dls[1:]):
            if dl is not None:
                seen[o & 15].add(dl)
    cov.check()
    assert all(s == set(small) for s in seen)
    assert GET_REG_DATA in small and GET_REG_DATA + 1 in small
    assert BIG_HOLE in small and HOLE_TRIP in small


# ---- 3. SET_DATA ------------------------------------------------------------

def test_set_data_at_the_slot_capacity(lad):
    """SET_DATA on created znodes at exactly the slot capacity, one byte
    past it (BAD_ARGUMENTS, the node untouched), down to 0 bytes (length -1
    on the wire, dataLength 0) and back up; on a static znode at the tree's
    ``data_bytes`` and one past."""
    m, paths = lad
    rng = random.Random(11)
    picks = [5, 128, 129, 300, 1024, 4097, 28 * 1024 + 8, 65537]
    caps = {dl: max(dl, 128) for dl in picks}
    assert all(int(m.slot_cap[m.node_of[paths[dl]]]) == caps[dl]
               for dl in picks)
    static = STATIC % 3
    sc = m.tree.data_bytes
    assert int(m.slot_cap[m.node_of[static]]) == sc == 4096
    # at the capacity
    m.serve([set_data(paths[dl], rand_bytes(rng, caps[dl])) for dl in picks] +
            [set_data(static, rand_bytes(rng, sc), 0)], audit=False)
    # one past: refused, and the reads of the next batch show the old bytes
    _, want = m.serve([set_data(paths[dl], rand_bytes(rng, caps[dl] + 1))
                       for dl in picks] +
                      [set_data(static, rand_bytes(rng, sc + 1))],
                      audit=False)
    assert {w[1] for w in want} == {'BAD_ARGUMENTS'}
    m.serve([get(paths[dl]) for dl in picks] + [get(static)], audit=False)
    # to nothing
    m.serve([set_data(paths[dl], b'', 1) for dl in picks] +
            [set_data(static, b'')], audit=False)
    pk = [get(paths[dl]) for dl in picks] + [get(static)]
    raw, starts = _raw_serve(m, pk)
    for o in starts:
        assert raw[o:o + 4] == struct.pack('>i', 16 + 4 + 68)
        assert raw[o + 20:o + 24] == b'\xff' * 4
        st = jute.JuteReader(raw[o + 24:o + 92], 0).read_stat()
        assert st.dataLength == 0 and st.version == 2
    # and back to the first length
    m.serve([set_data(paths[dl], rand_bytes(rng, dl), 2) for dl in picks] +
            [set_data(static, rand_bytes(rng, 4096))])


# ---- 4. recycling, a full slab ----------------------------------------------

def _recycle(m, old, new, dl, rng):
    """DELETE ``old`` and, in the next batch, CREATE ``new`` with ``dl``
    bytes on the node it freed.  Returns (node, its capacity before, the
    slab top before, its slot offset before)."""
    v = m.node_of[old]
    cap0 = int(m.tree.slot_cap[v].item())
    off0 = int(m.tree.slot_off[v].item())
    m.serve([delete(old)], audit=False)
    top0 = m.counter(_lib.TC_SLAB_TOP)
    m.serve([create(new, rand_bytes(rng, dl))])
    assert m.node_of[new] == v
    return v, cap0, top0, off0


def test_recycled_slots_and_a_full_slab(gpu):
    """A freed node's slot is kept when the new data fits its capacity and
    replaced (at the slab top) when it does not: smaller than, equal to and
    larger than the capacity of a large and of a small freed node.  Then
    CREATEs until the slab is full: the refusals are SYSTEMERROR, the audit
    passes, and the next small CREATE is refused too (the slab top is not
    rolled back: tree.hip, the serve's phase A claims it with wave_bytes
    before it knows that the slot fits)."""
    m = ladder_tree(gpu)
    t = m.tree
    rng = random.Random(13)
    R = '/bench/R'
    m.serve([create(R)], audit=False)
    m.serve([create(R + '/big0', rand_bytes(rng, 40000)),
             create(R + '/small0', rand_bytes(rng, 10)),
             create(R + '/keep', rand_bytes(rng, 5000))])
    # the large node: smaller, equal, larger
    v, cap0, top0, off0 = _recycle(m, R + '/big0', R + '/big1', 3000, rng)
    assert cap0 == 40000
    assert int(t.slot_cap[v].item()) == 40000
    assert int(t.slot_off[v].item()) == off0
    assert m.counter(_lib.TC_SLAB_TOP) == top0
    v, cap0, top0, off0 = _recycle(m, R + '/big1', R + '/big2', 40000, rng)
    assert (int(t.slot_cap[v].item()), int(t.slot_off[v].item())) == \
        (40000, off0)
    assert m.counter(_lib.TC_SLAB_TOP) == top0
    v, cap0, top0, off0 = _recycle(m, R + '/big2', R + '/big3', 40001, rng)
    assert (int(t.slot_cap[v].item()), int(t.slot_off[v].item())) == \
        (40001, top0)
    assert m.counter(_lib.TC_SLAB_TOP) == top0 + _lib.SLOT_DATA + 40016 + 4
    # the small one (capacity 128): within, equal, larger
    v, cap0, top0, off0 = _recycle(m, R + '/small0', R + '/small1', 0, rng)
    assert cap0 == 128
    assert (int(t.slot_cap[v].item()), int(t.slot_off[v].item())) == \
        (128, off0)
    v, cap0, top0, off0 = _recycle(m, R + '/small1', R + '/small2', 128, rng)
    assert (int(t.slot_cap[v].item()), int(t.slot_off[v].item())) == \
        (128, off0)
    assert m.counter(_lib.TC_SLAB_TOP) == top0
    v, cap0, top0, off0 = _recycle(m, R + '/small2', R + '/small3', 129, rng)
    assert (int(t.slot_cap[v].item()), int(t.slot_off[v].item())) == \
        (129, top0)
    # what the recycled slots hold is what a SET_DATA may grow to
    _, want = m.serve([set_data(R + '/big3', rand_bytes(rng, 40002)),
                       set_data(R + '/small3', rand_bytes(rng, 129)),
                       set_data(R + '/small3x', b'')])
    assert [w[1] for w in want] == ['BAD_ARGUMENTS', 'OK', 'NO_NODE']
    # fill the slab
    room = t.slab_cap - m.counter(_lib.TC_SLAB_TOP)
    each = _lib.SLOT_DATA + 65536 + 4
    n = room // each + 8
    assert 30 < n < 100
    got = m.serve_full_index([create('%s/f%03d' % (R, k),
                                     rand_bytes(rng, 65536))
                              for k in range(n)])
    assert got.count('OK') == room // each
    assert got.count('SYSTEM_ERROR') == 8
    assert m.counter(_lib.TC_SLAB_TOP) > t.slab_cap
    before = m.tree.digest()
    assert m.serve_full_index([create(R + '/late', b'x')]) == ['SYSTEM_ERROR']
    assert m.tree.digest() == before


# ---- 5. the ordered serve's snapshots ---------------------------------------

def _chain(path, big, big2, small):
    return [create(path, big), set_data(path, big2), get(path),
            set_data(path, small), get(path), delete(path)]


def test_ordered_chains_snapshot_their_replies(gpu):
    """create(big) -> set(big') -> get -> set(small) -> get -> delete of
    one path in one ordered batch, for data below the register path's
    bound, about 300 bytes and past the 28 KiB image, the three chains
    interleaved: every reply as the model gives it applying the batch one by
    one (the reads and sets that a later write overtakes answer from their
    snapshot in the scratch tail).  Then a chain whose snapshot does not fit
    the scratch tail: that read is answered SYSTEMERROR, order_stats reports
    more bytes asked for than the tail holds, and the nodes are sound."""
    m = ladder_tree(gpu, scratch=1 << 20)
    rng = random.Random(17)
    O = '/bench/O'
    m.serve([create(O)], audit=False)
    sizes = (100, 300, 28 * 1024 + 333)
    chains = [_chain('%s/c%d' % (O, k), rand_bytes(rng, dl),
                     rand_bytes(rng, dl), rand_bytes(rng, 5 + k))
              for k, dl in enumerate(sizes)]
    pk = [c[j] for j in range(6) for c in chains]
    reps, _ = m.serve(pk, zxids=False, ordered=True, passes=6)
    assert [r['err'] for r in reps] == ['OK'] * len(pk)
    rank, used = m.srv.order_stats()
    assert rank == 5
    # each chain's snapshots, a slot of SLOT_DATA + the data rounded up to
    # 16 + 4 bytes each: two sets (no data), the get of the long data, the
    # get of the short (under 16 bytes)
    slot = _lib.SLOT_DATA + 4
    assert used == sum(2 * slot + (slot + ((dl + 15) & ~15)) + (slot + 16)
                       for dl in sizes)
    # the chains again with nothing deleted: the last get is no snapshot
    pk = [c[j] for j in range(5) for c in chains]
    m.serve(pk, zxids=False, ordered=True, passes=6)
    # a snapshot that finds no room
    m2 = ladder_tree(gpu, scratch=4096)
    m2.serve([create(O)], audit=False)
    p = O + '/over'
    pk = [create(p, rand_bytes(rng, 30000)), get(p),
          set_data(p, rand_bytes(rng, 7))]
    for q in pk:
        q['xid'] = m2.xid
        m2.xid += 1
    s = _stream(pk)
    base = m2.counter(_lib.TC_ZXID)
    out, total, err, _ = m2.srv.serve(dev_bytes(s, gpu), len(s), ordered=True,
                                      passes=4)
    assert int(err.item()) == 0
    reps = _decode(out, total, pk)
    assert [r['err'] for r in reps] == ['OK', 'SYSTEM_ERROR', 'OK']
    rank, used = m2.srv.order_stats()
    assert rank == 2 and used > 4096
    assert m2._apply(pk[0], None, base + 1, False)[1] == 'OK'
    assert m2._apply(pk[2], None, base + 3, False)[1] == 'OK'
    m2.audit(zxids=False)


# ---- 6. the same requests through the mixed entry points --------------------

def _frames_of(raw, starts):
    return [raw[a:b] for a, b in zip(starts, starts[1:] + [len(raw)])]


def _rezxid(frame, zxid):
    return frame[:8] + struct.pack('>q', zxid) + frame[16:]


def test_mixed_entry_points_give_the_same_bytes(lad, gpu):
    """The read batch with GET_CHILDREN2 and GET_ACL frames between,
    through serve_mixed and through serve_sessions_mixed with 3 segments:
    every reply the bytes that serve, serve_list and serve_acl gave for it,
    the header's zxid apart (a served batch moves the counter on: the serve's
    class carries the counter as the batch found it, the other two engines'
    replies the counter behind the serve's requests).  The children of a
    reply are in one wave's order for parents of a few children; LADDER_DIR's
    are compared as a set."""
    from zkmi.server.engine import SessionSegments
    m, paths = lad
    srv = m.srv
    small = {dl: p for dl, p in paths.items() if dl != BIG}
    pk = read_batch(small)
    ls = lambda p: {'opcode': 'GET_CHILDREN2', 'path': p,    # noqa: E731
                    'watch': False}
    ga = lambda p: {'opcode': 'GET_ACL', 'path': p}          # noqa: E731
    extra = [ls('/bench'), ga(paths[300]), ls(D0), ga(D0 + '/nope'),
             ls(LADDER_DIR), ga(paths[65537]), ls(paths[5]), ga('/bench')]
    step = len(pk) // (len(extra) + 1)
    for k, e in enumerate(extra):
        pk.insert((k + 1) * step + k, e)
    cls = [2 if p['opcode'] == 'GET_CHILDREN2' else
           1 if p['opcode'] == 'GET_ACL' else 0 for p in pk]
    ref = {}
    for c, serve in ((0, srv.serve), (1, srv.serve_acl), (2, srv.serve_list)):
        part = [p for p, k in zip(pk, cls) if k == c]
        raw, starts = _raw_serve(m, part, serve)
        ref[c] = _frames_of(raw, starts)
    n_serve = cls.count(0)
    big_list = pk.index(extra[4])

    def check(raw, starts, base):
        got = _frames_of(raw, starts)
        it = {c: iter(ref[c]) for c in ref}
        for i, (g, c) in enumerate(zip(got, cls)):
            w = _rezxid(next(it[c]), base if c == 0 else base + n_serve)
            if i == big_list:
                x = {pk[i]['xid']: 'GET_CHILDREN2'}
                a, b = (jute.decode_response(f[4:], x) for f in (g, w))
                assert len(g) == len(w) and len(a['children']) > 250
                assert sorted(a['children']) == sorted(b['children'])
                assert g[-68:] == w[-68:] and g[:24] == w[:24]
                continue
            assert g == w, (i, pk[i]['opcode'], pk[i]['path'], len(g), len(w))

    xids = [p['xid'] for p in pk]
    s = _stream(pk)
    rx = dev_bytes(s, gpu)
    base = m.counter(_lib.TC_ZXID)
    out, total, err, _ = srv.serve_mixed(rx, len(s))
    assert int(err.item()) == 0
    raw = bytes(out[:int(total.item())].cpu().numpy().tobytes())
    starts = srv.last_rec_off[:len(pk)].cpu().tolist()
    check(raw, starts, base)
    # three connections: the batch cut in three
    cut = [0, len(pk) // 3, len(pk) // 2, len(pk)]
    fl = [len(jute.frame(jute.encode_request(p))) for p in pk]
    bstart = [sum(fl[:c]) for c in cut]
    segs = SessionSegments(
        torch.tensor(bstart, dtype=torch.int64, device=gpu),
        torch.tensor([0, 0, 0], dtype=torch.int64, device=gpu),
        torch.tensor([-1, -1, -1], dtype=torch.int32, device=gpu))
    base = m.counter(_lib.TC_ZXID)
    out, total, err, _ = srv.serve_sessions_mixed(rx, len(s), segs)
    assert int(err.item()) == 0
    raw2 = bytes(out[:int(total.item())].cpu().numpy().tobytes())
    starts2 = srv.last_rec_off[:len(pk)].cpu().tolist()
    assert starts2 == starts and len(raw2) == len(raw)
    check(raw2, starts2, base)
    off = srv.seg.rep_off.cpu().tolist()
    assert off == [starts[c] for c in cut[:3]] + [len(raw)]
    assert [p['xid'] for p in pk] == xids


# ---- 7. the image -----------------------------------------------------------

def test_image_of_the_ladder(lad, gpu):
    """tree.snapshot() unpacked on the host holds the model's znodes, byte
    for byte; loaded into a fresh tree, the model's audit passes on it."""
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    m, paths = lad
    img = m.tree.snapshot()
    raw = bytes(img.cpu().numpy().tobytes())
    assert TI.check(raw) == (TI.OK, -1)
    hd, recs = TI.unpack(raw)
    live = sorted(m.live())
    assert sorted(r['path'] for r in recs) == live
    assert hd['max_data'] == BIG
    for r in recs:
        node = m.db.nodes[r['path']]
        assert r['data'] == bytes(node.data or b''), r['path']
        st = r['stat']
        got = (st.version, st.dataLength, st.numChildren, st.cversion,
               st.ephemeralOwner, st.czxid, st.mzxid, st.pzxid)
        assert got == m._stat_key(r['path'], True), r['path']
    assert hd['digest'] == TI.digest(recs) == m.tree.digest()[0]
    t = GpuTree.load(img, device=gpu, acl_cap=8)
    assert torch.equal(t.snapshot(), img)
    m2 = copy.copy(m)
    m2.tree, m2.srv = t, GpuServer(t, 1024, 20 << 20)
    m2.touched = {'/bench', D0, LADDER_DIR}
    m2.audit()
    assert int(m2.slot_cap[m2.node_of[paths[BIG]]]) == BIG
    assert int(m2.slot_cap[m2.node_of[paths[5]]]) == 128


# ---- 8. the uniform writer at a large S -------------------------------------

@pytest.mark.parametrize('case', ['plain', 'one_error'])
def test_uniform_writer_large_replies(gpu, case):
    """K13 on a full block (and a ragged one) of successful GET_DATA replies
    of 4192 bytes each, a multiple of 16: the blocks emit_uniform takes.
    With one error reply in the first block that block goes through the
    image and the holes."""
    from zkmi.ops import batch as B
    from zkmi.server.tree import GpuTree
    tree = GpuTree(300, 4100, fanout=100, device=gpu, spare=0.0)
    assert 4 + 16 + 4 + 4100 + 68 == 4192 and 4192 % 16 == 0
    rng = random.Random(23)
    n = ENC_T + 40
    nodes = [rng.randrange(tree.leaf0, tree.n_static) for _ in range(n)]
    zx = [rng.randint(0, 2 ** 40) for _ in range(n)]
    errs = [0] * n
    if case == 'one_error':
        errs[77] = -101
    T = lambda a, dt: torch.tensor(a, dtype=dt, device=gpu)  # noqa: E731
    resp = B.ResponseBatch(
        T([consts.OP_CODES['GET_DATA']] * n, torch.int32),
        T(list(range(n)), torch.int32), T(errs, torch.int32),
        T(nodes, torch.int64), T(zx, torch.int64),
        T([0] * n, torch.int64), T([0] * n, torch.int32),
        dev_bytes(b'\0' * 16, gpu), T([1] * n, torch.int32),
        T([n], torch.int64))
    slots = {nd: tree.node_slot_host(nd) for nd in set(nodes)}
    want = b''.join(jute.frame(jute.encode_response(
        {'xid': i, 'zxid': zx[i], 'err': errs[i], 'opcode': 'GET_DATA',
         'stat': slots[nodes[i]][1], 'data': slots[nodes[i]][0]}))
        for i in range(n))
    t = len(want)
    assert t == 4192 * (n - sum(1 for e in errs if e)) + \
        20 * sum(1 for e in errs if e)
    cap = t + 256
    out = torch.full((cap,), 0xAB, dtype=torch.uint8, device=gpu)
    out, rec_off, total, err = B.encode_responses(resp, tree.store, cap,
                                                  out=out, terminate=True)
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and int(total.item()) == t
    hb = out.cpu().numpy().tobytes()
    if hb[:t] != want:
        bad = next(i for i in range(t) if hb[i] != want[i])
        raise AssertionError('stream differs at byte %d' % bad)
    assert hb[t:t + 4] == b'\xff' * 4
    end = (t + 4 + 15) & ~15
    assert hb[end:] == b'\xab' * (cap - end)


def test_uniform_writer_large_replies_lds_image(gpu):
    """The same full block through the LDS image and the holes instead of
    the uniform writer (ZKMI_ENC_UNIFORM=0 is read once per process: a child
    process)."""
    import subprocess
    import sys
    env = dict(os.environ, ZKMI_ENC_UNIFORM='0')
    res = subprocess.run(
        [sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider',
         os.path.abspath(__file__) +
         '::test_uniform_writer_large_replies[plain]'],
        env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


# ---- 9. over the socket -----------------------------------------------------

@pytest.fixture
def front(gpu):
    """tests/test_gpu_front_end.py's server with room for 100 000-byte
    znodes: a slab of 4.3 MB, 4 MiB of replies a tick.  ``raw_cap``, the
    longest request frame the front end takes, stays at its default of
    1 MiB."""
    from zkmi.server.gpu import GpuZKServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(10, 4096, fanout=10, spare=0.0, watch_cap=256, acl_cap=8,
                   device=gpu)
    s = GpuZKServer(tree, cap_frames=256, out_cap=4 << 20, max_conns=16)
    yield s
    s.shutdown()
    assert s.error is None, s.error


def _big_node_script(c, path, seed):
    rng = random.Random(seed)
    a, b = rand_bytes(rng, 100000), rand_bytes(rng, 40000)
    assert c.call_sync('create', path, a, {}, timeout=10) == path
    data, st = c.call_sync('get', path, timeout=10)
    assert bytes(data) == a and (st.dataLength, st.version) == (100000, 0)
    c.call_sync('set', path, b, 0, timeout=10)
    st = c.call_sync('stat', path, timeout=10)
    assert (st.dataLength, st.version) == (40000, 1)
    data, st = c.call_sync('get', path, timeout=10)
    assert bytes(data) == b and (st.dataLength, st.version) == (40000, 1)


def test_big_znodes_over_the_socket(front):
    """A Client creates a 100 000-byte znode, gets it, sets it to 40 000
    bytes and gets it again; then two clients do the same at once."""
    from zkhelpers import client
    c = client(front.servers())
    c.wait_connected(10)
    _big_node_script(c, D0 + '/big', 1)
    d = client(front.servers())
    d.wait_connected(10)
    errs = []

    def run(cl, path, seed):
        try:
            _big_node_script(cl, path, seed)
        except BaseException as e:          # noqa: B902 (reported below)
            errs.append(e)

    th = [threading.Thread(target=run, args=(c, D0 + '/two0', 2)),
          threading.Thread(target=run, args=(d, D0 + '/two1', 3))]
    for x in th:
        x.start()
    for x in th:
        x.join(40)
    assert not errs, errs
    assert not any(x.is_alive() for x in th)
    c.close_sync(10)
    d.close_sync(10)
    st = front.stats()
    assert st['batches_lost'] == 0 and st['bad_batches'] == 0
