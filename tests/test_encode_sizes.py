"""The batch encoders (csrc/kernels/encode.hip: K9 connect requests, K10
requests, K11 SET_WATCHES, K13 replies) against the pure-Python Jute oracle
(zkmi/jute.py) at the sizes their branches turn on: data from 0 bytes to
1 MB (tests/sizeladder.py), paths from 1 to 1000 bytes, every start residue
mod 16, records that fill the 28 KiB LDS image exactly and records larger
than it at every place of a 256-record block.  All comparisons are exact."""

import random

import numpy as np
import pytest
import torch

from sizeladder import (BIG, ENC_T, PATH_LENS, REQ_REG_PATH, STAGE_BYTES,
                        create_ladder, ladder, ladder_tree, rand_bytes,
                        rand_path, staged_runs)

from zkmi import consts, jute
from zkmi.ops import _lib

pytestmark = pytest.mark.gpu

CANARY = 0xAB


def _dev_bytes(b, dev):
    a = np.frombuffer(bytes(b) if b else b'\0', np.uint8).copy()
    return torch.from_numpy(a).to(dev)


def _frames(pk):
    return [jute.frame(jute.encode_request(p)) for p in pk]


def _starts(frames):
    out, o = [], 0
    for f in frames:
        out.append(o)
        o += len(f)
    return out, o


def _check_requests(gpu, pk, terminate=False):
    """Encode ``pk`` with K10 into a canary-filled buffer and compare the
    stream, the record offsets, the total, the error word, the terminator,
    the bytes past the stream's last 16-byte chunk, the xid table and the
    presized entry point with the oracle.  Returns (starts, sizes)."""
    from zkmi.ops import batch as B
    for i, p in enumerate(pk):
        p['xid'] = i + 1
    frames = _frames(pk)
    want = b''.join(frames)
    starts, t = _starts(frames)
    sizes = [len(f) for f in frames]
    rb = B.pack_requests(pk, gpu)
    cap = t + 256
    xt = B.XidTable(bits=12, device=gpu)
    buf = torch.full((cap,), CANARY, dtype=torch.uint8, device=gpu)
    out, rec_off, total, err = B.encode_requests(rb, xt, out=buf,
                                                 terminate=terminate)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    assert int(total.item()) == t
    hb = out.cpu().numpy().tobytes()
    if hb[:t] != want:
        bad = next(i for i in range(t) if hb[i] != want[i])
        rec = max(k for k, s in enumerate(starts) if s <= bad)
        raise AssertionError(
            'stream differs at byte %d: record %d (%s, path %d B, data %d B) '
            'at offset %d, byte %d of %d' % (
                bad, rec, pk[rec]['opcode'], len(pk[rec].get('path', '')),
                len(pk[rec].get('data', b'') or b''), starts[rec],
                bad - starts[rec], sizes[rec]))
    assert rec_off.cpu().tolist() == starts
    end = t
    if terminate:
        assert hb[t:t + 4] == b'\xff' * 4
        end = t + 4
    # whole 16-byte chunks are stored: nothing past the last one
    end = (end + 15) & ~15
    assert hb[end:] == bytes([CANARY]) * (cap - end)
    tab =xt.tab.cpu().tolist()
    for p in pk:
        e = tab[p['xid'] & xt.mask]
        assert (e >> 32) == p['xid']
        assert (e & 0xffffffff) == consts.OP_CODES[p['opcode']]
    # the presized entry point: sizes and block sums from the host
    sz = torch.tensor(sizes, dtype=torch.int64, device=gpu)
    nb = (len(pk) + ENC_T - 1) // ENC_T
    bs = torch.tensor([sum(sizes[k * ENC_T:(k + 1) * ENC_T])
                       for k in range(nb)], dtype=torch.int64, device=gpu)
    buf2 = torch.full((cap,), CANARY, dtype=torch.uint8, device=gpu)
    out2, off2, tot2, err2 = B.encode_requests(rb, out=buf2,
                                               terminate=terminate,
                                               presized=(sz, bs))
    assert int(err2.item()) == 0 and int(tot2.item()) == t
    assert torch.equal(off2, rec_off)
    assert torch.equal(out2, out)
    return starts, sizes


def _req(rng, op, pl, dl=0):
    if op == 'PING':
        return {'opcode': 'PING'}
    path = rand_path(rng, pl)
    if op == 'CREATE':
        return {'opcode': op, 'path': path, 'data': rand_bytes(rng, dl),
                'acl': jute.DEFAULT_ACL,
                'flags': rng.choice([[], ['EPHEMERAL'], ['SEQUENTIAL']])}
    if op == 'SET_DATA':
        return {'opcode': op, 'path': path, 'data': rand_bytes(rng, dl),
                'version': rng.randint(-1, 1 << 20)}
    if op == 'DELETE':
        return {'opcode': op, 'path': path,
                'version': rng.randint(-1, 1 << 20)}
    if op in ('GET_DATA', 'EXISTS', 'GET_CHILDREN2'):
        return {'opcode': op, 'path': path, 'watch': rng.random() < 0.5}
    assert op in ('GET_ACL', 'SYNC')
    return {'opcode': op, 'path': path}


PATH_OPS = ('GET_DATA', 'EXISTS', 'GET_CHILDREN2', 'GET_ACL', 'SYNC',
            'DELETE')


def _ladder_batch(rng, lead, sizes):
    """A SYNC of ``lead`` path bytes (the start residue), then in random
    order a CREATE or SET_DATA per data length of ``sizes`` (paths cycling
    through PATH_LENS), every pathed op at every path length, and PINGs."""
    pk = []
    for k, dl in enumerate(sizes):
        pk.append(_req(rng, ('CREATE', 'SET_DATA')[(k + lead) & 1],
                       PATH_LENS[(k + lead) % len(PATH_LENS)], dl))
    for pl in PATH_LENS:
        for op in PATH_OPS:
            pk.append(_req(rng, op, pl))
    pk += [_req(rng, 'PING', 0) for _ in range(5)]
    rng.shuffle(pk)
    return [_req(rng, 'SYNC', lead)] + pk


@pytest.mark.parametrize('lead', range(1, 17))
def test_encode_requests_ladder(gpu, lead):
    """K10 on the whole ladder of data lengths and path lengths, led by a
    SYNC whose path length sets the stream's start residue; the two batches
    led by 1 and by 16 path bytes carry the 1 000 000-byte record too.
    Asserted through the host mirror of staged_emit: some records took the
    ``k == 0`` branch, and the read requests lie on both sides of the
    register path's bound."""
    rng = random.Random(1000 + lead)
    pk = _ladder_batch(rng, lead, ladder(big=lead in (1, 16)))
    starts, sizes = _check_requests(gpu, pk, terminate=bool(lead & 1))
    assert starts[1] & 15 == lead & 15
    runs, direct = staged_runs(starts, sizes)
    assert direct and runs
    for i in direct:
        assert pk[i]['opcode'] in ('CREATE', 'SET_DATA')
        assert len(pk[i]['data']) > STAGE_BYTES - 1100
    reads = {len(p['path']) <= REQ_REG_PATH for p in pk
             if p['opcode'] in ('GET_DATA', 'EXISTS', 'GET_CHILDREN2')}
    assert reads == {False, True}


def _small(rng, n):
    return [_req(rng, rng.choice(PATH_OPS), rng.choice(PATH_LENS[:11]))
            for _ in range(n)]


def _over(rng, extra=1):
    """A SET_DATA larger than the image wherever it starts."""
    return _req(rng, 'SET_DATA', 2, STAGE_BYTES + extra)


def test_encode_requests_exact_fill_and_one_more(gpu):
    """A SET_DATA of '/a' at stream offset 0 with 28 630 data bytes fills
    the LDS image exactly (frame 28 656 bytes + the 16 of slack =
    STAGE_BYTES); the record after it starts 16-byte aligned and is one byte
    longer: the ``k == 0`` branch.  Then both again at every start residue
    (a leading SYNC), the exact fill recomputed for the residue."""
    rng = random.Random(5)
    a = {'opcode': 'SET_DATA', 'path': '/a', 'data': rand_bytes(rng, 28630),
         'version': 3}
    b = {'opcode': 'SET_DATA', 'path': '/a', 'data': rand_bytes(rng, 28631),
         'version': 4}
    pk = [a, b] + _small(rng, 5)
    starts, sizes = _check_requests(gpu, pk)
    runs, direct = staged_runs(starts, sizes)
    assert runs[0] == (0, 1, 0) and direct == [1]
    for lead in range(1, 17):
        sync = _req(rng, 'SYNC', lead)
        head = 16 + lead                       # the SYNC's frame
        # the second record's end fills the image: head + 26 + dl + 16 (the
        # run starts at stream offset 0, a0 = 0)
        dl = STAGE_BYTES - 16 - 26 - head
        pk = [sync,
              {'opcode': 'SET_DATA', 'path': '/a',
               'data': rand_bytes(rng, dl), 'version': -1},
              {'opcode': 'SET_DATA', 'path': '/b',
               'data': rand_bytes(rng, dl + 1), 'version': -1},
              {'opcode': 'SET_DATA', 'path': '/c',
               'data': rand_bytes(rng, STAGE_BYTES), 'version': -1}] + \
            _small(rng, 3)
        starts, sizes = _check_requests(gpu, pk, terminate=True)
        runs, direct = staged_runs(starts, sizes)
        assert runs[0] == (0, 2, 0), (lead, runs)
        assert 3 in direct


def test_encode_requests_over_image_placements(gpu):
    """Records larger than the image first, in the middle and last in
    their 256-record block, two of them adjacent, and one as the last
    record of a terminated batch: each placement asserted through the host
    mirror of staged_emit's ``fits`` rule."""
    rng = random.Random(6)
    pk = [_over(rng)] + _small(rng, 99) + [_over(rng, 7)] + \
        _small(rng, 50) + [_over(rng, 16), _over(rng, 33)] + \
        _small(rng, ENC_T - 154) + [_over(rng, 2)]
    assert len(pk) == ENC_T
    # the second block: small ones, then an over-image record the batch's
    # last
    pk += _small(rng, 40) + [_over(rng, 5)]
    starts, sizes = _check_requests(gpu, pk, terminate=True)
    runs, direct = staged_runs(starts, sizes)
    assert direct == [0, 100, 151, 152, ENC_T - 1, len(pk) - 1]
    # not terminated, the over-image record the first of the second block
    pk = _small(rng, ENC_T) + [_over(rng)] + _small(rng, 3)
    starts, sizes = _check_requests(gpu, pk)
    assert staged_runs(starts, sizes)[1] == [ENC_T]


# ---- K11 --------------------------------------------------------------------

def _sw_paths(rng, n):
    """``n`` paths: the empty string and a 1000-byte one among them."""
    out = [rand_path(rng, rng.choice((1, 2, 3, 4, 5, 15, 16, 17, 40)))
           for _ in range(n)]
    if n >= 1:
        out[rng.randrange(n)] = ''
    if n >= 2:
        out[0 if out[0] != '' else 1] = rand_path(rng, 1000)
    return out


@pytest.mark.parametrize('count', [1, 255, 256, 257, 5000])
def test_encode_set_watches_sizes(gpu, count):
    """K11 with ``count`` paths a list, in every combination of empty and
    non-empty lists, an empty string (wire length -1) and a 1000-byte path
    in each non-empty list."""
    from zkmi.ops import batch as B
    rng = random.Random(count)
    for mask in range(8):
        lists = [_sw_paths(rng, count) if mask >> k & 1 else []
                 for k in range(3)]
        got = B.encode_set_watches(0x1234567 + mask, lists[0], lists[1],
                                   lists[2], gpu)
        want = jute.frame(jute.encode_request(
            {'xid': -8, 'opcode': 'SET_WATCHES', 'relZxid': 0x1234567 + mask,
             'events': {'dataChanged': lists[0],
                        'createdOrDestroyed': lists[1],
                        'childrenChanged': lists[2]}}))
        assert bytes(got.cpu().numpy().tobytes()) == want, (count, mask)


# ---- K9 ---------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 256, 257, 3000])
def test_encode_connect_requests_sizes(gpu, n):
    """K9 with ``n`` records and passwords of 0, 1, 15, 16 and 17 bytes."""
    from zkmi.ops import batch as B
    rng = random.Random(n)
    lens = (0, 1, 15, 16, 17)
    reqs = [{'protocolVersion': rng.randint(0, 3),
             'lastZxidSeen': rng.getrandbits(50),
             'timeOut': rng.randint(1, 1 << 20),
             'sessionId': rng.getrandbits(62),
             'passwd': rand_bytes(rng, lens[(i + n) % 5])} for i in range(n)]
    got = B.encode_connect_requests(reqs, gpu)
    want = b''.join(jute.frame(jute.encode_connect_request(r)) for r in reqs)
    assert bytes(got.cpu().numpy().tobytes()) == want


# ---- K13 by node index ------------------------------------------------------

@pytest.fixture(scope='module')
def ladder_nodes(gpu):
    """The ladder as znodes of a tree: (model, {size: path})."""
    m = ladder_tree(gpu)
    return m, create_ladder(m, ladder(big=True))


def _slot_stat(tree, v):
    off = int(tree.slot_off[v].item())
    raw = bytes(tree.slab[off:off + 68].cpu().numpy().tobytes())
    return jute.JuteReader(raw, 0).read_stat()


@pytest.mark.parametrize('lead', [0, 5, 11])
def test_encode_responses_by_node_ladder(gpu, ladder_nodes, lead):
    """K13 without ``presized`` and without slot offsets (the ``r.node``
    path, where the serve passes ``r.slot``): GET_DATA / EXISTS / SET_DATA
    replies of the ladder's znodes, CREATE and NOTIFICATION replies with
    the path ladder between them, errors among them, against
    jute.encode_response; the terminator and the canary past it as
    test_encode_responses_serve_mix_matches_oracle checks them.  ``lead``
    NOTIFICATIONs of odd sizes move the start residues; the 1 000 000-byte
    znode is in the first case only."""
    from zkmi.ops import batch as B
    m, paths = ladder_nodes
    tree = m.tree
    rng = random.Random(40 + lead)
    sizes = [dl for dl in sorted(paths) if dl != BIG or lead == 0]
    recs = []
    for k in range(lead):
        recs.append(('NOTIFICATION', 0, None, rand_path(rng, 1 + 3 * k)))
    for k, dl in enumerate(sizes):
        recs.append(('GET_DATA', 0 if rng.random() < 0.95 else -101, dl, ''))
        if k % 4 == 0:
            recs.append((rng.choice(['EXISTS', 'SET_DATA', 'DELETE']),
                         0 if rng.random() < 0.8 else -101, dl, ''))
        if k % 5 == 0:
            pl = PATH_LENS[(k // 5) % len(PATH_LENS)]
            recs.append((rng.choice(['CREATE', 'NOTIFICATION']), 0, None,
                         rand_path(rng, pl)))
    n = len(recs)
    assert n > ENC_T
    stats = {dl: _slot_stat(tree, m.node_of[paths[dl]]) for dl in sizes}
    parena = b''.join(r[3].encode() for r in recs)
    poff = np.cumsum([0] + [len(r[3]) for r in recs[:-1]])
    zx = [rng.randint(0, 2 ** 40) for _ in range(n)]
    aux = [rng.choice([1, 2, 3, 4]) for _ in range(n)]
    T = lambda a, dt: torch.tensor(a, dtype=dt, device=gpu)  # noqa: E731
    resp = B.ResponseBatch(
        T([consts.OP_CODES[r[0]] for r in recs], torch.int32),
        T(list(range(n)), torch.int32), T([r[1] for r in recs], torch.int32),
        T([m.node_of[paths[r[2]]] if r[2] is not None else 0 for r in recs],
          torch.int64), T(zx, torch.int64), T(poff.tolist(), torch.int64),
        T([len(r[3]) for r in recs], torch.int32), _dev_bytes(parena, gpu),
        T(aux, torch.int32), T([n], torch.int64))
    want = []
    for i, (op, err, dl, path) in enumerate(recs):
        rep = {'xid': i, 'zxid': zx[i], 'err': err, 'opcode': op,
               'path': path, 'type': aux[i], 'state': 'SYNC_CONNECTED'}
        if dl is not None:
            rep['stat'] = stats[dl]
            rep['data'] = bytes(m.db.nodes[paths[dl]].data or b'')
            assert len(rep['data']) == dl == stats[dl].dataLength
        want.append(jute.frame(jute.encode_response(rep)))
    starts, t = _starts(want)
    want = b''.join(want)
    cap = t + 256
    out = torch.full((cap,), CANARY, dtype=torch.uint8, device=gpu)
    out, rec_off, total, err = B.encode_responses(resp, tree.store, cap,
                                                  out=out, terminate=True)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    assert int(total.item()) == t
    hb = out.cpu().numpy().tobytes()
    if hb[:t] != want:
        bad = next(i for i in range(t) if hb[i] != want[i])
        rec = max(k for k, s in enumerate(starts) if s <= bad)
        raise AssertionError('stream differs at byte %d: reply %d %r at '
                             'offset %d, byte %d' % (
                                 bad, rec, recs[rec][:3], starts[rec],
                                 bad - starts[rec]))
    assert hb[t:t + 4] == b'\xff' * 4
    end = (t + 4 + 15) & ~15
    assert hb[end:] == bytes([CANARY]) * (cap - end)
    assert rec_off[:n].cpu().tolist() == starts
    assert _lib.SLOT_STAT == 0
