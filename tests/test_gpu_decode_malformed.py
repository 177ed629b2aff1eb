"""The GPU decoders on wire input the project does not control: the reply
decode (K2-K8, decode_replies_k with expand_strings_k / expand_acl_k and the
fused GET check), the request parse (K12: decode_requests_k, and
parse_request inside the GPU server's tree_serve_k / list_mark_k) and the
ConnectResponse decode (K9) against the Jute oracle (zkmi/jute.py) on
corpora of well-formed frames with one mutation each or none
(tests/malformed_corpus.py): overwritten length words up to 2^31 - 1, cut
and over-long bodies, unknown / aliased / negative xids, unsupported
opcodes.  The accept side of the same kernels is in tests/test_kernels.py.

A frame only the oracle's UTF-8 check refuses is left out (the kernels do
not validate text); each test asserts that share stays under 2 %."""

import struct
import types

import numpy as np
import pytest
import torch

import malformed_corpus as M
from zkmi import consts, jute

pytestmark = pytest.mark.gpu

NODES = (11, 110, 16)         # the fused check's tree: leaves 11..110, 16 B
LIST_OPS = ('GET_CHILDREN', 'GET_CHILDREN2')


def _dev_bytes(b, dev):
    a = np.frombuffer(bytes(b) if b else b'\0', np.uint8).copy()
    return torch.from_numpy(a).to(dev)


def _norm(pkt):
    out = dict(pkt)
    if out.get('stat') is not None:
        out['stat'] = out['stat'].as_tuple()
    return out


def _scan(buf, s, n):
    """K1 over the stream; the frame table must be the host scan's."""
    from zkmi.ops import batch as B
    ft = B.frame_scan(buf, len(s), cap=n)
    want, used, bad = jute.scan_frames(s)
    assert bad < 0 and used == len(s) and len(want) == n
    assert int(ft.count.item()) == n
    assert ft.off.cpu().tolist() == [o for o, _ in want]
    assert ft.length.cpu().tolist() == [ln for _, ln in want]
    return ft


def _leave_out_share(statuses):
    share = M.stats(statuses)
    print('left out (text only): %.2f %%; decoded %.1f %%, rejected %.1f %%'
          % (100 * share[M.SKIP], 100 * share[M.ST_OK],
             100 * (1 - share[M.SKIP] - share[M.ST_OK])))
    assert share[M.SKIP] <= 0.02
    return share


# ---------------------------------------------------------------- replies

@pytest.fixture(scope='module')
def replies(gpu):
    """The reply corpus decoded once: corpus, stream, device buffer, frame
    table, reply table and the oracle's verdict per frame."""
    from zkmi.ops import batch as B
    c = M.ReplyCorpus(nodes=NODES)
    s = c.stream()
    buf = _dev_bytes(s, gpu)
    n = len(c.bodies)
    xt = B.XidTable(bits=M.XID_BITS, device=gpu)
    tab = xt.tab.cpu()
    for slot, ent in c.table():
        tab[slot] = ent
    xt.tab.copy_(tab)
    ft = _scan(buf, s, n)
    rep = B.decode_replies(buf, ft, xt)
    torch.cuda.synchronize()
    want = [c.expect(i) for i in range(n)]
    return types.SimpleNamespace(c=c, s=s, buf=buf, n=n, xt=xt, ft=ft,
                                 rep=rep, want=want)


def _reply_op(c, body):
    """The opcode name a reply body resolves to (None: no header / xid)."""
    if len(body) < 16:
        return None
    xid = struct.unpack_from('>i', body)[0]
    return consts.SPECIAL_XIDS.get(xid) or c.xid_map.get(xid)


def test_reply_corpus_matches_oracle(replies):
    from zkmi.ops import batch as B
    R = replies
    status = R.rep.status[:R.n].cpu().tolist()
    share = _leave_out_share([w[0] for w in R.want])
    for k in (M.ST_OK, M.ST_BAD_DECODE, M.ST_NO_XID, M.ST_BAD_OPCODE):
        assert share[k] > 0, 'no case of status %d' % k
    keep = [i for i, w in enumerate(R.want) if w[0] != M.SKIP]
    for i in keep:
        assert status[i] == R.want[i][0], (i, R.c.kind[i],
                                           R.c.bodies[i].hex())
    # accepted rows: every field, through the library's own host view
    ok = [i for i in keep if R.want[i][0] == M.ST_OK]
    ix = torch.tensor(ok, device=R.buf.device)
    r = R.rep
    sub = B.ReplyBatch(r.xid[ix], r.err[ix], r.opcode[ix], r.status[ix],
                       r.zxid[ix], r.stat64[:, ix], r.stat32[:, ix],
                       r.pay_off[ix], r.pay_len[ix], r.aux0[ix], r.aux1[ix],
                       None)
    got = B.replies_to_packets(R.buf, sub, n=len(ok))
    for i, g in zip(ok, got):
        assert _norm(g) == _norm(R.want[i][1]), (i, R.c.kind[i])
    # the corpus still reaches what it is for: each opcode's reject path,
    # the Stat read where bytes follow it (read_stat, not read_stat_regs),
    # err != OK with anything behind the header, the half-valid list reply
    rejected = {_reply_op(R.c, R.c.bodies[i]) for i in keep
                if R.want[i][0] == M.ST_BAD_DECODE}
    assert rejected >= {'GET_DATA', 'EXISTS', 'SET_DATA', 'CREATE',
                        'GET_CHILDREN', 'GET_CHILDREN2', 'GET_ACL',
                        'NOTIFICATION'}
    trailed = {R.want[i][1]['opcode'] for i in ok
               if R.c.kind[i] == 'trail' and R.want[i][1]['err'] == 'OK'}
    assert trailed >= {'GET_DATA', 'EXISTS', 'SET_DATA', 'GET_CHILDREN2',
                       'GET_ACL', 'CREATE', 'NOTIFICATION'}
    assert any(R.c.kind[i] == 'trail' and R.want[i][1]['err'] != 'OK'
               for i in ok)
    assert any(R.c.kind[i] == 'badop' and R.want[i][1]['err'] != 'OK'
               for i in ok)
    assert {R.c.kind[i] for i in keep if R.want[i][0] == M.ST_NO_XID} == \
        {'absent', 'alias', 'negative'}
    assert sum(M.short_stat_after_names(b, R.c.xid_map)
               for b in R.c.bodies) >= 5


def test_rejected_rows_point_at_nothing(replies):
    """Every rejected row: pay_off -1, pay_len 0, aux0 0, aux1 0 — the
    GET_CHILDREN2 replies with good names and a short Stat included."""
    R = replies
    r = R.rep
    bad = r.status[:R.n] != 0
    assert int(bad.sum().item()) > 1000
    for name, idle in (('pay_off', -1), ('pay_len', 0), ('aux0', 0),
                       ('aux1', 0)):
        col = getattr(r, name)[:R.n][bad]
        rows = torch.nonzero(col != idle).flatten().tolist()
        assert rows == [], (name, rows[:8])
    short = [i for i, b in enumerate(R.c.bodies)
             if M.short_stat_after_names(b, R.c.xid_map)]
    assert short and all(r.status[i].item() == M.ST_BAD_DECODE
                         for i in short)


def test_expand_unmasked_stays_inside_frames(replies):
    """expand_strings / expand_acl over the whole corpus by the rows'
    pay_off / aux0 as decoded (no status mask, as ListPipeline feeds them):
    exactly the oracle's names and ACL entries, each inside its frame."""
    from zkmi.ops import batch as B
    R = replies
    n = R.n
    op = R.rep.opcode[:n]
    zero = torch.zeros_like(R.rep.aux0[:n])
    # (the rows left out of the comparison have no oracle packet)
    known = torch.tensor([w[0] != M.SKIP for w in R.want],
                         device=R.buf.device)
    fo = R.ft.off.cpu().tolist()
    fl = R.ft.length.cpu().tolist()

    def inside(i, off, ln):
        return ln >= 0 and fo[i] + 20 <= off and off + ln <= fo[i] + fl[i]

    ch = torch.where(((op == 8) | (op == 12)) & known, R.rep.aux0[:n], zero)
    base, soff, slen = B.expand_strings(R.buf, R.rep.pay_off[:n], ch)
    lists = {i: w[1]['children'] for i, w in enumerate(R.want)
             if w[0] == M.ST_OK and w[1]['opcode'] in LIST_OPS and
             w[1]['err'] == 'OK'}
    assert soff.numel() == sum(len(v) for v in lists.values()) > 0
    assert ch.cpu().tolist() == [len(lists.get(i, ())) for i in range(n)]
    so, sl, bs = soff.cpu().tolist(), slen.cpu().tolist(), base.cpu().tolist()
    for i, names in lists.items():
        for k, name in enumerate(names):
            j = bs[i] + k
            assert inside(i, so[j], sl[j])
            assert R.s[so[j]:so[j] + sl[j]] == name.encode()

    ac = torch.where((op == 6) & known, R.rep.aux0[:n], zero)
    base, perms, s_o, s_l, i_o, i_l = B.expand_acl(R.buf, R.rep.pay_off[:n],
                                                   ac)
    acls = {i: w[1]['acl'] for i, w in enumerate(R.want)
            if w[0] == M.ST_OK and w[1]['opcode'] == 'GET_ACL' and
            w[1]['err'] == 'OK'}
    assert perms.numel() == sum(len(v) for v in acls.values()) > 0
    assert ac.cpu().tolist() == [len(acls.get(i, ())) for i in range(n)]
    pm, so, sl, io, il, bs = (x.cpu().tolist() for x in
                              (perms, s_o, s_l, i_o, i_l, base))
    for i, acl in acls.items():
        for k, a in enumerate(acl):
            j = bs[i] + k
            assert inside(i, so[j], sl[j]) and inside(i, io[j], il[j])
            assert [p for p, m in consts.PERM_MASKS.items()
                    if pm[j] & m] == a['perms']
            assert R.s[so[j]:so[j] + sl[j]].decode() == a['id']['scheme']
            assert R.s[io[j]:io[j] + il[j]].decode() == a['id']['id']


def test_fused_check_counts_only_clean_gets(replies, gpu):
    """decode_replies(check=...) over the same corpus: acc counts the clean
    GET_DATA successes with the request's xid, the node's czxid and data
    length, as the host counts them from the oracle's packets; no mutated
    row is among them.  The reply table is the unchecked decode's."""
    from zkmi.server.tree import GpuTree
    from zkmi.ops import batch as B
    R = replies
    tree = GpuTree(100, NODES[2], fanout=10, device=gpu)
    assert (tree.leaf0, tree.leaf0 + tree.n_leaves - 1) == NODES[:2]
    dlen = tree.data_len.cpu().tolist()
    want = 0
    for i, (st, pkt) in enumerate(R.want):
        if st == M.ST_OK and pkt['opcode'] == 'GET_DATA' and \
                pkt['err'] == 'OK':
            v = R.c.chk_idx[i]
            hit = pkt['xid'] == R.c.chk_xid[i] and \
                pkt['stat'].czxid == v + 1 and len(pkt['data']) == dlen[v]
            assert hit == (i in set(R.c.chk_rows)), i
            want += hit
    assert want == len(R.c.chk_rows) > 100
    assert all(R.c.kind[i] == '' for i in R.c.chk_rows)
    idx = torch.tensor(R.c.chk_idx, dtype=torch.int64, device=gpu)
    xid = torch.tensor(R.c.chk_xid, dtype=torch.int32, device=gpu)
    for slots in (1, 5):
        acc = torch.zeros(slots, dtype=torch.int64, device=gpu)
        out = B.decode_replies(R.buf, R.ft, R.xt,
                               check=(idx, xid, tree.data_len, acc))
        assert int(acc.sum().item()) == want
        for name in ('xid', 'err', 'opcode', 'status', 'zxid', 'pay_off',
                     'pay_len', 'aux0', 'aux1'):
            assert torch.equal(getattr(out, name)[:R.n],
                               getattr(R.rep, name)[:R.n]), name


# --------------------------------------------------------------- requests

def test_request_corpus_matches_oracle(gpu):
    from zkmi.ops import batch as B
    c = M.RequestCorpus()
    s = c.stream()
    n = len(c.bodies)
    buf = _dev_bytes(s, gpu)
    ft = _scan(buf, s, n)
    rt = B.decode_requests(buf, ft)
    names = ('xid', 'opcode', 'status', 'path_off', 'path_len', 'data_off',
             'data_len', 'arg', 'vec_count', 'rel_zxid')
    cols = {k: getattr(rt, k)[:n].cpu().tolist() for k in names}
    fo = ft.off.cpu().tolist()
    want = [M.expect_request(b) for b in c.bodies]
    share = _leave_out_share([w[0] for w in want])
    for k in (M.ST_OK, M.ST_BAD_DECODE, M.ST_BAD_OPCODE):
        assert share[k] > 0
    for i, (st, f) in enumerate(want):
        if st == M.SKIP:
            continue
        row = {k: cols[k][i] for k in names}
        if st != M.ST_OK:
            assert row['status'] == st, (i, c.kind[i], c.bodies[i].hex())
            continue
        M.check_request_row(c.bodies[i], fo[i], row, f)
    # every mutation kind is there, and each one's verdicts
    verdicts = {}
    for k, w in zip(c.kind, want):
        verdicts.setdefault(k, set()).add(w[0])
    assert verdicts['watch'] == {M.ST_BAD_DECODE}
    assert verdicts['acl'] == {M.ST_OK}          # negative count: empty
    assert verdicts['neglen'] >= {M.ST_OK, M.ST_BAD_DECODE}
    assert verdicts['lists'] == {M.ST_BAD_DECODE}
    assert verdicts['op'] == {M.ST_BAD_OPCODE}
    assert verdicts['tiny'] == {M.ST_BAD_DECODE}
    assert verdicts['word'] >= {M.ST_OK, M.ST_BAD_DECODE}
    assert verdicts['trail'] == {M.ST_OK}
    assert {c.ops[i] for i, w in enumerate(want)
            if w[0] == M.ST_BAD_DECODE and len(c.bodies[i]) >= 8} >= \
        {'GET_DATA', 'EXISTS', 'GET_CHILDREN', 'GET_CHILDREN2', 'CREATE',
         'DELETE', 'SET_DATA', 'GET_ACL', 'SYNC', 'SET_WATCHES'}


# --------------------------------------------------------- ConnectResponse

def test_connect_responses_match_oracle(gpu):
    from zkmi.ops import batch as B
    pw = bytes(range(1, 17))
    full = jute.encode_connect_response(
        {'protocolVersion': 0, 'timeOut': 30000, 'sessionId': 0x123456789ab,
         'passwd': pw})
    assert len(full) == 20 + len(pw)

    def with_len(word, tail=b''):
        return full[:16] + struct.pack('>i', word) + tail
    bodies = [b'', full[:19], full[:20], full[:20 + len(pw) - 1], full,
              full + b'\x01', with_len(-1), with_len(-1, b'\x00'),
              with_len(0), with_len(0x7fffffff), with_len(0x7fffffff, pw),
              with_len(-2**31, pw), with_len(len(pw) + 1, pw)]
    bodies = bodies * 21                  # more than one block (273 rows)
    s = b''.join(jute.frame(b) for b in bodies)
    buf = _dev_bytes(s, gpu)
    ft = _scan(buf, s, len(bodies))
    o = {k: v.cpu().tolist() for k, v in
         B.decode_connect_responses(buf, ft, len(bodies)).items()}
    fo = ft.off.cpu().tolist()
    seen = set()
    for i, b in enumerate(bodies):
        try:
            w = jute.decode_connect_response(b)
        except jute.ZKDecodeError:
            w = None
        seen.add(w is None)
        if w is None:
            assert o['status'][i] == M.ST_BAD_DECODE
            assert o['passwd_off'][i] == -1 and o['passwd_len'][i] == 0
            continue
        assert o['status'][i] == 0
        assert (o['protocolVersion'][i], o['timeOut'][i],
                o['sessionId'][i]) == (w['protocolVersion'], w['timeOut'],
                                       w['sessionId'])
        po, pl = o['passwd_off'][i], o['passwd_len'][i]
        assert fo[i] + 20 == po and po + pl <= fo[i] + len(b)
        assert s[po:po + pl] == w['passwd']
    assert seen == {True, False}


# ------------------------------------------- the server, bad frames inside

NOPE = {'opcode': 'GET_DATA', 'path': '/nope', 'watch': False}


def _leaf(i):
    return '/bench/d%06d/n%09d' % (i // 100, i)


def _fixed_clock(monkeypatch):
    """Both replicas stamp the same mtime / ctime."""
    import time
    from zkmi.server import engine as S
    monkeypatch.setattr(S, 'time', types.SimpleNamespace(
        time=lambda: 1.7e9, perf_counter=time.perf_counter,
        sleep=time.sleep))


def _replica(gpu, **kw):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(4000, 16, fanout=100, device=gpu, spare=1.0,
                   ctime_ms=1600000000000, **kw)
    return tree, GpuServer(tree, 1024, 1 << 20, window=256)


def _create(flags):
    return jute.encode_request(
        {'xid': 77, 'opcode': 'CREATE', 'path': '/bench/d000002/s',
         'data': b'abcdefgh' * 6, 'acl': jute.DEFAULT_ACL, 'flags': flags})


_SEQ_CREATE = _create(['SEQUENTIAL'])
_PLAIN_CREATE = _create([])


def _bad_acl(create):
    """The create with its ACL's scheme length word set to 2^31 - 1."""
    at = 12 + len('/bench/d000002/s') + 4 + 48 + 4 + 4
    assert create[at:at + 4] == struct.pack('>i', 5)              # 'world'
    return create[:at] + struct.pack('>i', 0x7fffffff) + create[at + 4:]


def _bad_bodies(n, seed=5):
    """n request bodies the oracle refuses, of every kind in the request
    corpus, then the two length words that overflowed 32-bit sums in the
    kernels: a SEQUENTIAL create whose path length is 2^31 - 1 (seq_parent /
    seq_key: `12 + pl + 12`) and a create whose ACL scheme length is
    (skip_strings: `4 + l`)."""
    c = M.RequestCorpus(seed=seed, n=1500)
    by_kind = {}
    for k, b in zip(c.kind, c.bodies):
        if M.expect_request(b)[0] in (M.ST_BAD_DECODE, M.ST_BAD_OPCODE):
            by_kind.setdefault(k, []).append(b)
    assert set(by_kind) >= {'cut', 'word', 'op', 'tiny', 'watch', 'neglen',
                            'lists'}
    big = struct.pack('>i', 0x7fffffff)
    out = [_SEQ_CREATE[:8] + big + _SEQ_CREATE[12:],
           _bad_acl(_PLAIN_CREATE)]
    for b in out:
        assert len(b) >= 64 and M.expect_request(b)[0] == M.ST_BAD_DECODE
    kinds = sorted(by_kind)
    k = 0
    while len(out) < n:
        pool = by_kind[kinds[k % len(kinds)]]
        out.append(pool[(k // len(kinds)) % len(pool)])
        k += 1
    return out


def _serve_bodies(srv, bodies, gpu, call='serve', **kw):
    s = b''.join(jute.frame(b) for b in bodies)
    out, total, err, ft = getattr(srv, call)(_dev_bytes(s, gpu), len(s),
                                             **kw)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    raw = bytes(out[:int(total.item())].cpu().numpy().tobytes())
    frames, used, bad = jute.scan_frames(raw)
    assert bad < 0 and used == len(raw)
    assert len(frames) == len(bodies)          # one reply a frame
    return [raw[o:o + ln] for o, ln in frames]


def _assert_refused(reply, body):
    """A header-only BAD_ARGUMENTS reply echoing the request's xid (0 when
    the body is too short to hold one)."""
    assert len(reply) == 16
    xid, _, err = struct.unpack('>iqi', reply)
    assert err == consts.ERR_CODES['BAD_ARGUMENTS']
    assert xid == (struct.unpack_from('>i', body)[0] if len(body) >= 8
                   else 0)


def _mixed_batch(ordered):
    """~600 well-formed requests on distinct paths; ``ordered``: also
    chains on one path each (set, get, set / create, get, delete)."""
    pk = []
    for i in range(600):
        x = 1000 + i
        p = _leaf(i)
        kind = i % 5
        if kind == 0:
            pk.append({'xid': x, 'opcode': 'GET_DATA', 'path': p,
                       'watch': False})
        elif kind == 1:
            pk.append({'xid': x, 'opcode': 'EXISTS', 'path': p,
                       'watch': False})
        elif kind == 2:
            pk.append({'xid': x, 'opcode': 'SET_DATA', 'path': p,
                       'data': b'v%05d' % i, 'version': -1})
        elif kind == 3:
            pk.append({'xid': x, 'opcode': 'CREATE',
                       'path': '/bench/d%06d/new%05d' % (i % 7, i),
                       'data': b'c%05d' % i, 'acl': jute.DEFAULT_ACL,
                       'flags': []})
        else:
            pk.append({'xid': x, 'opcode': 'DELETE', 'path': p,
                       'version': -1})
    if ordered:
        for j, at in enumerate(range(20, 600, 40)):
            p = _leaf(2000 + j)
            new = '/bench/d000030/chain%03d' % j
            x = 5000 + 10 * j
            pk[at:at] = [
                {'xid': x, 'opcode': 'SET_DATA', 'path': p, 'data': b'one',
                 'version': -1},
                {'xid': x + 1, 'opcode': 'GET_DATA', 'path': p,
                 'watch': False},
                {'xid': x + 2, 'opcode': 'SET_DATA', 'path': p,
                 'data': b'three', 'version': 1},
                {'xid': x + 3, 'opcode': 'CREATE', 'path': new,
                 'data': b'n', 'acl': jute.DEFAULT_ACL, 'flags': []},
                {'xid': x + 4, 'opcode': 'GET_DATA', 'path': new,
                 'watch': False},
                {'xid': x + 5, 'opcode': 'DELETE', 'path': new,
                 'version': -1}]
    return pk


@pytest.mark.parametrize('ordered', [False, True])
def test_serve_with_bad_frames_in_the_batch(gpu, monkeypatch, ordered):
    """Replica A serves a batch with ~60 malformed frames scattered in it
    (first, last, across the 256 boundary, inside the same-path chains);
    replica B the same batch with each of them replaced by GET_DATA '/nope'
    at the same index, so every write keeps its zxid.  A answers each bad
    frame BAD_ARGUMENTS and everything else exactly as B does, and the two
    trees end up equal."""
    _fixed_clock(monkeypatch)
    kw = {'scratch': 1 << 20} if ordered else {}
    tree_a, srv_a = _replica(gpu, **kw)
    tree_b, srv_b = _replica(gpu, **kw)
    assert tree_a.digest() == tree_b.digest()
    good = [jute.encode_request(p) for p in _mixed_batch(ordered)]
    n = len(good) + 60
    r = np.random.default_rng(9)
    at = {0, n - 1, 255, 256, 257}
    if ordered:
        at |= {22, 25, 63}                # inside two of the chains
    while len(at) < 60:
        at.add(int(r.integers(1, n - 1)))
    at = sorted(at)
    bad = _bad_bodies(len(at))
    a_bodies, b_bodies, it = [], [], iter(good)
    for i in range(n):
        if i in at:
            body = bad[at.index(i)]
            a_bodies.append(body)
            b_bodies.append(jute.encode_request(dict(NOPE, xid=9000 + i)))
        else:
            body = next(it)
            a_bodies.append(body)
            b_bodies.append(body)
    assert any(len(a_bodies[i]) < 8 for i in at)
    skw = {'ordered': True, 'passes': 4} if ordered else {}
    rep_a = _serve_bodies(srv_a, a_bodies, gpu, **skw)
    rep_b = _serve_bodies(srv_b, b_bodies, gpu, **skw)
    for i in range(n):
        if i in at:
            _assert_refused(rep_a[i], a_bodies[i])
            xid, _, err = struct.unpack_from('>iqi', rep_b[i])
            assert (xid, err) == (9000 + i, consts.ERR_CODES['NO_NODE'])
        else:
            assert rep_a[i] == rep_b[i], i
    # the batch did something: the writes took, in both
    errs = [struct.unpack_from('>i', x, 12)[0] for x in rep_b]
    assert sum(e == 0 for e in errs) > 0.85 * len(good)
    assert tree_a.digest() == tree_b.digest()
    if ordered:
        for srv in (srv_a, srv_b):
            assert srv.order_stats()[0] < 4         # nothing refused


def test_refused_sequential_create_counts_as_a_failed_one(gpu, monkeypatch):
    """The numbering pass reads a frame's op, path and flags only, so a
    SEQUENTIAL create under an existing parent whose ACL is malformed is
    numbered before the full parse refuses it.  It is answered
    BAD_ARGUMENTS and leaves what any failed SEQUENTIAL create leaves (here
    the same create with an empty ACL, INVALID_ACL): no child, and its
    number as a gap in the parent's cversion."""
    _fixed_clock(monkeypatch)
    tree_a, srv_a = _replica(gpu)
    tree_b, srv_b = _replica(gpu)
    ok = jute.encode_request(
        {'xid': 5, 'opcode': 'CREATE', 'path': '/bench/d000002/s',
         'data': b'x', 'acl': jute.DEFAULT_ACL, 'flags': ['SEQUENTIAL']})
    no_acl = jute.encode_request(
        {'xid': 77, 'opcode': 'CREATE', 'path': '/bench/d000002/s',
         'data': b'abcdefgh' * 6, 'acl': [], 'flags': ['SEQUENTIAL']})
    bad = _bad_acl(_SEQ_CREATE)
    assert M.expect_request(bad)[0] == M.ST_BAD_DECODE
    rep_a = _serve_bodies(srv_a, [ok, bad, ok], gpu)
    rep_b = _serve_bodies(srv_b, [ok, no_acl, ok], gpu)
    _assert_refused(rep_a[1], bad)
    assert struct.unpack_from('>i', rep_b[1], 12)[0] == \
        consts.ERR_CODES['INVALID_ACL']
    assert rep_a[0] == rep_b[0] and rep_a[2] == rep_b[2]
    made = [jute.decode_response(x, {5: 'CREATE'})['path']
            for x in (rep_a[0], rep_a[2])]
    assert [m[:-10] for m in made] == ['/bench/d000002/s'] * 2
    assert int(made[1][-10:]) - int(made[0][-10:]) == 2       # the gap
    assert tree_a.digest() == tree_b.digest()


def test_serve_list_with_bad_frames_in_the_batch(gpu, monkeypatch):
    """The list path: malformed frames among GET_CHILDREN2 requests are
    answered BAD_ARGUMENTS, the others as without them, and a rejected
    frame arms no child watch (its watch byte never counts)."""
    _fixed_clock(monkeypatch)
    tree_a, srv_a = _replica(gpu, watch_cap=256)
    tree_b, srv_b = _replica(gpu, watch_cap=256)
    dirs = ['/bench/d%06d' % d for d in range(40)]

    def ls(x, d, watch=False, op='GET_CHILDREN2'):
        return jute.encode_request({'xid': x, 'opcode': op, 'path': d,
                                    'watch': watch})
    a_bodies, b_bodies, at = [], [], []
    for i in range(300):
        d = dirs[i % 40]
        good = ls(100 + i, d, watch=(d == dirs[0]),
                  op=LIST_OPS[i % 2])
        nope = ls(9000 + i, '/nope', op='GET_CHILDREN')
        kind = {0: 'tiny', 7: 'watch2', 8: 'cut', 255: 'cut', 256: 'watchff',
                299: 'word'}.get(i) or ('watch2' if i % 23 == 5 else None)
        if kind is None:
            a_bodies.append(good)
            b_bodies.append(good)
            continue
        w = ls(100 + i, dirs[1 + i % 3], watch=True)  # would arm d1..d3
        body = {'tiny': w[:5], 'watch2': w[:-1] + b'\x02',
                'watchff': w[:-1] + b'\xff', 'cut': w[:-1],
                'word': w[:8] + struct.pack('>i', 0x7fffffff) + w[12:]}[kind]
        assert M.expect_request(body)[0] == M.ST_BAD_DECODE
        at.append(i)
        a_bodies.append(body)
        b_bodies.append(nope)
    rep_a = _serve_bodies(srv_a, a_bodies, gpu, call='serve_list', wslot=3)
    rep_b = _serve_bodies(srv_b, b_bodies, gpu, call='serve_list', wslot=3)
    xmap = {100 + i: LIST_OPS[i % 2] for i in range(300)}
    for i in range(300):
        if i in at:
            _assert_refused(rep_a[i], a_bodies[i])
            continue
        # (the order of the names inside a reply is unspecified)
        pa, pb = (jute.decode_response(x[i], xmap) for x in (rep_a, rep_b))
        assert len(rep_a[i]) == len(rep_b[i]) and pa['err'] == 'OK'
        assert len(pa['children']) == 100
        pa['children'].sort()
        pb['children'].sort()
        assert _norm(pa) == _norm(pb)
    assert tree_a.digest() == tree_b.digest()
    # only d0 was armed: a create under d1..d3 notifies nobody

    def create(x, path):
        return jute.encode_request({'xid': x, 'opcode': 'CREATE',
                                    'path': path, 'data': b'',
                                    'acl': jute.DEFAULT_ACL, 'flags': []})
    reps = _serve_bodies(srv_a, [create(1, dirs[k] + '/kid')
                                 for k in (1, 2, 3, 0)], gpu)
    assert [struct.unpack_from('>i', x, 12)[0] for x in reps] == [0] * 4
    buf, total, slots, count = srv_a.notif
    assert int(count.item()) == 1
    raw = bytes(buf[:int(total.item())].cpu().numpy().tobytes())
    (o, ln), = jute.scan_frames(raw)[0]
    note = jute.decode_response(raw[o:o + ln], {})
    assert (slots[0].item(), note['type'], note['path']) == \
        (3, 'CHILDREN_CHANGED', dirs[0])


@pytest.mark.parametrize('plen', [0, 1, 255, 256, 4096, 70000])
def test_path_lengths(gpu, plen):
    """Well-formed requests whose path is 0 .. 70 000 bytes long (the packed
    path word of zk_tree.h keeps 24 bits of length, 16 MiB, the frame cap):
    GET_DATA and EXISTS answer NO_NODE; a CREATE either succeeds and reads
    back, path and data, or fails and leaves the tree as it was."""
    tree, srv = _replica(gpu)
    path = ('/' + 'x' * (plen - 1)) if plen else ''
    assert len(path) == plen
    xmap = {1: 'GET_DATA', 2: 'EXISTS', 3: 'CREATE'}
    reads = [jute.encode_request({'xid': 1, 'opcode': 'GET_DATA',
                                  'path': path, 'watch': False}),
             jute.encode_request({'xid': 2, 'opcode': 'EXISTS',
                                  'path': path, 'watch': False})]
    got = [jute.decode_response(x, xmap)
           for x in _serve_bodies(srv, reads, gpu)]
    assert [(g['xid'], g['err']) for g in got] == [(1, 'NO_NODE'),
                                                   (2, 'NO_NODE')]
    before = tree.digest()
    rep, = _serve_bodies(srv, [jute.encode_request(
        {'xid': 3, 'opcode': 'CREATE', 'path': path, 'data': b'payload',
         'acl': jute.DEFAULT_ACL, 'flags': []})], gpu)
    made = jute.decode_response(rep, xmap)
    if made['err'] != 'OK':
        assert tree.digest() == before
        return
    assert made['path'] == path
    assert tree.digest()[1] == before[1] + 1          # one more live node
    got = [jute.decode_response(x, xmap)
           for x in _serve_bodies(srv, reads, gpu)]
    assert [g['err'] for g in got] == ['OK', 'OK']
    assert got[0]['data'] == b'payload'
    assert got[0]['stat'].dataLength == 7 and got[1]['stat'] == got[0]['stat']
