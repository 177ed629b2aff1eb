"""The read-only tiles serve stages each wave's request frames in LDS
(csrc/kernels/zk_frame_rows.h fr_span_load / fr_span_store; tree.hip
tree_serve_tiles_k<true>): a wave whose 64 frames, with the span's
misalignment from 16 bytes, fit a SRV_STAGE-byte image copies them with
coalesced loads and parses, hashes and compares the path there; any other
wave reads global memory as the plain serve does.  The tests: full,
short-by-one and over-by-one waves and blocks, spans at, one byte over and
far over the image, long paths, streams that end inside a wave, malformed
frames, and the same stream at odd byte offsets of its buffer with two
different fills around it.  The reply side (the tiles decoder, which is not
staged: measured and rejected, profiles/stage_frames_ab.log) runs the same
shapes.

Differential, in the manner of tests/test_fused_rows.py (whose helpers this
file uses): the same stream through (a) the three-launch scan and the plain
consumers, (b) the deferred scan and the tiles consumers.  Everything either
path writes must be equal — reply columns, Stats, frame table rows, the
fused check's count, the serve's reply tables and the encoded reply stream —
and where it is cheap the rows are compared with zkmi/jute.py as well.
Every stream is longer than one 4 KiB tile, or the tiles path is not taken."""

import numpy as np
import pytest
import torch

import malformed_corpus as M
import test_fused_rows as FR
from zkmi import jute
from zkmi.ops import batch as B

pytestmark = pytest.mark.gpu

SRV_STAGE = 4096              # csrc/kernels/tree.hip: a wave's image
# a wave and a block full, short by one and over by one
COUNTS = (22, 63, 64, 65, 255, 256, 257, 600)
XID0 = 0x1000
XID_BITS = 12                 # 4096 slots > the largest stream here


def _be(rec, col, v, w):
    for b in range(w):
        rec[:, col + b] = (v >> (8 * (w - 1 - b))) & 0xff


def _get_replies(rng, dls):
    """GET_DATA replies, frame i = request i: xid XID0 + i, node idx i (czxid
    i + 1), dls[i] data bytes.  Returns the stream (numpy bytes) and the
    frame starts."""
    dls = np.asarray(dls, np.int64)
    n = len(dls)
    lens = 16 + 4 + dls + 68
    buf, starts = FR._stream(rng, lens)
    i = np.arange(n, dtype=np.int64)
    for col, v, w in ((4, XID0 + i, 4), (8, 0x5000 + i, 8), (16, 0 * i, 4),
                      (20, dls, 4)):
        for b in range(w):
            buf[starts + col + b] = (v >> (8 * (w - 1 - b))) & 0xff
    st = starts + 24 + dls                       # the Stat: czxid = i + 1
    for b in range(8):
        buf[st + b] = ((i + 1) >> (8 * (7 - b))) & 0xff
    return buf, starts


@pytest.fixture(scope='module')
def xt(gpu):
    """xid XID0 + i -> GET_DATA for i < 4096."""
    t = B.XidTable(bits=XID_BITS, device=gpu)
    x = np.arange(XID0, XID0 + (1 << XID_BITS), dtype=np.int64)
    tab = np.empty(1 << XID_BITS, np.int64)
    tab[x & t.mask] = (x << 32) | 4
    t.tab.copy_(torch.from_numpy(tab))
    return t


def _both(gpu, xt, d, n, cap, dlen=None, window=512, sent=None):
    """The plain and the tiles decode of ``d[:n]`` (device bytes), with the
    fused check when ``dlen`` (the per-node data lengths) is given, against
    the requests ``sent`` = (idx, xid) (default: node i, xid XID0 + i).
    Returns
    everything the tiles path wrote, on the host, after comparing it with
    the plain path's."""
    outs = []
    for tiles in (False, True):
        sc = B.FrameScanner(cap, gpu, window=window)
        ft = sc.scan(d, n, rows=not tiles)
        assert (sc.pending is not None) == tiles
        chk, acc = None, None
        if dlen is not None:
            acc = torch.zeros(3, dtype=torch.int64, device=gpu)
            idx, xid = sent if sent is not None else (
                torch.arange(cap, dtype=torch.int64, device=gpu),
                torch.arange(XID0, XID0 + cap, dtype=torch.int32,
                             device=gpu))
            chk = (idx, xid, dlen, acc)
        rep = B.decode_replies(d, ft, xt, check=chk, tiles=sc.pending)
        assert sc.pending is None
        outs.append((ft, rep, acc))
    (fa, pa, aa), (fb, pb, ab) = outs
    res, rows = FR._same_table(fa, fb, cap)
    FR._same_replies(pa, pb, rows)
    got = {'res': res, 'off': fb.off[:rows].cpu(),
           'len': fb.length[:rows].cpu(),
           'stat64': pb.stat64[:, :rows].cpu(),
           'stat32': pb.stat32[:, :rows].cpu()}
    for c in FR.REPLY_COLS:
        got[c] = getattr(pb, c)[:rows].cpu()
    if dlen is not None:
        assert int(aa.sum().item()) == int(ab.sum().item())
        got['good'] = int(ab.sum().item())
    return got


def _same_outputs(a, b):
    assert a.keys() == b.keys()
    for k, v in a.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, b[k]), k
        else:
            assert v == b[k], k


def _check_gets(got, buf, starts, dls):
    """The decoded GET rows against the stream's own construction and, for a
    few rows, the Jute oracle."""
    n = len(starts)
    assert got['res'][:1] == [n] and got.get('good', n) == n
    assert np.array_equal(got['off'].numpy(), starts + 4)
    assert np.array_equal(got['len'].numpy(), 88 + np.asarray(dls))
    assert got['status'].eq(0).all() and got['opcode'].eq(4).all()
    assert np.array_equal(got['xid'].numpy(), XID0 + np.arange(n))
    assert np.array_equal(got['pay_off'].numpy(), starts + 24)
    assert np.array_equal(got['pay_len'].numpy(), np.asarray(dls))
    assert np.array_equal(got['stat64'][0].numpy(), 1 + np.arange(n))
    for i in (0, n // 2, n - 1):
        o = int(starts[i]) + 4
        pkt = jute.decode_response(bytes(buf[o:o + 88 + int(dls[i])]),
                                   {XID0 + i: 'GET_DATA'})
        s = pkt['stat']
        assert got['zxid'][i].item() == pkt['zxid']
        assert got['stat64'][:, i].tolist() == [
            s.czxid, s.mzxid, s.ctime, s.mtime, s.ephemeralOwner, s.pzxid]
        assert got['stat32'][:, i].tolist() == [
            s.version, s.cversion, s.aversion, s.dataLength, s.numChildren]


# ---- GET replies at the benchmark's pitch and at an odd one ---------------

@pytest.mark.parametrize('n', COUNTS)
@pytest.mark.parametrize('dl', [100, 37], ids=['pitch192', 'odd'])
def test_get_replies(gpu, xt, n, dl):
    """188-byte bodies (192 B pitch: every frame at 4 mod 16), and 37 data
    bytes (129 B pitch: every alignment); for 22 frames the odd pitch is
    273 B, so that the stream still passes one tile."""
    if dl == 37 and n * 129 <= 4096:
        dl = 181
    rng = np.random.default_rng(n + dl)
    dls = np.full(n, dl)
    buf, starts = _get_replies(rng, dls)
    assert len(buf) > 4096
    d = torch.from_numpy(buf).to(gpu)
    dlen = torch.full((n + 3,), dl, dtype=torch.int32, device=gpu)
    got = _both(gpu, xt, d, len(buf), n + 3, dlen)
    _check_gets(got, buf, starts, dls)


def test_stream_ends_inside_a_frame_of_a_wave(gpu, xt):
    """The device length cuts the last frame: the wave's span ends at the
    last whole frame, and no byte past the length counts."""
    rng = np.random.default_rng(6)
    dls = np.full(100, 100)
    buf, starts = _get_replies(rng, dls)
    cut = int(starts[-1]) + 50
    d = torch.from_numpy(buf).to(gpu)
    got = _both(gpu, xt, d, cut, 128)
    assert got['res'] == [99, int(starts[-1]), 0, 0]
    _check_gets(got, buf, starts[:-1], dls[:-1])


# ---- bounds and alignment --------------------------------------------------

@pytest.mark.parametrize('dl', [100, 37], ids=['pitch192', 'odd'])
def test_offsets_and_fills(gpu, xt, dl):
    """The same stream at byte offsets 0, 1, 3 and 13 of a larger buffer (a
    tensor slice), the bytes before the slice and after the stream's length
    filled with two different values: all outputs are identical (offsets are
    relative to the slice).  No byte outside [buf, buf + n) matters."""
    rng = np.random.default_rng(7)
    n = 257
    dls = np.full(n, dl)
    buf, starts = _get_replies(rng, dls)
    dlen = torch.full((n + 3,), dl, dtype=torch.int32, device=gpu)
    sb = torch.from_numpy(buf)
    base = None
    for fill in (0x00, 0xa5):
        for off in (0, 1, 3, 13):
            big = torch.full((off + len(buf) + 64,), fill, dtype=torch.uint8)
            big[off:off + len(buf)] = sb
            d = big.to(gpu)[off:]
            assert d.data_ptr() % 16 == off
            got = _both(gpu, xt, d, len(buf), n + 3, dlen)
            if base is None:
                base = got
                _check_gets(got, buf, starts, dls)
            _same_outputs(base, got)


# ---- a Stat that is not at the tail, and no Stat ---------------------------

def test_create_replies(gpu, xt):
    """The storm workload's CREATE replies (50 B frames, no Stat; their xids
    are not in the table here: ST_NO_XID rows, header fields only)."""
    buf, starts = FR._create_replies(600)
    d = torch.from_numpy(buf).to(gpu)
    got = _both(gpu, xt, d, len(buf), 616)
    assert got['res'] == [600, len(buf), 0, 0]
    assert np.array_equal(got['off'].numpy(), starts + 4)


@pytest.fixture(scope='module')
def corpus(gpu):
    c = M.ReplyCorpus(seed=3, n=600)
    t = B.XidTable(bits=M.XID_BITS, device=gpu)
    tab = t.tab.cpu()
    for slot, ent in c.table():
        tab[slot] = ent
    t.tab.copy_(tab)
    return c, t


@pytest.mark.parametrize('off', [0, 3])
def test_malformed_corpus_in_a_long_stream(gpu, corpus, off):
    """Replies of every opcode (EXISTS / SET_DATA / CREATE / list / ACL /
    notifications) with one mutation each or none, cut bodies and trailing
    bytes included: the tiles path rejects exactly what the plain path
    rejects, which is what the oracle rejects."""
    c, t = corpus
    s = c.stream()
    assert len(s) > 3 * 4096
    big = torch.zeros(off + len(s) + 32, dtype=torch.uint8)
    big[off:off + len(s)] = torch.from_numpy(
        np.frombuffer(s, np.uint8).copy())
    d = big.to(gpu)[off:]
    got = _both(gpu, t, d, len(s), 600)
    assert got['res'] == [600, len(s), 0, 0]
    status = got['status'].tolist()
    seen = set()
    for i in range(600):
        st, _ = c.expect(i)
        if st != M.SKIP:
            assert status[i] == st, (i, c.kind[i])
            seen.add(st)
    assert seen == {M.ST_OK, M.ST_BAD_DECODE, M.ST_NO_XID, M.ST_BAD_OPCODE}


# ---- the fused check through the tiles decoder ------------------------------

@pytest.mark.parametrize('off', [0, 3])
def test_fused_check_on_the_malformed_corpus(gpu, off):
    """The corpus through the check: against the xids its replies were built
    with (most replies carry the expected xid — clean, mutated behind the
    header, or with an unsupported opcode in the table; 'absent', 'alias' and
    'negative' ones and the special xids do not), and against xids no reply
    carries.  Rows and count are the plain decoder's, the count the
    corpus's own."""
    from zkmi.server.tree import GpuTree
    nodes = (11, 110, 16)
    c = M.ReplyCorpus(seed=4, n=600, nodes=nodes)
    t = B.XidTable(bits=M.XID_BITS, device=gpu)
    tab = t.tab.cpu()
    for slot, ent in c.table():
        tab[slot] = ent
    t.tab.copy_(tab)
    tree = GpuTree(100, nodes[2], fanout=10, device=gpu)
    assert (tree.leaf0, tree.leaf0 + tree.n_leaves - 1) == nodes[:2]
    s = c.stream()
    big = torch.zeros(off + len(s) + 32, dtype=torch.uint8)
    big[off:off + len(s)] = torch.from_numpy(
        np.frombuffer(s, np.uint8).copy())
    d = big.to(gpu)[off:]
    idx = torch.tensor(c.chk_idx, dtype=torch.int64, device=gpu)
    xid = torch.tensor(c.chk_xid, dtype=torch.int32, device=gpu)
    got = _both(gpu, t, d, len(s), 600, tree.data_len, sent=(idx, xid))
    assert got['good'] == len(c.chk_rows) > 20
    status = got['status'].tolist()
    for i in range(600):
        st, _ = c.expect(i)
        if st != M.SKIP:
            assert status[i] == st, (i, c.kind[i])
    other = _both(gpu, t, d, len(s), 600, tree.data_len,
                  sent=(idx, xid + 7))
    assert other['good'] == 0
    del got['good'], other['good']
    _same_outputs(got, other)


def test_fused_check_expected_xid_without_an_entry(gpu, xt):
    """Replies that carry the expected xid whose table slot holds nothing,
    another xid, or an opcode that is no reply's: ST_NO_XID / ST_BAD_OPCODE as
    the plain decoder says, and not counted."""
    rng = np.random.default_rng(9)
    n = 300
    dls = np.full(n, 100)
    buf, starts = _get_replies(rng, dls)
    t = B.XidTable(bits=XID_BITS, device=gpu)
    tab = xt.tab.cpu().clone()
    i = np.arange(n)
    slot = torch.from_numpy((XID0 + i) & t.mask)
    tab[slot[i % 7 == 0]] = B.SENTINEL_XID
    tab[slot[i % 7 == 1]] += 1 << 32                  # xid + 1 in the slot
    tab[slot[i % 7 == 2]] += 3                        # GET_DATA -> SET_ACL
    t.tab.copy_(tab)
    d = torch.from_numpy(buf).to(gpu)
    dlen = torch.full((n + 3,), 100, dtype=torch.int32, device=gpu)
    got = _both(gpu, t, d, len(buf), n + 3, dlen)
    want = np.where(i % 7 <= 1, 2, np.where(i % 7 == 2, 3, 0))
    assert np.array_equal(got['status'].numpy(), want)
    assert got['good'] == int((want == 0).sum())


# ---- requests: the serve's tables and the encoded reply stream -------------

@pytest.mark.parametrize('n', COUNTS)
def test_get_pipeline(gpu, n):
    """The GET pipeline end to end on n requests of the synthetic tree's
    paths: request rows, the serve's reply tables, the encoded reply stream
    (192 B pitch), the reply rows and the fused check with its payload
    sample, plain against tiles."""
    FR._get_pair(gpu, 'sf100', n, steps=2, n_nodes=2000, data_bytes=100)


@pytest.mark.parametrize('n', [65, 600])
def test_get_pipeline_long_paths(gpu, n):
    """Paths of 41 .. 71 bytes (past the entry's inline path words) and
    replies of 0 .. 300 data bytes."""
    FR._get_pair(gpu, 'sfpad', n, steps=2, n_nodes=2000, data_dist=(0, 300),
                 name_pad=(20, 50))


# ---- request streams through the read-only serve, plain against staged ------

def _leaf(i):
    return '/bench/d%06d/n%09d' % (i // 1000, i)          # FR._servers' tree


def _get_req(xid, path, op='GET_DATA'):
    return jute.frame(jute.encode_request(
        {'xid': xid, 'opcode': op, 'path': path, 'watch': False}))


def _serve_both(gpu, d, n, cap):
    """The plain and the fused (tiles, staged) read-only serve of ``d[:n]``;
    returns what the fused one wrote, on the host, after comparing."""
    va, vb = FR._servers(gpu, cap)
    va.serve(d, n)
    vb.serve(d, n)
    assert vb.scanner.pending is None
    res, rows = FR._same_table(va.result[3], vb.result[3], cap)
    FR._same_serve(va, vb, rows)
    got = {'res': res}
    for c in ('opcode', 'xid', 'err', 'node', 'slot'):
        got[c] = getattr(vb.resp, c)[:rows].cpu()
    # (a serve advances its tree's zxid, and the two servers' trees live as
    # long as the module: against the plain path the zxids were compared as
    # they are, above; across calls they are taken relative to the batch's
    # first, and left out of the reply stream's headers)
    z = vb.resp.zxid[:rows].cpu()
    got['zxid'] = z - z[:1] if rows else z
    out, total = vb.result[0], int(vb.result[1].item())
    raw = bytearray(out[:total].cpu().numpy().tobytes())
    frames, used, bad = jute.scan_frames(bytes(raw))
    assert bad < 0 and used == len(raw) and len(frames) == rows
    for o, ln in frames:
        assert ln >= 16
        raw[o + 4:o + 12] = bytes(8)
    got['stream'] = bytes(raw)
    return got


def _placed(gpu, s, off, fill=0):
    big = torch.full((off + len(s) + 48,), fill, dtype=torch.uint8)
    big[off:off + len(s)] = torch.from_numpy(np.frombuffer(s, np.uint8).copy())
    return big.to(gpu)[off:]


@pytest.mark.parametrize('n', COUNTS)
def test_serve_requests(gpu, n):
    """n GET_DATA / EXISTS requests, nine in ten on the tree's paths; 22 of
    them take a 190-byte path each so that the stream passes one tile."""
    pad = 'x' * 170 if n * 42 <= 4096 else ''
    s = b''.join(_get_req(7 + i, _leaf((37 * i) % 2200) + pad,
                          'EXISTS' if i % 5 == 0 else 'GET_DATA')
                 for i in range(n))
    assert len(s) > 4096
    got = _serve_both(gpu, _placed(gpu, s, 0), len(s), n + 3)
    assert got['res'][:2] == [n, len(s)]
    hit = np.array([(37 * i) % 2200 < 2000 and not pad for i in range(n)])
    assert np.array_equal(got['err'].numpy() == 0, hit)


@pytest.mark.parametrize('off', [0, 12])
def test_serve_spans_at_the_image(gpu, off):
    """Wave 0's span with its head is exactly the image, wave 1's one byte
    over, wave 2 has one frame larger than the whole image in its middle (its
    neighbours stay staged), wave 3 is plain requests, wave 4 is short."""
    def frames(k0, last_extra):
        fr = [_get_req(k0 + k, _leaf(k0 + k)) for k in range(63)]
        return fr, sum(map(len, fr)) + last_extra
    out, pos = [], 0
    for w, over in ((0, 0), (1, 1)):
        fr, _ = frames(64 * w, 0)
        head = (off + pos + 4) % 16
        # 64 frames' bytes less the first length word = the span
        need = SRV_STAGE + over - head + 4 - sum(map(len, fr))
        fr.append(_get_req(64 * w + 63, '/' + 'y' * (need - 17 - 1)))
        assert head + sum(map(len, fr)) - 4 == SRV_STAGE + over
        out += fr
        pos += sum(map(len, fr))
    fr, _ = frames(128, 0)
    fr.insert(31, _get_req(191, '/' + 'z' * 5000))
    out += fr
    out += [_get_req(192 + k, _leaf(192 + k)) for k in range(64 + 22)]
    s = b''.join(out)
    n = len(out)
    got = _serve_both(gpu, _placed(gpu, s, off), len(s), n + 2)
    assert got['res'][:2] == [n, len(s)]
    miss = {63, 127, 128 + 31}
    assert [i for i in range(n) if got['err'][i].item() != 0] == sorted(miss)


@pytest.mark.parametrize('dl', [25, 58], ids=['short', 'long'])
def test_serve_offsets_and_fills(gpu, dl):
    """The same request stream at byte offsets 0, 1, 3 and 13 of a larger
    buffer, two fills around it: every table and the reply stream are the
    same.  (``long``: 58-byte paths that no node has; long paths that exist
    are in test_get_pipeline_long_paths.)"""
    s = b''.join(_get_req(i, _leaf(i) + 'p' * (dl - 25)) for i in range(257))
    base = None
    for fill in (0x00, 0xa5):
        for off in (0, 1, 3, 13):
            d = _placed(gpu, s, off, fill)
            assert d.data_ptr() % 16 == off
            got = _serve_both(gpu, d, len(s), 260)
            if base is None:
                base = got
                assert got['res'][:2] == [257, len(s)]
            _same_outputs(base, got)


def test_serve_stream_ends_inside_a_frame(gpu):
    s = b''.join(_get_req(i, _leaf(i)) for i in range(150))
    cut = len(s) - 20
    got = _serve_both(gpu, _placed(gpu, s, 0, 0x5a), cut, 160)
    assert got['res'][:2] == [149, len(s) - 42]
    assert got['err'].eq(0).all()


@pytest.mark.parametrize('off', [0, 3])
def test_serve_malformed_requests(gpu, off):
    """The request corpus (one mutation a frame or none): the staged parse
    refuses exactly what the plain one refuses, and answers the rest alike."""
    c = M.RequestCorpus(seed=6, n=600)
    s = c.stream()
    assert len(s) > 3 * 4096
    got = _serve_both(gpu, _placed(gpu, s, off), len(s), 600)
    assert got['res'][:2] == [600, len(s)]
    bad = [M.expect_request(b)[0] in (M.ST_BAD_DECODE, M.ST_BAD_OPCODE)
           for b in c.bodies]
    err = got['err'].tolist()
    assert sum(bad) > 100
    for i, b in enumerate(bad):
        if b:
            assert err[i] != 0, (i, c.kind[i])


# ---- graph capture ---------------------------------------------------------

def test_captured_step_replays(gpu):
    from zkmi.bench import synthetic as S
    ta, _ = FR._tree(gpu, 'sf100', n_nodes=2000, data_bytes=100)
    pipe = S.GetPipeline(ta, 2048, seed=5, streams=2)
    assert int(pipe.step().item()) == 2048         # eager: buffers sized
    acc = torch.zeros(1, dtype=torch.int64, device=gpu)
    g = pipe.capture(acc)
    acc.zero_()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert int(acc.item()) == 3 * 2048
