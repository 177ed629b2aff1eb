"""K1 with its rows pass deferred to the frame table's first reader.

``FrameScanner.scan(..., rows=False)`` launches fs_tile and fs_link only;
the fused consumers — ``decode_replies(..., tiles=)`` and the GPU server's
fused serve — take each workgroup's 256 rows from the scan's tile lists
(csrc/kernels/zk_frame_rows.h), write them to the frame table and clear the
scan's flags, as fs_rows did.  Every case here is differential on one
stream: (a) the three-launch scan and the plain consumer, (b) the deferred
scan and the fused consumer on a second scanner; everything either path
writes must be equal, and where a Python walk of the length chain is cheap
the offsets are compared with it too."""

import numpy as np
import pytest
import torch

from zkmi.ops import batch as B

pytestmark = pytest.mark.gpu

REPLY_COLS = ('xid', 'err', 'opcode', 'status', 'zxid', 'pay_off', 'pay_len',
              'aux0', 'aux1')


def _stream(rng, lens, payload='random'):
    """Frames with the given body lengths (tests/test_frame_repair.py)."""
    lens = np.asarray(lens, np.int64)
    starts = np.zeros(len(lens), np.int64)
    np.cumsum(lens[:-1] + 4, out=starts[1:])
    total = int(starts[-1] + lens[-1] + 4)
    if payload == 'random':
        buf = rng.integers(0, 256, total, dtype=np.uint8)
    else:
        words = rng.integers(8, 201, (total + 3) // 4).astype('>u4')
        buf = np.frombuffer(words.tobytes(), np.uint8)[:total].copy()
    for k in range(4):
        buf[starts + k] = ((lens >> (8 * (3 - k))) & 0xff).astype(np.uint8)
    return buf, starts


def _create_replies(n, xid0=0x300401, zxid0=0x3f4a2c):
    """The storm workload's CREATE replies (tests/test_frame_repair.py)."""
    i = np.arange(n, dtype=np.int64)
    rec = np.zeros((n, 50), np.uint8)

    def be(col, v, w):
        for b in range(w):
            rec[:, col + b] = (v >> (8 * (w - 1 - b))) & 0xff
    be(0, np.full(n, 46), 4)
    be(4, xid0 + i, 4)
    be(8, zxid0 + i, 8)
    be(20, np.full(n, 26), 4)
    paths = np.frombuffer(b''.join(b'/storm/d%05d/e-%010d' % (k % 100, k)
                                   for k in range(n)), np.uint8)
    rec[:, 24:] = paths.reshape(n, 26)
    return rec.reshape(-1), np.arange(n, dtype=np.int64) * 50


def _host_frames(b, maxp=1 << 24):
    """(body offsets, consumed, bad) of the length chain of bytes ``b``."""
    off, p = [], 0
    while p + 4 <= len(b):
        ln = int.from_bytes(b[p:p + 4], 'big', signed=True)
        if ln < 0 or ln > maxp:
            return off, p, True
        if p + 4 + ln > len(b):
            break
        off.append(p + 4)
        p += 4 + ln
    return off, p, False


def _same_table(fa, fb, cap):
    ra, rb = fa.result.cpu(), fb.result.cpu()
    assert torch.equal(ra, rb), (ra, rb)
    n = min(int(ra[0]), cap)
    assert torch.equal(fa.off[:n], fb.off[:n])
    assert torch.equal(fa.length[:n], fb.length[:n])
    return ra.tolist(), n


def _same_replies(pa, pb, n):
    for c in REPLY_COLS:
        assert torch.equal(getattr(pa, c)[:n], getattr(pb, c)[:n]), c
    assert torch.equal(pa.stat64[:, :n], pb.stat64[:, :n])
    assert torch.equal(pa.stat32[:, :n], pb.stat32[:, :n])


@pytest.fixture(scope='module')
def xt(gpu):
    return B.XidTable(bits=16, device=gpu)


_trees = {}


def _tree(gpu, key, **kw):
    """Two identical small trees per key (the plain and the fused server's:
    a serve advances its tree's zxid)."""
    from zkmi.server.tree import GpuTree
    if key not in _trees:
        # (one creation time: the nodes' ctime / mtime are in every Stat)
        _trees[key] = tuple(GpuTree(device=gpu, seed=0,
                                    ctime_ms=1_700_000_000_000, **kw)
                            for _ in range(2))
    return _trees[key]


def _servers(gpu, cap):
    from zkmi.server.engine import GpuServer
    ta, tb = _tree(gpu, 'srv', n_nodes=2000, data_bytes=37)
    mk = lambda t, f: GpuServer(t, cap, cap * 160 + 64,        # noqa: E731
                                seq_order=False, fused_rows=f)
    sa, sb = mk(ta, False), mk(tb, True)
    sa.read_only = sb.read_only = True
    return sa, sb


def _same_serve(sa, sb, n):
    ra, rb = sa.resp, sb.resp
    for c in ('opcode', 'xid', 'err', 'node', 'zxid', 'slot'):
        assert torch.equal(getattr(ra, c)[:n], getattr(rb, c)[:n]), c
    assert torch.equal(sa.presized[0][:n], sb.presized[0][:n])       # sizes
    nb = (n + 255) // 256
    assert torch.equal(sa.presized[1][:nb], sb.presized[1][:nb])     # bsum
    (oa, ta, ea, _), (ob, tb, eb, _) = sa.result, sb.result
    tot = int(ta.item())
    assert tot == int(tb.item()) and int(ea.item()) == int(eb.item())
    assert torch.equal(oa[:tot], ob[:tot])


def _pair(gpu, xt, buf, cap, window, n=None, serve=True, want=None, **kw):
    """Both paths over ``buf`` (numpy bytes): the decode and (read-only) the
    serve.  ``n``: a device length (default: the host length).  Returns the
    fused scanner and the host result."""
    d = torch.from_numpy(buf).to(gpu)
    ln = len(buf) if n is None else n
    sa = B.FrameScanner(cap, gpu, window=window)
    sb = B.FrameScanner(cap, gpu, window=window)
    fa = sa.scan(d, ln, **kw)
    pa = B.decode_replies(d, fa, xt)
    fb = sb.scan(d, ln, rows=False, **kw)
    assert sb.pending is not None and sb.clean_for == -1
    pb = B.decode_replies(d, fb, xt, tiles=sb.pending)
    assert sb.pending is None and sb.clean_for == sb.last_cap
    res, rows = _same_table(fa, fb, cap)
    _same_replies(pa, pb, rows)
    if want is not None:
        assert np.array_equal(fb.off[:rows].cpu().numpy(),
                              np.asarray(want[:rows], np.int64))
    if serve:
        va, vb = _servers(gpu, cap)
        va.serve(d, ln)
        vb.serve(d, ln)
        assert vb.scanner.pending is None
        _same_table(va.result[3], vb.result[3], cap)
        _same_serve(va, vb, rows)
    return sb, res


# ---- 1, 2, 3b: GET end to end ------------------------------------------

def _plain_twin(pipe):
    """Make a GetPipeline take the three-launch scans and the plain
    consumers (what every other pipeline still runs)."""
    pipe.server.fused_rows = False       # the reply side follows the server
    return pipe


def _get_pair(gpu, key, batch, steps=3, **tree_kw):
    from zkmi.bench import synthetic as S
    ta, tb = _tree(gpu, key, **tree_kw)
    pa = _plain_twin(S.GetPipeline(ta, batch, seed=3))
    pb = S.GetPipeline(tb, batch, seed=3)
    assert pb.server.fused_rows
    for _ in range(steps):
        aa, ab = pa.step(), pb.step()
        assert pa.server.scanner.pending is None
        assert pa.rscanner.pending is None
        assert int(aa.item()) == batch and int(ab.item()) == batch
        (ia, ra, xa, fa), (ib, rb, xb, fb) = pa.last, pb.last
        assert torch.equal(ia, ib)
        res, rows = _same_table(fa, fb, batch)
        assert rows == batch and res[2] == 0 and res[3] == 0
        _same_replies(ra, rb, rows)
        _same_table(pa.server.result[3], pb.server.result[3], batch)
        _same_serve(pa.server, pb.server, batch)
        # the host framing of the reply stream
        want, used, bad = _host_frames(xb[:res[1]].cpu().numpy().tobytes())
        assert not bad and used == res[1]
        assert np.array_equal(fb.off[:rows].cpu().numpy(),
                              np.asarray(want, np.int64))
    return pa, pb


def test_get_odd_sizes(gpu):
    """5000 requests (not a multiple of 256): ~52 request tiles (one count
    block), ~158 reply tiles (three)."""
    pa, pb = _get_pair(gpu, 'g37', 5000, n_nodes=20000, data_bytes=37)
    # both scans of the fused pipeline ran deferred, and clean after step 1
    assert pb.server.scanner.last_clean and pb.rscanner.last_clean
    assert pb.server.scanner.pending is None and pb.rscanner.pending is None


def test_get_on_an_acl_tree_stays_plain(gpu):
    """A tree with an ACL table: the serve may not be fused, and the reply
    side stays on the three-launch scan with it."""
    from zkmi.bench import synthetic as S
    from zkmi.server.tree import GpuTree
    tree = GpuTree(2000, 37, device=gpu, seed=0, acl_cap=4)
    pipe = S.GetPipeline(tree, 3000, seed=3)
    assert not pipe.server.fused_rows
    for _ in range(2):
        assert int(pipe.step().item()) == 3000
        assert pipe.rscanner.pending is None
        assert pipe.rscanner.clean_for == pipe.rscanner.last_cap


def test_get_several_count_blocks_of_requests(gpu):
    """20000 requests: ~205 request tiles, four 64-tile count blocks."""
    _get_pair(gpu, 'g37', 20000, steps=2, n_nodes=20000, data_bytes=37)


def test_get_frames_longer_than_a_tile(gpu):
    """Replies of 0..9000 data bytes: tiles without a frame start, frame
    blocks spanning more than 256 tiles, long-frame mode."""
    _get_pair(gpu, 'g9000', 2000, steps=2, n_nodes=2000,
              data_dist=(0, 9000))


# ---- 3a: long frames with plausible payloads ---------------------------

def test_long_frames_span_many_tiles(gpu, xt):
    rng = np.random.default_rng(8)
    lens = rng.integers(2000, 9001, 3000)
    buf, starts = _stream(rng, lens, payload='plausible')
    for kw in ({}, {'misspec': 2}):
        _, res = _pair(gpu, xt, buf, len(lens) + 16, 256, want=starts + 4,
                       **kw)
        assert res == [len(lens), len(buf), 0, 0]


# ---- 4: stale tiles ------------------------------------------

@pytest.mark.parametrize('kw', [{}, {'misspec': 3}, {'nospec': True}],
                         ids=['spec', 'misspec3', 'nospec'])
def test_stale_tiles_are_walked(gpu, xt, kw):
    """Create replies whose zxids run through 0x2Exxxx inside the stream: a
    phantom chain that fs_link's chase settles by lookup, leaving stale
    tiles whose rows the consumer must walk."""
    n = 100000
    buf, starts = _create_replies(n, zxid0=0x2E0000 - 30000)
    sb, res = _pair(gpu, xt, buf, n + 16, 256, want=starts + 4, **kw)
    assert res == [n, len(buf), 0, 0]
    if not kw:
        # (the forced repairs re-walk tiles instead of looking them up)
        assert sb.chain_stats()['looked_up'] > 0


# ---- 5: terminals ------------------------------------------

def _benign(seed=4, n=6000):
    rng = np.random.default_rng(seed)
    lens = rng.integers(20, 301, n)
    return _stream(rng, lens) + (lens,)


def test_bad_length_in_the_middle(gpu, xt):
    buf, starts, lens = _benign()
    k = 3111
    buf = buf.copy()
    buf[starts[k]:starts[k] + 4] = (0xff, 0xff, 0xff, 0xf0)     # negative
    sb, res = _pair(gpu, xt, buf, len(lens) + 16, 512, want=starts[:k] + 4)
    assert res == [k, int(starts[k]), 1, 0]
    # tiles past the bad frame are dead, their flags cleared all the same:
    # the next scan of the workspace runs clean and is exact
    d = torch.from_numpy(buf).to(gpu)
    ft = sb.scan(d, len(buf), rows=False)
    assert sb.last_clean
    B.decode_replies(d, ft, xt, tiles=sb.pending)
    assert ft.result.cpu().tolist() == res
    assert np.array_equal(ft.off[:k].cpu().numpy(), starts[:k] + 4)
    # a flag left set would cost the second scan its speculation: the
    # chain counters of the two scans are the plain path's
    plain = B.FrameScanner(len(lens) + 16, gpu, window=512)
    for _ in range(2):
        plain.scan(d, len(buf))
    assert sb.chain_stats() == plain.chain_stats()


def test_partial_trailing_frame(gpu, xt):
    buf, starts, lens = _benign()
    cut = int(starts[-1]) + 9                     # inside the last frame
    _, res = _pair(gpu, xt, buf[:cut].copy(), len(lens) + 16, 512,
                   want=starts[:-1] + 4)
    assert res == [len(lens) - 1, int(starts[-1]), 0, 0]


def test_empty_stream(gpu, xt):
    """A device length of zero over a many-tile buffer: fs_link's early exit
    (*lastk = -1), no row, the flags' tail still cleared."""
    buf, starts, lens = _benign()
    n0 = torch.zeros(1, dtype=torch.int64, device=gpu)
    sb, res = _pair(gpu, xt, buf, len(lens) + 16, 512, n=n0)
    assert res == [0, 0, 0, 0]


def test_table_smaller_than_the_stream(gpu, xt):
    buf, starts, lens = _benign()
    cap = 2500                                    # not a multiple of 256
    _, res = _pair(gpu, xt, buf, cap, 512, want=starts + 4)
    assert res == [len(lens), len(buf), 0, 1]


def test_one_tile_streams_keep_the_plain_path(gpu, xt):
    buf, starts, lens = _benign(n=12)
    d = torch.from_numpy(buf).to(gpu)
    assert len(buf) <= 4096
    sc = B.FrameScanner(64, gpu, window=512)
    ft = sc.scan(d, len(buf), rows=False)
    assert sc.pending is None                     # one launch wrote the rows
    assert np.array_equal(ft.off[:12].cpu().numpy(), starts + 4)


# ---- 6: housekeeping ------------------------------------------

def test_consumer_leaves_the_workspace_clean(gpu, xt):
    lens = range(20000)
    buf, starts = _create_replies(len(lens), zxid0=0x500000)   # no phantom
    d = torch.from_numpy(buf).to(gpu)
    cap = len(lens) + 16
    plain = B.FrameScanner(cap, gpu, window=512)
    for _ in range(3):
        plain.scan(d, len(buf))
    want = plain.chain_stats()
    sc = B.FrameScanner(cap, gpu, window=512)
    cleans = []
    for _ in range(3):
        ft = sc.scan(d, len(buf), rows=False)
        cleans.append(sc.last_clean)
        B.decode_replies(d, ft, xt, tiles=sc.pending)
        assert ft.result.cpu().tolist() == [len(lens), len(buf), 0, 0]
        assert np.array_equal(ft.off[:len(lens)].cpu().numpy(), starts + 4)
    assert cleans == [False, True, True]
    st = sc.chain_stats()
    assert st == want
    assert st['rewalked'] == 0 and st['rounds'] == 0 and st['no_spec'] == 0
    # a deferred scan whose consumer was skipped: the next scan memsets
    sc.scan(d, len(buf), rows=False)
    assert sc.pending is not None
    ft = sc.scan(d, len(buf), rows=False)
    assert not sc.last_clean
    B.decode_replies(d, ft, xt, tiles=sc.pending)
    assert np.array_equal(ft.off[:len(lens)].cpu().numpy(), starts + 4)
    sc.scan(d, len(buf))                           # plain again, and clean
    assert sc.last_clean and sc.pending is None


def test_fused_serve_only_as_first_reader(gpu):
    from zkmi.server.engine import GpuServer
    ta, _ = _tree(gpu, 'srv', n_nodes=2000, data_bytes=37)
    with pytest.raises(ValueError):
        GpuServer(ta, 256, 1 << 16, seq_order=True, fused_rows=True)
    srv = GpuServer(ta, 256, 1 << 16, seq_order=False, fused_rows=True)
    rx = torch.zeros(8192, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        srv.serve(rx, 8192, ordered=True)


# ---- 7: graph capture ------------------------------------------

def test_captured_step_replays(gpu):
    from zkmi.bench import synthetic as S
    ta, _ = _tree(gpu, 'g37', n_nodes=20000, data_bytes=37)
    pipe = S.GetPipeline(ta, 8192, seed=5, streams=2)
    assert int(pipe.step().item()) == 8192         # eager: buffers sized
    acc = torch.zeros(1, dtype=torch.int64, device=gpu)
    g = pipe.capture(acc)
    acc.zero_()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert int(acc.item()) == 3 * 8192
