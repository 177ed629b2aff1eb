"""The split and the merge of mixed batches alone (csrc/kernels/tree_mix.hip,
torch.ops.zkmi.tree_mix_split / tree_mix_merge): synthetic frame tables and
byte streams, no tree; the expectation is numpy's — the stable selection per
class for the split, the gather of the replies for the merge."""

import struct

import numpy as np
import pytest
import torch

from zkmi.ops import _lib

pytestmark = pytest.mark.gpu

A, C, L = _lib.MIX_A, _lib.MIX_C, _lib.MIX_L
I64, I32, U8 = torch.int64, torch.int32, torch.uint8
NS = [0, 1, 63, 64, 65, 255, 256, 257, 600]


# ---- split -------------------------------------------------------------------

def _body(cls, k):
    """A frame body of class `cls` (on a tree with an ACL table), the k-th:
    well-formed and truncated list / GET_ACL frames; for the serve's class
    known ops, frames shorter than 8 bytes and unknown opcodes."""
    xid = struct.pack('>i', 1000 + k)
    path = b'/bench/d%06d' % k
    tail = struct.pack('>i', len(path)) + path
    if cls == L:
        op = (8, 12)[k % 2]
        full = xid + struct.pack('>i', op) + tail + b'\0'
        return full[:8 + (k % 5)] if k % 3 == 0 else full
    if cls == C:
        full = xid + struct.pack('>i', 6) + tail
        return full[:8 + (k % 4)] if k % 3 == 1 else full
    kind = k % 6
    if kind == 0:
        return (xid + struct.pack('>i', 4))[:k % 8]     # 0..7 bytes
    if kind == 1:
        op = (9999, -1, 7, 13, 0x06000000, 0x0c000000)[(k // 6) % 6]
        return xid + struct.pack('>i', op) + tail
    op = (4, 3, 5, 1)[kind - 2]
    return xid + struct.pack('>i', op) + tail + b'\0' * (kind + 1)


def _patterns(n):
    rng = np.random.default_rng(1234 + n)
    i = np.arange(n)
    pats = {'rotation': np.array([A, L, C])[i % 3],
            'runs70': np.array([A, C, L])[(i // 70) % 3],
            'random': rng.integers(0, 3, n)}
    for c in (A, C, L):
        pats['only%d' % c] = np.full(n, c)
    for a, b in ((A, C), (A, L), (C, L)):
        pats['pair%d%d' % (a, b)] = np.where(rng.integers(0, 2, n) == 0, a, b)
    return pats


def _split_case(gpu, n, classes, has_acl, ncap):
    bodies = [_body(int(c), k) for k, c in enumerate(classes)]
    raw = bytearray()
    foff = np.zeros(ncap, np.int64)
    flen = np.zeros(ncap, np.int32)
    for k, b in enumerate(bodies):
        raw += struct.pack('>i', len(b))
        foff[k], flen[k] = len(raw), len(b)
        raw += b
    raw += b'\0' * 16
    rx = torch.frombuffer(raw, dtype=U8).to(gpu)
    dev = dict(device=gpu)
    cls = torch.full((ncap,), 77, dtype=I32, **dev)
    sub = torch.full((ncap,), 77, dtype=I32, **dev)
    foff_c = torch.full((3 * ncap,), -5, dtype=I64, **dev)
    flen_c = torch.full((3 * ncap,), -5, dtype=I32, **dev)
    counts = torch.full((3,), -5, dtype=I64, **dev)
    ws = torch.empty(max(_lib.tree_mix_split_workspace(ncap), 16), dtype=U8,
                     **dev)
    _lib.tree_mix_split(rx, torch.from_numpy(foff).to(gpu),
                        torch.from_numpy(flen).to(gpu),
                        torch.tensor([n], dtype=I64, **dev), ncap, has_acl,
                        cls, sub, foff_c, flen_c, counts, ws)
    want = np.array([int(c) for c in classes], np.int64)
    if not has_acl:
        want[want == C] = A
    got_cls = cls.cpu().numpy()
    got_sub = sub.cpu().numpy()
    assert got_cls[:n].tolist() == want.tolist()
    assert (got_cls[n:] == -1).all()
    fo = foff_c.cpu().numpy().reshape(3, ncap) if ncap else np.zeros((3, 0))
    fl = flen_c.cpu().numpy().reshape(3, ncap) if ncap else np.zeros((3, 0))
    got_counts = counts.cpu().tolist()
    for c in (A, C, L):
        sel = np.nonzero(want == c)[0]
        assert got_counts[c] == len(sel)
        assert got_sub[sel].tolist() == list(range(len(sel)))
        assert fo[c, :len(sel)].tolist() == foff[sel].tolist()
        assert fl[c, :len(sel)].tolist() == flen[sel].tolist()
        # nothing past the class's rows was written
        assert (fo[c, len(sel):] == -5).all()


@pytest.mark.parametrize('n', NS)
def test_split(gpu, n):
    """cls / sub / counts exact and every sub-table the stable selection, for
    the rotation A, L, C, runs of 70 a class (longer than a wave), a seeded
    random pattern, every class alone and every pair; frames shorter than 8
    bytes and unknown opcodes in the serve's class, truncated list and
    GET_ACL frames with their engines; GET_ACL in the serve's class when the
    ACL flag is off.  The table holds a few rows more than the batch."""
    for name, classes in _patterns(n).items():
        for has_acl in (True, False):
            _split_case(gpu, n, classes, has_acl, n + 3)
    _split_case(gpu, n, _patterns(n)['random'], True, max(n, 1))


def test_split_empty_table(gpu):
    _split_case(gpu, 0, np.zeros(0, np.int64), True, 0)


# ---- merge -------------------------------------------------------------------

def _merge_inputs(gpu, lens, classes, ncap, seed=0, skew=(3, 9, 14)):
    """Three source streams of random bytes holding the replies of their
    class back to back (each tensor starts `skew` bytes into its allocation,
    so the three differ modulo 16), the engines' rec_off / total / err, the
    split's cls / sub / counts, and numpy's merged stream."""
    rng = np.random.default_rng(seed)
    n = len(lens)
    lens = np.asarray(lens, np.int64)
    classes = np.asarray(classes, np.int64)
    dev = dict(device=gpu)
    cls = np.full(ncap, -1, np.int32)
    sub = np.zeros(ncap, np.int32)
    cls[:n] = classes
    streams, rec_offs, totals, errs, host = [], [], [], [], []
    counts = []
    for c in range(3):
        sel = np.nonzero(classes == c)[0]
        sub[sel] = np.arange(len(sel))
        ro = np.zeros(ncap, np.int64)
        cs = np.concatenate([[0], np.cumsum(lens[sel])])
        ro[:len(sel)] = cs[:-1]
        ro[len(sel):] = cs[-1]
        tot = int(cs[-1])
        data = rng.integers(0, 256, tot + 40, dtype=np.uint8)
        host.append(data)
        buf = torch.zeros(skew[c] + tot + 40, dtype=U8, **dev)
        buf[skew[c]:] = torch.from_numpy(data).to(gpu)
        streams.append(buf[skew[c]:])
        rec_offs.append(torch.from_numpy(ro).to(gpu))
        totals.append(torch.tensor([tot], dtype=I64, **dev))
        errs.append(torch.zeros(1, dtype=I32, **dev))
        counts.append(len(sel))
    want = bytearray()
    starts = []
    pos = [0, 0, 0]
    for k in range(n):
        c = int(classes[k])
        starts.append(len(want))
        want += host[c][pos[c]:pos[c] + int(lens[k])].tobytes()
        pos[c] += int(lens[k])
    return dict(cls=torch.from_numpy(cls).to(gpu),
                sub=torch.from_numpy(sub).to(gpu),
                count=torch.tensor([n], dtype=I64, **dev),
                counts=torch.tensor(counts, dtype=I64, **dev), ncap=ncap,
                streams=streams, rec_offs=rec_offs, totals=totals, errs=errs,
                want=bytes(want), starts=starts)


FILL = 0xA5


def _merge(gpu, m, out_cap=None, terminate=False, dskew=0, **over):
    """Run the merge into a buffer prefilled with FILL (`dskew` bytes into its
    allocation); returns (out bytes, rec_off, total, err)."""
    dev = dict(device=gpu)
    T = len(m['want'])
    if out_cap is None:
        out_cap = T + 24
    buf = torch.full((dskew + out_cap + 64,), FILL, dtype=U8, **dev)
    out = buf[dskew:]
    ncap = m['ncap']
    a = dict(cls=m['cls'], sub=m['sub'], count=m['count'],
             counts=m['counts'], ncap=ncap, streams=m['streams'],
             rec_offs=m['rec_offs'], totals=m['totals'], errs=m['errs'],
             out=out, out_cap=out_cap,
             rec_off=torch.full((ncap,), -7, dtype=I64, **dev),
             total=torch.full((1,), -7, dtype=I64, **dev),
             err=torch.full((1,), -7, dtype=I32, **dev),
             ws=torch.empty(max(_lib.tree_mix_merge_workspace(ncap), 16),
                            dtype=U8, **dev))
    a.update(over)
    _lib.tree_mix_merge(a['cls'], a['sub'], a['count'], a['counts'],
                        a['ncap'], a['streams'], a['rec_offs'], a['totals'],
                        a['errs'], a['out'], a['out_cap'], a['rec_off'],
                        a['total'], a['err'], a['ws'], terminate)
    return (bytes(buf.cpu().numpy().tobytes())[dskew:],
            a['rec_off'].cpu().tolist(), int(a['total'].item()),
            int(a['err'].item()))


def _check_merged(m, got, terminate, out_cap=None):
    raw, rec_off, total, err = got
    T = len(m['want'])
    n = len(m['starts'])
    assert err == 0 and total == T
    assert rec_off[:n] == m['starts']
    assert all(x == T for x in rec_off[n:])
    assert raw[:T] == m['want']
    rest = raw[T:]
    if terminate:
        assert rest[:4] == b'\xff' * 4
        rest = rest[4:]
    assert rest == bytes([FILL]) * len(rest)       # not a byte past the stream


def _alignment_lens():
    """Every reply length from 20 to 20 + 64, four times over in a seeded
    order, with seeded classes."""
    rng = np.random.default_rng(7)
    lens = np.concatenate([rng.permutation(np.arange(20, 85))
                           for _ in range(4)])
    return lens, rng.integers(0, 3, len(lens))


def test_merge_every_alignment(gpu):
    """Replies of every length from 20 to 84 bytes: every source alignment
    and every destination alignment modulo 16 occurs, and most of their 256
    pairs; byte-equal to the numpy gather, with rec_off, total, the
    terminator, and no byte written past it."""
    lens, classes = _alignment_lens()
    skew = (3, 9, 14)
    m = _merge_inputs(gpu, lens, classes, len(lens) + 5, skew=skew)
    pairs = set()
    pos = [0, 0, 0]
    for k, c in enumerate(classes):
        pairs.add(((skew[c] + pos[c]) % 16, m['starts'][k] % 16))
        pos[c] += int(lens[k])
    assert {s for s, _ in pairs} == set(range(16))
    assert {d for _, d in pairs} == set(range(16))
    assert len(pairs) >= 128
    for terminate in (False, True):
        _check_merged(m, _merge(gpu, m, terminate=terminate), terminate)
    # the destination itself off the 16-byte grid
    _check_merged(m, _merge(gpu, m, terminate=True, dskew=5), True)


def test_merge_tier_bounds(gpu):
    """Each tier bound of the copy, minus 1, exact and plus 1, in every
    class, between 20-byte replies."""
    small, wave = _lib.tree_mix_bounds()
    assert 20 < small < wave
    lens, classes = [], []
    for k, b in enumerate((small, wave)):
        for d in (-1, 0, 1):
            for c in range(3):
                lens += [20, b + d, 21 + c]
                classes += [(c + 1) % 3, c, (c + k) % 3]
    m = _merge_inputs(gpu, lens, classes, len(lens), seed=3)
    _check_merged(m, _merge(gpu, m, terminate=True), True)
    _check_merged(m, _merge(gpu, m, dskew=11), False)


def test_merge_one_large_reply(gpu):
    """One reply of about 70 KB (past the wave tier: the queue of the whole
    grid takes it) beside 20-byte ones; then two of them in one batch."""
    lens = [20] * 70 + [70_001] + [20] * 70
    classes = [k % 2 for k in range(70)] + [L] + [k % 3 for k in range(70)]
    m = _merge_inputs(gpu, lens, classes, 256, seed=5)
    _check_merged(m, _merge(gpu, m, terminate=True), True)
    lens = [20, 70_001, 33, 131_072 + 7, 20]
    m = _merge_inputs(gpu, lens, [A, L, C, L, A], 8, seed=6)
    _check_merged(m, _merge(gpu, m, terminate=True, dskew=7), True)


@pytest.mark.parametrize('ncap', [0, 4])
def test_merge_empty_batch(gpu, ncap):
    m = _merge_inputs(gpu, [], [], ncap)
    for terminate in (False, True):
        _check_merged(m, _merge(gpu, m, terminate=terminate), terminate)


def test_merge_overflow_and_engine_errors(gpu):
    """The merged stream one byte too long for out: err 2; an engine's
    non-zero err is the merged one, the serve's first.  total 0 and out
    unchanged either way.  The terminator is left out when it does not fit."""
    lens, classes = _alignment_lens()
    m = _merge_inputs(gpu, lens[:100], classes[:100], 128)
    T = len(m['want'])

    def untouched(got, err):
        raw, _, total, e = got
        assert (e, total) == (err, 0)
        assert raw == bytes([FILL]) * len(raw)

    untouched(_merge(gpu, m, out_cap=T - 1, terminate=True), 2)
    raw, _, total, err = _merge(gpu, m, out_cap=T + 3, terminate=True)
    assert (err, total) == (0, T) and raw[:T] == m['want']
    assert raw[T:] == bytes([FILL]) * len(raw[T:])
    for c in range(3):
        m['errs'][c].fill_(2 + c)
        untouched(_merge(gpu, m), 2 + c)
        m['errs'][c].zero_()
    m['errs'][A].fill_(3)
    m['errs'][L].fill_(7)
    untouched(_merge(gpu, m), 3)
    m['errs'][A].zero_()
    m['errs'][C].fill_(5)
    untouched(_merge(gpu, m), 5)
    for c in range(3):
        m['errs'][c].zero_()
    _check_merged(m, _merge(gpu, m), False)


def test_merge_ignores_rows_the_engines_do_not_bear_out(gpu):
    """A class or an index out of range and a span past its stream's total
    are merged as empty replies: the copies stay in bounds."""
    m = _merge_inputs(gpu, [20, 30, 40, 50], [A, C, L, A], 6)
    cls = m['cls'].clone()
    sub = m['sub'].clone()
    cls[1] = 9
    sub[2] = 5
    raw, rec_off, total, err = _merge(gpu, m, cls=cls, sub=sub)
    assert err == 0 and total == 70 and rec_off[:4] == [0, 20, 20, 20]
    assert raw[:20] == m['want'][:20] and raw[20:70] == m['want'][90:140]
    short = [t.clone() for t in m['totals']]
    short[A].fill_(10)                   # the A replies are [0, 20), [20, 70)
    raw, rec_off, total, err = _merge(gpu, m, totals=short)
    assert err == 0 and total == 70 and rec_off[:4] == [0, 0, 30, 70]
    assert raw[:70] == m['want'][20:90]


def test_argument_checks(gpu):
    """Both ops check dtype, device and length before a pointer reaches a
    kernel."""
    m = _merge_inputs(gpu, [20, 30, 40], [A, C, L], 4)
    for bad in (dict(cls=m['cls'].to(I64)),
                dict(sub=m['sub'].cpu()),
                dict(rec_off=torch.zeros(3, dtype=I64, device=gpu)),
                dict(counts=torch.zeros(2, dtype=I64, device=gpu)),
                dict(streams=m['streams'][:2]),
                dict(rec_offs=[t[:3] for t in m['rec_offs']]),
                dict(errs=[t.to(I64) for t in m['errs']]),
                dict(total=torch.zeros(1, dtype=I32, device=gpu)),
                dict(out=torch.empty(8, dtype=U8, device=gpu)),
                dict(out=m['streams'][0]),
                dict(ws=torch.empty(16, dtype=U8, device=gpu))):
        with pytest.raises(RuntimeError):
            _merge(gpu, m, **bad)
            pytest.fail('accepted: %s' % sorted(bad))
    big = torch.zeros(2048, dtype=U8, device=gpu)
    with pytest.raises(RuntimeError, match='overlaps'):
        _merge(gpu, m, streams=[big[:1024]] + m['streams'][1:],
               out=big[512:])
    _check_merged(m, _merge(gpu, m), False)

    ncap = 4
    dev = dict(device=gpu)
    good = dict(rx=torch.zeros(64, dtype=U8, **dev),
                foff=torch.zeros(ncap, dtype=I64, **dev),
                flen=torch.zeros(ncap, dtype=I32, **dev),
                count=torch.zeros(1, dtype=I64, **dev), cls=None, sub=None,
                foff_c=None, flen_c=None, counts=None, ws=None)

    def split(**over):
        a = dict(good,
                 cls=torch.empty(ncap, dtype=I32, **dev),
                 sub=torch.empty(ncap, dtype=I32, **dev),
                 foff_c=torch.empty(3 * ncap, dtype=I64, **dev),
                 flen_c=torch.empty(3 * ncap, dtype=I32, **dev),
                 counts=torch.empty(3, dtype=I64, **dev),
                 ws=torch.empty(_lib.tree_mix_split_workspace(ncap),
                                dtype=U8, **dev))
        a.update(over)
        _lib.tree_mix_split(a['rx'], a['foff'], a['flen'], a['count'], ncap,
                            True, a['cls'], a['sub'], a['foff_c'],
                            a['flen_c'], a['counts'], a['ws'])
        return a

    for bad in (dict(rx=torch.zeros(64, dtype=I32, **dev)),
                dict(foff=torch.zeros(ncap, dtype=I32, **dev)),
                dict(flen=torch.zeros(ncap, dtype=I32)),
                dict(count=torch.zeros(1, dtype=I32, **dev)),
                dict(cls=torch.empty(ncap - 1, dtype=I32, **dev)),
                dict(sub=torch.empty(ncap, dtype=I64, **dev)),
                dict(foff_c=torch.empty(2 * ncap, dtype=I64, **dev)),
                dict(flen_c=torch.empty(3 * ncap, dtype=I64, **dev)),
                dict(counts=torch.empty(2, dtype=I64, **dev)),
                dict(ws=torch.empty(16, dtype=U8, **dev))):
        with pytest.raises(RuntimeError):
            split(**bad)
            pytest.fail('accepted: %s' % sorted(bad))
    a = split()
    assert a['counts'].cpu().tolist() == [0, 0, 0]
