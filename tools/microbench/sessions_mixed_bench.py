"""Session batches of any op mix: GpuServer.serve_sessions_mixed
(csrc/kernels/tree_sess.hip sess_split_seg_k, the session instances of the
list and GET_ACL engines) on a 1M-znode tree with an ACL table and a watch
table.

S connections send r requests each: about 10 % GET_CHILDREN2 on the tree's
directories (list_bench's shape), about 10 % GET_ACL on random leaves
(acl_bench's shape), the rest 80 % GET_DATA and 20 % SET_DATA on random leaves
(sessions_bench's shape).  Three sides, captured graphs in the same run (CUDA
events, median after warm-up replays):

  sessions_mixed  ONE serve_sessions_mixed over the concatenated stream with
                  the segment table (a session and a watcher slot a
                  connection);
  serves          S serve_mixed(session=, wslot=) calls over the same bytes, a
                  stream a connection, on a server sized for r frames: the
                  path the new call replaces;
  floor           ONE serve_mixed of the same bytes as a single session: what
                  the batch costs without segments.

All three produce the same number of reply bytes (checked; the order of the
names inside a list reply is the sweep's).  The SET_DATAs write the same
bytes every replay, so the graphs replay on an unchanged tree.
``--side`` times one side alone (a kernel trace of it).

``--enforce-acl``: the sessions_mixed side serves with ``perms=`` (an address
a connection; csrc/kernels/tree_aclperm.hip), the other sides as ever.  On the
tree as built every node carries the open ACL: the check's fast path.
``--acl-vector`` first binds every node to one three-entry vector whose last
entry grants (a digest entry, an ip entry of another network, world:anyone):
every check walks the arena's bytes; nothing is denied either way, so all
sides still produce the same reply bytes.

``--setacl``: the cost of the SET_ACL pass (csrc/kernels/tree_setacl.hip) on
the sessions_mixed side alone, ``--runs`` runs a variant (a run: a captured
graph, the median of ``--reps`` replays): ``off`` (``setacl=False``: the
launches of the call without the argument, the number to hold against the
parent commit's ``--side new``), ``on, none`` (``setacl=True``, no SET_ACL
frame in the batch) and ``on, one a connection`` (every connection's first
frame is a SET_ACL of a leaf of its own with version -1, so every replay
applies it again)."""

import argparse
import os
import statistics
import struct
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
from zkmi import consts  # noqa: E402
from zkmi.ops import _lib  # noqa: E402
from zkmi.server.engine import (AclIdentity, GpuServer,  # noqa: E402
                                SessionSegments)
from zkmi.server.tree import GpuTree  # noqa: E402

I64, I32, U8 = torch.int64, torch.int32, torch.uint8
SHAPES = ((1024, 16), (8, 65536))


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        fn()
    return g


def connection(rng, r, nodes, fanout, data):
    """The frames of one connection, xids from 1; returns (bytes, lists)."""
    op = consts.OP_CODES
    leaf = rng.integers(0, nodes, r)
    kind = rng.random(r)
    wr = rng.random(r) < 0.2
    ndirs = max(nodes // fanout, 1)
    out, lists = [], 0
    for k in range(r):
        v = int(leaf[k])
        path = b'/bench/d%06d/n%09d' % (v // fanout, v)
        if kind[k] < 0.1:
            path = b'/bench/d%06d' % (v % ndirs)
            body = struct.pack('>iii', k + 1, op['GET_CHILDREN2'],
                               len(path)) + path + b'\0'
            lists += 1
        elif kind[k] < 0.2:
            body = struct.pack('>iii', k + 1, op['GET_ACL'], len(path)) + path
        elif wr[k]:
            body = struct.pack('>iii', k + 1, op['SET_DATA'], len(path)) + \
                path + struct.pack('>i', len(data)) + data + \
                struct.pack('>i', -1)
        else:
            body = struct.pack('>iii', k + 1, op['GET_DATA'], len(path)) + \
                path + b'\0'
        out.append(struct.pack('>i', len(body)) + body)
    return b''.join(out), lists


def setacl_frame(xid, path):
    """A SET_ACL of ``path`` to the open ACL, any version."""
    vec = struct.pack('>iii', 1, 31, 5) + b'world' + \
        struct.pack('>i', 6) + b'anyone'
    body = struct.pack('>iii', xid, consts.OP_CODES['SET_ACL'], len(path)) + \
        path + vec + struct.pack('>i', -1)
    return struct.pack('>i', len(body)) + body


def setacl_variants(tree, S, r, a, dev, conns, sids, slots, out_cap, perms):
    """--setacl: the three variants, ``a.runs`` runs each."""
    def batch(parts):
        cuts = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
        return (dev_bytes(b''.join(parts), dev), int(cuts[-1]),
                SessionSegments(torch.tensor(cuts, dtype=I64, device=dev),
                                torch.tensor(sids, dtype=I64, device=dev),
                                torch.tensor(slots, dtype=I32, device=dev)))
    plain = [c[0] for c in conns]
    withset = []
    for s_, p in enumerate(plain):
        first = 4 + struct.unpack_from('>i', p, 0)[0]
        v = (s_ * 977) % a.nodes
        withset.append(setacl_frame(
            1, b'/bench/d%06d/n%09d' % (v // a.fanout, v)) + p[first:])
    srv = GpuServer(tree, S * r, out_cap, seq_order=False)
    print('S %5d x r %6d = %7d requests' % (S, r, S * r), flush=True)
    for name, parts, kw in (
            ('off', plain, {}),
            ('on, none', plain, {'setacl': True}),
            ('on, one a connection', withset, {'setacl': True})):
        rx, n, segs = batch(parts)
        _, total, err, ft = srv.serve_sessions_mixed(rx, n, segs, perms=perms,
                                                     **kw)
        torch.cuda.synchronize()
        assert int(err.item()) == 0 and int(ft.count.item()) == S * r
        meds = []
        for _ in range(a.runs):
            g = graph_of(lambda: srv.serve_sessions_mixed(
                rx, n, segs, perms=perms, **kw))
            meds.append(timed(g.replay, a.reps)[0])
            del g
        print('  %-22s %s us  (range %.1f .. %.1f, reply %.2f MB)' % (
            name, ' '.join('%.1f' % m for m in meds), min(meds), max(meds),
            int(total.item()) / 1e6), flush=True)
    st = srv.setacl_stats()
    assert st['applied'] > 0 and st['unreached'] == 0 and \
        st['store_full'] == 0, st
    del srv
    torch.cuda.empty_cache()


def bind_vector(tree):
    """Every node's ACL word -> one three-entry vector, its bytes put on
    the store's arena top (the intern index is not told: no CREATE of the
    benchmark carries it)."""
    def entry(perms, scheme, ident):
        return struct.pack('>ii', perms, len(scheme)) + scheme + \
            struct.pack('>i', len(ident)) + ident
    vec = struct.pack('>i', 3) + entry(31, b'digest', b'bench:kQq8nOxk1N') \
        + entry(31, b'ip', b'10.9.0.0/16') + entry(31, b'world', b'anyone')
    node_acl, arena, _, _, ctr = tree.acl
    top = int(ctr[_lib.AC_TOP].item())
    assert top + len(vec) <= arena.numel()
    arena[top:top + len(vec)] = dev_bytes(vec, arena.device)
    ctr[_lib.AC_TOP] = top + len(vec)
    ctr[_lib.AC_OLD_TOP] = top + len(vec)
    node_acl.fill_((top << 24) | len(vec))


def dev_bytes(raw, dev):
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)


def shape(tree, S, r, a, dev):
    rng = np.random.default_rng(1000 * S + r)
    conns = [connection(rng, r, a.nodes, a.fanout, b'x' * 100)
             for _ in range(S)]
    parts = [c[0] for c in conns]
    per_list = a.fanout * 20 + 256          # a directory's reply, rounded up
    cuts = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    n = int(cuts[-1])
    rx = dev_bytes(b''.join(parts), dev)
    sids = [(1 << 56) | (s + 1) for s in range(S)]
    slots = [s % 64 for s in range(S)]
    segs = SessionSegments(torch.tensor(cuts, dtype=I64, device=dev),
                           torch.tensor(sids, dtype=I64, device=dev),
                           torch.tensor(slots, dtype=I32, device=dev))
    out_cap = S * r * 256 + sum(c[1] for c in conns) * per_list + (1 << 16)
    perms = None
    if a.enforce_acl:
        # 10.1.x.y, a connection an address
        perms = AclIdentity(torch.tensor(
            [0x0A010000 + (s & 0xFFFF) for s in range(S)], dtype=I32,
            device=dev))
    if a.setacl:
        setacl_variants(tree, S, r, a, dev, conns, sids, slots, out_cap,
                        perms)
        return
    one = GpuServer(tree, S * r, out_cap, seq_order=False)
    _, total, err, ft = one.serve_sessions_mixed(rx, n, segs, perms=perms)
    torch.cuda.synchronize()
    T = int(total.item())
    st = one.session_stats()
    assert int(err.item()) == 0 and st['bad'] == 0, (int(err.item()), st)
    assert int(ft.count.item()) == S * r
    head = 'S %5d x r %6d = %7d requests  reply %8.2f MB ' % (
        S, r, S * r, T / 1e6)
    res = {}
    if a.side in ('all', 'new'):
        g = graph_of(lambda: one.serve_sessions_mixed(rx, n, segs,
                                                      perms=perms))
        res['sessions_mixed'] = timed(g.replay, a.reps)
        del g
        if perms is not None:
            st = one.acl_enforce_stats()
            assert st['denied'] == 0 and st['checked'] > 0, st
    if a.side in ('all', 'floor'):
        _, total, err, _ = one.serve_mixed(rx, n, session=sids[0],
                                           wslot=slots[0])
        torch.cuda.synchronize()
        assert int(err.item()) == 0 and int(total.item()) == T
        g = graph_of(lambda: one.serve_mixed(rx, n, session=sids[0],
                                             wslot=slots[0]))
        res['floor'] = timed(g.replay, a.reps)
        del g
    t_cap = 0.0
    if a.side in ('all', 'serves'):
        ref = GpuServer(tree, r, r * 256 + max(c[1] for c in conns) *
                        per_list + (1 << 16), seq_order=False)
        each = [dev_bytes(p, dev) for p in parts]
        totals = torch.zeros(S, dtype=I64, device=dev)

        def serves():
            for s in range(S):
                _, total, _, _ = ref.serve_mixed(each[s], len(parts[s]),
                                                 session=sids[s],
                                                 wslot=slots[s])
                totals[s:s + 1].copy_(total)

        serves()
        torch.cuda.synchronize()
        assert int(totals.sum().item()) == T, (int(totals.sum().item()), T)
        off = one.seg.rep_off.cpu().numpy()
        assert np.array_equal(np.diff(off), totals.cpu().numpy())
        t0 = time.time()
        g = graph_of(serves)
        t_cap = time.time() - t0
        res['serves'] = timed(g.replay, a.reps)
        del g, ref, each
    print(head + '  '.join('%s %.1f us (min %.1f, max %.1f)' % ((k,) + v)
                           for k, v in res.items()), end='')
    if 'sessions_mixed' in res and 'floor' in res:
        print('  over the floor %+.1f us' % (res['sessions_mixed'][0] -
                                             res['floor'][0]), end='')
    if 'sessions_mixed' in res and 'serves' in res:
        print('  ratio to the serves %.4f  (capture %.1f s)' % (
            res['sessions_mixed'][0] / res['serves'][0], t_cap), end='')
    print(flush=True)
    del one
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--fanout', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--shape', action='append',
                    help='SxR (default: %s)' % ', '.join(
                        '%dx%d' % s for s in SHAPES))
    ap.add_argument('--side', default='all',
                    choices=('all', 'new', 'floor', 'serves'))
    ap.add_argument('--enforce-acl', action='store_true',
                    help='serve the sessions_mixed side with perms=')
    ap.add_argument('--acl-vector', action='store_true',
                    help='every node carries a three-entry ACL vector')
    ap.add_argument('--setacl', action='store_true',
                    help='the SET_ACL pass: off / on without / on with one '
                    'SET_ACL a connection, --runs runs each')
    ap.add_argument('--runs', type=int, default=5)
    a = ap.parse_args()
    shapes = SHAPES if not a.shape else \
        [tuple(int(x) for x in s.split('x')) for s in a.shape]
    dev = torch.device('cuda', 0)
    tree = GpuTree(a.nodes, 100, fanout=a.fanout, device=dev,
                   acl_cap=1 << 12, watch_cap=1 << 16)
    print('tree: %d znodes, fanout %d, an ACL table and a watch table; ~10 %% '
          'GET_CHILDREN2, ~10 %% GET_ACL, the rest 80 %% GET_DATA / 20 %% '
          'SET_DATA; captured graphs, median of %d' % (
              a.nodes, a.fanout, a.reps), flush=True)
    if a.acl_vector:
        bind_vector(tree)
    if a.enforce_acl or a.acl_vector:
        print('enforce-acl %s, %s' % (
            'on' if a.enforce_acl else 'off',
            'a three-entry vector a node' if a.acl_vector else
            'the open ACL everywhere'), flush=True)
    for S, r in shapes:
        shape(tree, S, r, a, dev)
    return 0


if __name__ == '__main__':
    sys.exit(main())
