"""The SET_WATCHES catch-up of a session batch: GpuServer.serve_sessions(
resume=True) (csrc/kernels/tree_resume.hip) against the only other way to do
the same work, S calls of serve(resume=True) (csrc/kernels/tree_watch.hip
wt_resume_k: one workgroup, thread 0 lists every frame's paths), on a tree
with a watch table.

S connections send one SET_WATCHES frame of P paths each (the reconnect
storm's first frames).  The eight outcomes of the session rule (three of a
data watch, two of an exist watch, three of a child watch) come in about
equal shares: relZxid is the zxid of the middle static node, so a listed leaf
above it reads as changed (data and child lists alike) and one below it is
re-armed; names the tree does not hold are the deleted and the still-missing
ones.  Two sides, timed with device events around the whole call (median
after warm-up calls; the single-session side allocates its buffers in every
call, as the parent does):

  batch    ONE serve_sessions(resume=True) over the concatenated stream;
  singles  S serve(resume=True) calls over the same bytes, a stream and a
           watcher slot a connection.

Both find the same number of events and re-arm the same number of watches
(checked).  ``--side`` times one side alone (a kernel trace of it)."""

import argparse
import os
import statistics
import struct
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
from zkmi.server.engine import GpuServer, SessionSegments  # noqa: E402
from zkmi.server.tree import GpuTree  # noqa: E402

I64, I32, U8 = torch.int64, torch.int32, torch.uint8
SHAPES = ((1024, 64), (8, 65536))
SET_WATCHES = 101


def timed(fn, reps, warm):
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


def connection(rng, P, nodes, fanout, rel):
    """One SET_WATCHES frame of P paths, the eight outcomes in equal shares."""
    leaf0 = 1 + (nodes + fanout - 1) // fanout          # node of leaf 0
    cut = max(rel - leaf0, 1)                           # leaves below: older

    def leaf(v):
        return b'/bench/d%06d/n%09d' % (v // fanout, v)

    def gone(v):
        return b'/bench/d%06d/gone%08d' % (v % 64, v)

    kind = rng.integers(0, 8, P)
    old = rng.integers(0, cut, P)
    new = rng.integers(cut, nodes, P)
    lists = [[], [], []]
    for k in range(P):
        o, n = int(old[k]), int(new[k])
        g, path = ((0, gone(n)), (0, leaf(n)), (0, leaf(o)), (1, leaf(o)),
                   (1, gone(o)), (2, gone(n)), (2, leaf(n)),
                   (2, leaf(o)))[kind[k]]
        lists[g].append(path)
    body = struct.pack('>iiq', -8, SET_WATCHES, rel)
    for ls in lists:
        body += struct.pack('>i', len(ls)) + b''.join(
            struct.pack('>i', len(p)) + p for p in ls)
    return struct.pack('>i', len(body)) + body


def dev_bytes(raw, dev):
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)


def shape(tree, S, P, a, dev):
    rng = np.random.default_rng(1000 * S + P)
    rel = tree.n_static // 2
    parts = [connection(rng, P, a.nodes, a.fanout, rel) for _ in range(S)]
    cuts = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    n = int(cuts[-1])
    rx = dev_bytes(b''.join(parts), dev)
    slots = [s % 64 for s in range(S)]
    segs = SessionSegments(torch.tensor(cuts, dtype=I64, device=dev),
                           torch.zeros(S, dtype=I64, device=dev),
                           torch.tensor(slots, dtype=I32, device=dev))
    cap = max(S, 64)
    head = 'S %5d x P %6d = %7d paths  %7.2f MB ' % (S, P, S * P, n / 1e6)
    res, st = {}, None
    if a.side in ('all', 'batch'):
        one = GpuServer(tree, cap, cap * 64 + (1 << 16), seq_order=False)

        def batch():
            one.serve_sessions(rx, n, segs, resume=True)

        batch()
        torch.cuda.synchronize()
        st = one.resume_stats()
        assert st['listed'] == S * P and st['dropped'] == 0 and \
            st['encode_err'] == 0 and st['events'] == st['events_written'], st
        res['batch'] = timed(batch, a.reps, 3)
        del one
    if a.side in ('all', 'singles'):
        ref = GpuServer(tree, 64, 1 << 16, seq_order=False)
        each = [dev_bytes(p, dev) for p in parts]
        tot = torch.zeros(4, dtype=I64, device=dev)

        def singles():
            tot.zero_()
            for s in range(S):
                ref.serve(each[s], len(parts[s]), wslot=slots[s], resume=True)
                tot.add_(ref.rs_out)

        singles()
        torch.cuda.synchronize()
        t = tot.cpu().tolist()
        assert t[3] == 0 and t[0] == t[2], t
        if st is not None:
            assert (t[2], t[1]) == (st['events'], st['rearmed']), (t, st)
        res['singles'] = timed(singles, max(a.reps // 5, 3), 1)
        del ref, each
    print(head + '  '.join('%s %.1f us (min %.1f, max %.1f)' % ((k,) + v)
                           for k, v in res.items()), end='')
    if st is not None:
        print('  events %d rearmed %d' % (st['events'], st['rearmed']), end='')
    if 'batch' in res and 'singles' in res:
        print('  ratio to the singles %.5f' % (res['batch'][0] /
                                               res['singles'][0]), end='')
    print(flush=True)
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--fanout', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--shape', action='append',
                    help='SxP (default: %s)' % ', '.join(
                        '%dx%d' % s for s in SHAPES))
    ap.add_argument('--side', default='all',
                    choices=('all', 'batch', 'singles'))
    a = ap.parse_args()
    shapes = SHAPES if not a.shape else \
        [tuple(int(x) for x in s.split('x')) for s in a.shape]
    dev = torch.device('cuda', 0)
    tree = GpuTree(a.nodes, 100, fanout=a.fanout, device=dev,
                   watch_cap=1 << 21)
    print('tree: %d znodes, fanout %d, a watch table; one SET_WATCHES frame '
          'of P paths a connection, the outcomes in equal shares; device '
          'events around the call, median of %d (singles: of %d)' % (
              a.nodes, a.fanout, a.reps, max(a.reps // 5, 3)), flush=True)
    for S, P in shapes:
        shape(tree, S, P, a, dev)
    return 0


if __name__ == '__main__':
    sys.exit(main())
