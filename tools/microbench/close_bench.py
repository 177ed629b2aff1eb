"""Ending K sessions: ONE GpuServer.close_sessions (csrc/kernels/
tree_close.hip: one sweep of the node table, whatever K) against the only
other way to do the same work, a loop of K GpuServer.expire calls
(tree_expire_k + tree_finish_k a session: K sweeps, 2 K launches), on the
1M-znode tree.

K sessions own E ephemerals each, spread over the tree's directories.  They
are created, untimed, by one session batch (serve_sessions, a segment a
session) before every timed call; the timed call is device events around the
whole close (the list's upload included) and ends in a synchronise.  The two
sides alternate, ``--runs`` runs a side (a run: the median of ``--reps``
create + close rounds), and every round checks that K * E nodes went.  The
line gives the median run of each side with the smallest and the largest.

``--watch``: a tree with a watch table (the watcher-drop sweep and the fire
instance of the removal; the loop's expire then drops, records and encodes
per session).  ``--side`` times one side alone (a kernel trace of it)."""

import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
from zkmi import jute  # noqa: E402
from zkmi.server.engine import GpuServer, SessionSegments  # noqa: E402
from zkmi.server.tree import GpuTree  # noqa: E402

I64, I32 = torch.int64, torch.int32
KS = (1, 16, 256, 4096)


def sid_of(k):
    return (1 << 56) | (k + 1)


def stream(K, E, ndirs):
    """The create batch: segment k = session k's E EPHEMERAL creates.
    -> (bytes, segment starts)."""
    parts = []
    for k in range(K):
        b = b''
        for j in range(E):
            b += jute.frame(jute.encode_request({
                'opcode': 'CREATE', 'xid': 1 + j,
                'path': '/bench/d%06d/e%07d_%03d' % ((k * E + j) % ndirs, k,
                                                     j),
                'data': b'e', 'acl': jute.DEFAULT_ACL,
                'flags': ['EPHEMERAL']}))
        parts.append(b)
    cuts = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    return b''.join(parts), cuts


def one_k(tree, K, E, a, dev):
    ndirs = (a.nodes + a.fanout - 1) // a.fanout
    raw, cuts = stream(K, E, ndirs)
    n = len(raw)
    rx = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)
    sids_h = [sid_of(k) for k in range(K)]
    slots_h = [k % 64 for k in range(K)]
    segs = SessionSegments(
        torch.tensor(cuts, dtype=I64, device=dev),
        torch.tensor(sids_h, dtype=I64, device=dev),
        torch.full((K,), -1, dtype=I32, device=dev))
    frames = K * E
    srv = GpuServer(tree, max(frames, 64), frames * 64 + (1 << 16),
                    seq_order=False)
    sids_cpu = torch.tensor(sids_h, dtype=I64).pin_memory()
    slots_cpu = torch.tensor(slots_h, dtype=I32).pin_memory()
    watch = tree.watch is not None
    removed1 = torch.zeros(1, dtype=I64, device=dev)

    def born():
        srv.serve_sessions(rx, n, segs)
        torch.cuda.synchronize()

    def batch():
        sids = sids_cpu.to(dev, non_blocking=True)
        ws = slots_cpu.to(dev, non_blocking=True) if watch else None
        return srv.close_sessions(sids, ws).sum()

    def loop():
        removed1.zero_()
        for k in range(K):
            srv.expire(sids_h[k], wslot=slots_h[k] if watch else None,
                       removed=removed1)
        return removed1

    def run(fn, reps):
        ts = []
        for _ in range(reps):
            born()
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            got = fn()
            t1.record()
            t1.synchronize()
            ts.append(t0.elapsed_time(t1) * 1e3)
            assert int(got.item()) == frames, (int(got.item()), frames)
        return statistics.median(ts)

    sides = [s for s in (('batch', batch), ('loop', loop))
             if a.side in ('all', s[0])]
    live0 = tree.digest()[1]
    for _, fn in sides:                              # warm-up, both sides
        run(fn, 1)
    res = {name: [] for name, _ in sides}
    for _ in range(a.runs):
        for name, fn in sides:
            reps = a.reps if name == 'batch' or K <= 256 else \
                max(a.reps // 3, 1)
            res[name].append(run(fn, reps))
    assert tree.digest()[1] == live0
    line = 'K %5d x E %3d = %6d nodes ' % (K, E, frames)
    for name, _ in sides:
        v = sorted(res[name])
        line += ' %s %.1f us (min %.1f, max %.1f)' % (
            name, statistics.median(v), v[0], v[-1])
    if len(sides) == 2:
        line += '  loop / batch %.1f' % (statistics.median(res['loop']) /
                                         statistics.median(res['batch']))
    print(line, flush=True)
    del srv
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--fanout', type=int, default=1000)
    ap.add_argument('--eph', type=int, default=16,
                    help='ephemerals a session (E)')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('-k', action='append', type=int,
                    help='sessions (default: %s)' % ', '.join(map(str, KS)))
    ap.add_argument('--watch', action='store_true')
    ap.add_argument('--side', default='all', choices=('all', 'batch', 'loop'))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    kw = {'watch_cap': 1 << 18} if a.watch else {}
    tree = GpuTree(a.nodes, 100, fanout=a.fanout, device=dev, **kw)
    print('tree: %d znodes, fanout %d%s; K sessions of E ephemerals; device '
          'events around the whole close; %d alternating runs a side, a run '
          'the median of %d create + close rounds (loop at K > 256: %d)' % (
              a.nodes, a.fanout, ', a watch table' if a.watch else '',
              a.runs, a.reps, max(a.reps // 3, 1)), flush=True)
    for K in (a.k or KS):
        one_k(tree, K, a.eph, a, dev)
    return 0


if __name__ == '__main__':
    sys.exit(main())
