"""Session-batch microbenchmark: GpuServer.serve_sessions (csrc/kernels/
tree_sess.hip around the serve's MS instances) on a 1M-znode tree.

S connections send r requests each, 80 % GET_DATA and 20 % SET_DATA on random
leaves.  The two sides, captured graphs in the same run (CUDA events, median):

  sessions  ONE serve_sessions over the concatenated stream with the segment
            table (a session and a watcher slot a connection);
  serves    S serve(session=, wslot=) calls over the same bytes, a stream a
            connection, on a server sized for r frames.

Both sides produce the same reply bytes (checked).  The SET_DATAs write the
same bytes every replay, so the graphs replay on an unchanged tree.  With a
watch table (the default) both sides also expand and encode the batch's
notifications; ``--no-watch`` leaves them out."""

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
from zkmi.server.engine import GpuServer, SessionSegments  # noqa: E402
from zkmi.server.tree import GpuTree  # noqa: E402

I64, I32, U8 = torch.int64, torch.int32, torch.uint8
SHAPES = ((64, 16), (1024, 16), (4096, 4), (8, 65536))


def timed(fn, reps, warm=3):
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
    return statistics.median(ts)


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        fn()
    return g


def connection(rng, r, nodes, fanout, data):
    """The frames of one connection: xids from 1, 80 % GET_DATA, 20 %
    SET_DATA (version -1) on random leaves."""
    get, setd = consts.OP_CODES['GET_DATA'], consts.OP_CODES['SET_DATA']
    leaf = rng.integers(0, nodes, r)
    wr = rng.random(r) < 0.2
    out = []
    for k in range(r):
        v = int(leaf[k])
        path = b'/bench/d%06d/n%09d' % (v // fanout, v)
        if wr[k]:
            body = struct.pack('>iii', k + 1, setd, len(path)) + path + \
                struct.pack('>i', len(data)) + data + struct.pack('>i', -1)
        else:
            body = struct.pack('>iii', k + 1, get, len(path)) + path + b'\0'
        out.append(struct.pack('>i', len(body)) + body)
    return b''.join(out)


def dev_bytes(raw, dev):
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)


def shape(tree, S, r, a, dev):
    rng = np.random.default_rng(1000 * S + r)
    parts = [connection(rng, r, a.nodes, a.fanout, b'x' * 100)
             for _ in range(S)]
    cuts = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    rx = dev_bytes(b''.join(parts), dev)
    sids = [(1 << 56) | (s + 1) for s in range(S)]
    slots = [s % 64 for s in range(S)]
    segs = SessionSegments(torch.tensor(cuts, dtype=I64, device=dev),
                           torch.tensor(sids, dtype=I64, device=dev),
                           torch.tensor(slots, dtype=I32, device=dev))
    out_cap = S * r * 256 + (1 << 16)
    one = GpuServer(tree, S * r, out_cap, seq_order=False)
    ref = GpuServer(tree, r, r * 256 + (1 << 16), seq_order=False)
    each = [dev_bytes(p, dev) for p in parts]
    totals = torch.zeros(S, dtype=I64, device=dev)

    def serves():
        for s in range(S):
            _, total, _, _ = ref.serve(each[s], len(parts[s]),
                                       session=sids[s], wslot=slots[s])
            totals[s:s + 1].copy_(total)

    _, total, err, ft = one.serve_sessions(rx, int(cuts[-1]), segs)
    torch.cuda.synchronize()
    T = int(total.item())
    st = one.session_stats()
    assert int(err.item()) == 0 and st['bad'] == 0, st
    assert int(ft.count.item()) == S * r
    if a.no_serves:
        # (a kernel trace of the session side alone)
        g_one = graph_of(lambda: one.serve_sessions(rx, int(cuts[-1]), segs))
        print('S %5d x r %6d = %7d requests  reply %7.2f MB  serve_sessions '
              '%9.1f us' % (S, r, S * r, T / 1e6, timed(g_one.replay, a.reps)),
              flush=True)
        return
    serves()
    torch.cuda.synchronize()
    assert int(totals.sum().item()) == T, (int(totals.sum().item()), T)
    off = one.seg.rep_off.cpu().numpy()
    assert np.array_equal(np.diff(off), totals.cpu().numpy())
    t0 = time.time()
    g_one = graph_of(lambda: one.serve_sessions(rx, int(cuts[-1]), segs))
    g_ref = graph_of(serves)
    t_cap = time.time() - t0
    t_one = timed(g_one.replay, a.reps)
    t_ref = timed(g_ref.replay, a.reps)
    print('S %5d x r %6d = %7d requests  reply %7.2f MB  serve_sessions '
          '%9.1f us  %d serves %10.1f us  ratio %.4f  (capture %.1f s)'
          % (S, r, S * r, T / 1e6, t_one, S, t_ref, t_one / t_ref, t_cap),
          flush=True)
    del one, ref, each, g_one, g_ref
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--fanout', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--shape', action='append',
                    help='SxR (default: %s)' % ', '.join(
                        '%dx%d' % s for s in SHAPES))
    ap.add_argument('--no-watch', action='store_true')
    ap.add_argument('--no-serves', action='store_true',
                    help='time serve_sessions alone')
    a = ap.parse_args()
    shapes = SHAPES if not a.shape else \
        [tuple(int(x) for x in s.split('x')) for s in a.shape]
    dev = torch.device('cuda', 0)
    tree = GpuTree(a.nodes, 100, fanout=a.fanout, device=dev,
                   watch_cap=0 if a.no_watch else 1 << 16)
    print('tree: %d znodes, %s; 80 %% GET_DATA, 20 %% SET_DATA; captured '
          'graphs, median of %d' % (
              a.nodes, 'no watch table' if a.no_watch else 'a watch table',
              a.reps), flush=True)
    for S, r in shapes:
        shape(tree, S, r, a, dev)
    return 0


if __name__ == '__main__':
    sys.exit(main())
