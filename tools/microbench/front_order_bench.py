"""What the ordered tick of the GPU server's front end buys and costs
(zkmi/server/gpu.py ``GpuZKServer(order_passes=P)``).

1. Through the sockets, with the real client: the wall time for one client
   to complete W pipelined sets — on W distinct paths and on one path — and
   for C clients to complete a create / set / get / delete chain on paths of
   their own, with ``order_passes`` 0 (one write a connection a tick), 4 and
   8.  The median of ``--reps`` runs and their spread, and the ticks a run
   took.

2. Without the sockets: the serve phase of a read-only tick (S connections x
   f GET_DATA frames, ``profiles/front_end.md``'s shapes) with the unordered
   serve and the ordered one with deferral, device events around the phase,
   and the host's wall time for issuing it: what ordering adds to a tick that
   has nothing to order."""

import argparse
import os
import statistics
import sys
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
from zkmi import Client, jute  # noqa: E402
from zkmi.server.engine import (GpuServer, OrderDefer,  # noqa: E402
                                SessionSegments)
from zkmi.server.tree import GpuTree  # noqa: E402
from zkmi.server.gpu import GpuZKServer  # noqa: E402

I64, I32, U8 = torch.int64, torch.int32, torch.uint8
D0 = '/bench/d000000'


def _pipeline(c, calls, timeout=60):
    """Issue ``calls`` from one turn of the client's loop; wait for all."""
    left = [len(calls)]
    errs = []
    done = threading.Event()
    lock = threading.Lock()

    def cb(err=None, *res):
        with lock:
            if err is not None:
                errs.append(err.code)
            left[0] -= 1
            if left[0] == 0:
                done.set()

    def issue():
        for method, args in calls:
            getattr(c, method)(*(tuple(args) + (cb,)))
    c.loop.run(issue)
    if not done.wait(timeout):
        raise RuntimeError('the pipeline did not complete')
    return errs


def sockets(a, dev):
    print('through the sockets: wall ms to complete, median of %d (min .. '
          'max), ticks of the median-most run' % a.reps, flush=True)
    for P in (0, 4, 8):
        tree = GpuTree(2000, 100, fanout=100, device=dev, watch_cap=4096,
                       acl_cap=64, scratch=1 << 22)
        srv = GpuZKServer(tree, cap_frames=4096, out_cap=1 << 22,
                          max_conns=128, order_passes=P)
        try:
            cs = [Client({'servers': srv.servers()}) for _ in range(a.conns)]
            for c in cs:
                c.wait_connected(10)
            W = a.writes
            leaves = [D0 + '/n%09d' % (k % 100) for k in range(W)]
            if W > 100:
                leaves = ['/bench/d%06d/n%09d' % (k // 100, k)
                          for k in range(W)]
            work = {
                '%d sets, distinct paths' % W:
                    lambda: [_pipeline(cs[0], [('set', (p, b'v', -1))
                                               for p in leaves])],
                '%d sets, one path' % W:
                    lambda: [_pipeline(cs[0], [('set', (leaves[0], b'v', -1))
                                               for _ in range(W)])],
            }

            def mix():
                out = [None] * len(cs)

                def go(k, c):
                    calls = []
                    for j in range(4):
                        p = D0 + '/m%03d_%d' % (k, j)
                        calls += [('create', (p, b'c', {})),
                                  ('set', (p, b'dd', -1)), ('get', (p,)),
                                  ('delete', (p, -1))]
                    out[k] = _pipeline(c, calls)
                ts = [threading.Thread(target=go, args=(k, c))
                      for k, c in enumerate(cs)]
                for t in ts:
                    t.start()
                for t in ts:
                    t.join()
                return out
            work['%d connections x 4 chains of 4' % len(cs)] = mix
            for name, fn in work.items():
                fn()                                      # warm
                runs = []
                for _ in range(a.reps):
                    t0 = srv.stats()['ticks']
                    w0 = time.perf_counter()
                    errs = fn()
                    w = (time.perf_counter() - w0) * 1e3
                    assert not any(errs), errs
                    runs.append((w, srv.stats()['ticks'] - t0))
                runs.sort()
                med = runs[len(runs) // 2]
                print('  order_passes %d  %-34s %8.2f (%7.2f .. %7.2f)  '
                      'ticks %d' % (P, name, med[0], runs[0][0], runs[-1][0],
                                    med[1]), flush=True)
            st = srv.stats()
            print('  order_passes %d  deferred_frames %d  max_writes_per_tick '
                  '%d  order_max_rank %d  order_scratch_full %d' % (
                      P, st['deferred_frames'], st['max_writes_per_tick'],
                      st['order_max_rank'], st['order_scratch_full']),
                  flush=True)
            for c in cs:
                c.close_sync(10)
        finally:
            srv.shutdown()
        if srv.error is not None:
            raise srv.error


def serve_phase(a, dev):
    print('the serve phase of a read-only tick, S connections x f GET_DATA '
          'frames: device us between events | host wall us to issue and '
          'finish it, medians of %d' % a.ticks, flush=True)
    tree = GpuTree(2000, 100, fanout=100, device=dev, watch_cap=4096,
                   acl_cap=64, scratch=1 << 22)
    for sh in a.shape or ['64,1', '64,16', '1024,16']:
        S, f = (int(x) for x in sh.split(','))
        parts = []
        for s in range(S):
            b = b''
            for j in range(f):
                i = (s * f + j) % 2000
                b += jute.frame(jute.encode_request({
                    'opcode': 'GET_DATA', 'xid': 1 + j, 'watch': False,
                    'path': '/bench/d%06d/n%09d' % (i // 100, i)}))
            parts.append(b)
        raw = b''.join(parts)
        cuts = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
        rx = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)
        segs = SessionSegments(
            torch.from_numpy(cuts.astype(np.int64)).to(dev),
            torch.tensor([(1 << 56) | (s + 1) for s in range(S)], dtype=I64,
                         device=dev),
            torch.tensor([s if s < 64 else -1 for s in range(S)], dtype=I32,
                         device=dev))
        frames = S * f
        line = 'S %5d x f %3d:' % (S, f)
        for P in (0, 4, 8):
            srv = GpuServer(tree, max(frames, 64), frames * 256 + (1 << 16))
            df = OrderDefer(S, dev) if P else None
            kw = dict(ordered=True, passes=P, defer=df) if P else {}

            def tick():
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                e0.record()
                srv.serve_sessions_mixed(rx, len(raw), segs, resume=True,
                                         close=True, **kw)
                e1.record()
                torch.cuda.synchronize()
                return (e0.elapsed_time(e1) * 1e3,
                        (time.perf_counter() - w0) * 1e6)
            for _ in range(3):
                tick()
            ts = [tick() for _ in range(a.ticks)]
            if P:
                assert int(df.deferred.item()) == 0
            line += '  P=%d %7.1f | %7.1f' % (
                P, statistics.median(t[0] for t in ts),
                statistics.median(t[1] for t in ts))
            del srv
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--writes', type=int, default=256)
    ap.add_argument('--conns', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ticks', type=int, default=20)
    ap.add_argument('--shape', action='append', help='S,f of the serve phase')
    ap.add_argument('--skip-sockets', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    if not a.skip_sockets:
        sockets(a, dev)
    serve_phase(a, dev)
    return 0


if __name__ == '__main__':
    sys.exit(main())
