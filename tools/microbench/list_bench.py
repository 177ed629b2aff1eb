"""List-path microbenchmark: GET_CHILDREN2 batches served from the HBM tree
(csrc/kernels/tree_list.hip, GpuServer.serve_list) on a 1M-znode tree with
1000 children a directory.  Three batches:

  distinct   one request per directory, up to 1024 (1000 on this tree)
  dup        8192 requests over the 1000 directories (the duplicate path)
  hot        1024 requests over 8 directories (the contended accumulators)

For each: a whole ListPipeline step (serve_list + K1 + reply decode + name
expansion + device check) and the server half alone, as captured graphs
(CUDA events, median), the reply bytes, and beside them one
``tree_digest`` — the existing single sweep over the same node table — as
the yardstick for a sweep.  ``--eager`` times the uncaptured calls too."""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
from zkmi.ops import _lib  # noqa: E402
from zkmi.bench.synthetic import ListPipeline  # noqa: E402
from zkmi.server.tree import GpuTree  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--fanout', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--eager', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    tree = GpuTree(a.nodes, 100, fanout=a.fanout, device=dev)
    ndirs = tree.leaf0 - 1
    dig = torch.zeros(4, dtype=torch.int64, device=dev)
    L = _lib.lib()
    print('tree: %d znodes, %d directories of %d; node table %d slots'
          % (a.nodes, ndirs, a.fanout, tree.cap), flush=True)
    for name, batch, nd in (('distinct', min(1024, ndirs), ndirs),
                            ('dup', 8192, ndirs), ('hot', 1024, 8)):
        pipe = ListPipeline(tree, batch, ndirs=nd)
        acc = pipe.step()
        torch.cuda.synchronize()
        ok = int(acc.item()) == batch and int(pipe.bad.item()) == 0
        if not ok:
            print('list %-8s CHECK FAILED %r' % (name, pipe.diagnose()))
            return 1
        out_bytes = int(pipe.last[3].item())
        acc = torch.zeros(1, dtype=torch.int64, device=dev)
        g_step = pipe.capture(acc)
        g_srv = graph_of(pipe.server_step)
        g_dig = graph_of(lambda: L.tree_digest(tree.tensors, dig))
        t_step = timed(g_step.replay, a.reps)
        t_srv = timed(g_srv.replay, a.reps)
        t_dig = timed(g_dig.replay, a.reps)
        torch.cuda.synchronize()
        ok = int(pipe.bad.item()) == 0
        line = ('list %-8s requests=%-5d dirs=%-5d reply=%8.2f MB  '
                'step %8.1f us  server %8.1f us  digest %7.1f us  '
                'server/digest %5.2f  %s'
                % (name, batch, pipe.ndirs, out_bytes / 1e6, t_step, t_srv,
                   t_dig, t_srv / t_dig, 'ok' if ok else 'CHECK FAILED'))
        if a.eager:
            line += '  eager: step %.1f us server %.1f us' % (
                timed(lambda: pipe.step(acc=acc), a.reps),
                timed(pipe.server_step, a.reps))
        print(line, flush=True)
        del pipe, g_step, g_srv, g_dig
        torch.cuda.empty_cache()
    return 0


if __name__ == '__main__':
    sys.exit(main())
