"""Tree image microbenchmark: GpuTree.snapshot and GpuTree.load
(csrc/kernels/tree_snap.hip) on a 1M-znode tree of 100-byte nodes that a few
hundred MixPipeline steps have left with holes and recycled nodes.

  snapshot  snapshot(out=...) — sizes, two scans, digest, header, the two
            writer tiers — as a captured graph (CUDA events, median), with
            the image's size;
  copy      a torch device-to-device copy of the same byte count, the
            yardstick for the writer;
  load      GpuTree.load of that image end to end (allocation, header read,
            the device load, outcome read; wall clock), and the device load
            alone into the same tree emptied again, as a captured graph;
  rehash    the in-place index rebuild of the same tree (the index reset and
            tree_build), captured: the yardstick for the index-build part of
            a load.

All four in one process, one after the other."""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
from zkmi.ops import _lib  # noqa: E402
from zkmi.bench.synthetic import MixPipeline  # noqa: E402
from zkmi.server.tree import GpuTree  # noqa: E402
from zkmi.utils import treeimage as TI  # noqa: E402

I64, U8 = torch.int64, torch.uint8


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
    ap.add_argument('--batch', type=int, default=98304)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--reps', type=int, default=30)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    tree = GpuTree(a.nodes, 100, device=dev, compact_free=True)
    pipe = MixPipeline(tree, a.batch, 100)
    ok = torch.zeros(1, dtype=I64, device=dev)
    for _ in range(a.steps):
        pipe.step(acc=ok)
    torch.cuda.synchronize()
    assert int(ok.item()) == pipe.n * a.steps, (int(ok.item()), pipe.n)
    dig = tree.digest()
    hwm = int(tree.counters[_lib.TC_NODES].item())
    print('tree: %d znodes of 100 bytes after %d mix steps of %d requests: '
          '%d live, node high-water mark %d (%d free below it), %d index '
          'entries in use, %d tombstones; captured graphs, median of %d'
          % (a.nodes, a.steps, pipe.n, dig[1], hwm, hwm - dig[1], dig[2],
             dig[3], a.reps), flush=True)

    img = tree.snapshot()
    T = img.numel()
    hd = TI.header(bytes(img[:64].cpu().numpy().tobytes()))
    assert hd['n'] == dig[1] and hd['digest'] == dig[0]
    out = torch.empty(T + 4096, dtype=U8, device=dev)
    g_snap = graph_of(lambda: tree.snapshot(out=out))
    torch.cuda.synchronize()
    assert torch.equal(out[:T], img)
    src = torch.randint(0, 256, (T,), dtype=U8, device=dev)
    dst = torch.empty(T, dtype=U8, device=dev)
    g_copy = graph_of(lambda: dst.copy_(src))
    t_snap = timed(g_snap.replay, a.reps)
    t_copy = timed(g_copy.replay, a.reps)
    print('snapshot  %d records, image %.1f MB (%.1f bytes a record)  '
          'snapshot(out) %8.1f us  %6.3f TB/s  torch copy %8.1f us  '
          '%6.3f TB/s  ratio %.2f'
          % (hd['n'], T / 1e6, T / hd['n'], t_snap, T / t_snap / 1e6, t_copy,
             T / t_copy / 1e6, t_snap / t_copy), flush=True)
    del src, dst

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t2 = GpuTree.load(img, device=dev)
    torch.cuda.synchronize()
    t_wall = (time.perf_counter() - t0) * 1e6
    assert t2.digest()[:2] == dig[:2]
    n = hd['n']
    ws = torch.empty(L.tree_load_workspace(n), dtype=U8, device=dev)
    status = torch.zeros(2, dtype=I64, device=dev)

    def reload():
        t2.ht.zero_()
        t2.counters.zero_()
        _lib.tree_load(t2.tensors, None, img, T, n, 128, ws, status)

    def rehash():
        L.tree_ht_reset(t2.tensors)
        L.tree_build(t2.tensors, 0, n)

    g_load = graph_of(reload)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, -1] and t2.digest()[:2] == dig[:2]
    g_rehash = graph_of(rehash)
    torch.cuda.synchronize()
    assert t2.digest()[:3] == (dig[0], dig[1], n)
    t_load = timed(g_load.replay, a.reps)
    t_rehash = timed(g_rehash.replay, a.reps)
    print('load      GpuTree.load end to end %10.1f us (wall, once)  device '
          'load (index reset included) %8.1f us  %6.3f TB/s of image  '
          'rehash of the same tree %8.1f us  ratio %.2f'
          % (t_wall, t_load, T / t_load / 1e6, t_rehash, t_load / t_rehash),
          flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
