"""Mixed-batch microbenchmark: GpuServer.serve_mixed (csrc/kernels/
tree_mix.hip around the three serve engines) on a 1M-znode tree.

  server   the server half of serve_mixed on a batch of mixed ops (the
           shares are printed), as a captured graph (CUDA events, median),
           beside the sum of the three existing entry points — serve,
           serve_acl, serve_list — over the same requests split on the host,
           captured together in the same run; their ratio.
  idle     the same batch with the list and GET_ACL requests replaced by
           GET_DATA: serve_mixed against serve, the cost of the two engines
           and the split / merge that have nothing to do.
  copy     the merge alone (sizes, scan, total, the two copy kernels) over
           synthetic streams, one per tier of the copy, in bytes per second
           beside a device-to-device torch copy of the same byte count.

The batch's SET_DATAs write the same bytes every replay, so the graphs
replay on an unchanged tree."""

import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
from zkmi import jute  # noqa: E402
from zkmi.ops import _lib  # noqa: E402
from zkmi.server.engine import GpuServer  # noqa: E402
from zkmi.server.tree import GpuTree  # noqa: E402

I64, I32, U8 = torch.int64, torch.int32, torch.uint8
# op shares of the batch, per 100 requests
SHARES = (('GET_DATA', 60), ('EXISTS', 10), ('SET_DATA', 10), ('SYNC', 2),
          ('GET_ACL', 12), ('GET_CHILDREN2', 3), ('GET_CHILDREN', 3))


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


def requests(batch, nodes, fanout, idle=False, seed=1):
    """The batch's packets: ops in the SHARES' proportions, interleaved."""
    ops = [op for op, share in SHARES for _ in range(share)]
    rng = np.random.default_rng(seed)
    ops = [ops[i] for i in rng.permutation(100)]
    ndirs = nodes // fanout
    leaf = rng.permutation(nodes)
    pk = []
    for k in range(batch):
        op = ops[k % 100]
        if idle and op in ('GET_ACL', 'GET_CHILDREN2', 'GET_CHILDREN'):
            op = 'GET_DATA'
        v = int(leaf[k % nodes])
        path = '/bench/d%06d/n%09d' % (v // fanout, v)
        p = {'xid': k + 1, 'opcode': op, 'path': path}
        if op in ('GET_CHILDREN2', 'GET_CHILDREN'):
            p['path'] = '/bench/d%06d' % (v % ndirs)
        if op == 'SET_DATA':
            p.update(data=b'x' * 100, version=-1)
        pk.append(p)
    return pk


def stream(pk, dev):
    raw = b''.join(jute.frame(jute.encode_request(p)) for p in pk)
    a = np.frombuffer(raw or b'\0', np.uint8).copy()
    return torch.from_numpy(a).to(dev), len(raw)


def server_half(tree, batch, a, dev):
    out_cap = 64 << 20
    pk = requests(batch, a.nodes, a.fanout)
    idle = requests(batch, a.nodes, a.fanout, idle=True)
    cls = {'GET_ACL': 1, 'GET_CHILDREN': 2, 'GET_CHILDREN2': 2}
    part = [[p for p in pk if cls.get(p['opcode'], 0) == c] for c in range(3)]
    print('batch: %d requests; shares per 100: %s' % (
        batch, ', '.join('%s %d' % s for s in SHARES)))
    print('classes: serve %d, GET_ACL %d, list %d' % tuple(map(len, part)))
    mixed = GpuServer(tree, batch, out_cap, seq_order=False)
    ref = GpuServer(tree, batch, out_cap, seq_order=False)
    rx, n = stream(pk, dev)
    rxi, ni = stream(idle, dev)
    parts = [stream(p, dev) for p in part]

    def three():
        ref.serve(*parts[0])
        ref.serve_acl(*parts[1])
        ref.serve_list(*parts[2])

    _, total, err, _ = mixed.serve_mixed(rx, n)
    torch.cuda.synchronize()
    T = int(total.item())
    assert int(err.item()) == 0 and T > 0
    three()
    torch.cuda.synchronize()
    sums = sum(int(ref_total.item()) for ref_total in (
        ref.total_err[0], ref.acl_total_err[0], ref.list_total_err[0]))
    assert sums == T, (sums, T)
    g_mixed = graph_of(lambda: mixed.serve_mixed(rx, n))
    g_three = graph_of(three)
    g_idle = graph_of(lambda: mixed.serve_mixed(rxi, ni))
    g_serve = graph_of(lambda: ref.serve(rxi, ni))
    t_mixed = timed(g_mixed.replay, a.reps)
    t_three = timed(g_three.replay, a.reps)
    t_idle = timed(g_idle.replay, a.reps)
    t_serve = timed(g_serve.replay, a.reps)
    print('server  reply %.2f MB  serve_mixed %8.1f us  serve + serve_acl + '
          'serve_list %8.1f us  ratio %.3f'
          % (T / 1e6, t_mixed, t_three, t_mixed / t_three), flush=True)
    print('idle    (lists and GET_ACLs replaced by GET_DATA)  serve_mixed '
          '%8.1f us  serve %8.1f us  idle engines + split + merge %8.1f us'
          % (t_idle, t_serve, t_idle - t_serve), flush=True)


def copy_tiers(a, dev):
    small, wave = _lib.tree_mix_bounds()
    print('copy tiers: <= %d B eight lanes a reply, <= %d B a wave a reply, '
          'past it the whole grid' % (small, wave))
    for name, size, count in (('small', 192, 1 << 20),
                              ('wave', 14 * 1024 + 24, 16384),
                              ('grid', (4 << 20) + 20, 64)):
        # replies of three classes in rotation, sources 3 / 9 / 14 bytes off
        # the 16-byte grid
        n = count
        cls = torch.arange(n, dtype=I32, device=dev) % 3
        sub = (torch.arange(n, dtype=I32, device=dev) // 3).to(I32)
        per = [(n + 2 - c) // 3 for c in range(3)]
        streams, rec_offs, totals, errs = [], [], [], []
        for c, skew in enumerate((3, 9, 14)):
            buf = torch.randint(0, 256, (skew + per[c] * size + 64,),
                                dtype=U8, device=dev)
            streams.append(buf[skew:])
            rec_offs.append(torch.arange(n, dtype=I64, device=dev) * size)
            totals.append(torch.tensor([per[c] * size], dtype=I64,
                                       device=dev))
            errs.append(torch.zeros(1, dtype=I32, device=dev))
        T = n * size
        out = torch.empty(T + 64, dtype=U8, device=dev)
        rec_off = torch.empty(n, dtype=I64, device=dev)
        total = torch.zeros(1, dtype=I64, device=dev)
        err = torch.zeros(1, dtype=I32, device=dev)
        ws = torch.empty(_lib.tree_mix_merge_workspace(n), dtype=U8,
                         device=dev)
        count_t = torch.tensor([n], dtype=I64, device=dev)
        counts = torch.tensor(per, dtype=I64, device=dev)

        def merge():
            _lib.tree_mix_merge(cls, sub, count_t, counts, n, streams,
                                rec_offs, totals, errs, out, out.numel(),
                                rec_off, total, err, ws)
        src = torch.randint(0, 256, (T,), dtype=U8, device=dev)
        dst = torch.empty(T, dtype=U8, device=dev)
        g_merge = graph_of(merge)
        g_copy = graph_of(lambda: dst.copy_(src))
        torch.cuda.synchronize()
        assert int(total.item()) == T and int(err.item()) == 0
        # the first and the last reply, against their sources
        assert torch.equal(out[:size], streams[0][:size])
        c, j = (n - 1) % 3, (n - 1) // 3
        assert torch.equal(out[T - size:T],
                           streams[c][j * size:(j + 1) * size])
        t_merge = timed(g_merge.replay, a.reps)
        t_copy = timed(g_copy.replay, a.reps)
        print('copy %-5s %8d replies of %8d B = %7.1f MB  merge %8.1f us '
              '%6.3f TB/s  torch copy %8.1f us %6.3f TB/s  ratio %.2f'
              % (name, n, size, T / 1e6, t_merge, T / t_merge / 1e6, t_copy,
                 T / t_copy / 1e6, t_merge / t_copy), flush=True)
        del streams, out, src, dst
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--fanout', type=int, default=1000)
    ap.add_argument('--batch', type=int, default=16384)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--no-copy', action='store_true')
    ap.add_argument('--no-server', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    tree = GpuTree(a.nodes, 100, fanout=a.fanout, device=dev, acl_cap=64)
    print('tree: %d znodes, %d directories of %d, an ACL table; captured '
          'graphs, median of %d' % (a.nodes, a.nodes // a.fanout, a.fanout,
                                    a.reps), flush=True)
    if not a.no_server:
        server_half(tree, a.batch, a, dev)
    if not a.no_copy:
        copy_tiers(a, dev)
    return 0


if __name__ == '__main__':
    sys.exit(main())
