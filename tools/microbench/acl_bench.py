"""ACL-path microbenchmark (csrc/kernels/tree_acl.hip) on a 1M-znode tree,
captured graphs, CUDA events, median of ``--reps``:

  get_acl   a 512K-request GET_ACL batch on random leaves: the server half
            (K1 on the requests + the ACL kernels, GpuServer.serve_acl) and
            the whole AclPipeline step (K10 encode, server, K1 + reply
            decode + ACL expansion + device check)
  exists    the SAME paths as an EXISTS batch through the existing serve()
            (its read-only instance, the GET pipeline's) in the same run:
            the server half (K1 + tree_serve_k + K13) and the step (K10,
            server, K1 + reply decode) — the yardstick, existing code.  An
            EXISTS reply is 88 bytes, a GET_ACL reply of the open ACL 115
            and one dependent read (node -> ACL word -> arena) more
  create    a 512K-CREATE batch (EPHEMERAL, expired untimed after every
            run, so each run creates the same nodes) served by a tree with
            and one without the ACL table, for 1, 2 and 1024 distinct ACLs
            in the batch: the cost of the record pass, and the pass alone
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
from zkmi import consts  # noqa: E402
from zkmi.ops import _lib  # noqa: E402
from zkmi.ops import batch as B  # noqa: E402
from zkmi.bench.synthetic import (AclPipeline, MIX_ACLS,  # noqa: E402
                                  _acl_table, _arena)
from zkmi.server.engine import GpuServer  # noqa: E402
from zkmi.server.tree import GpuTree  # noqa: E402

I64, I32, U8 = torch.int64, torch.int32, torch.uint8
SESSION = 0x5EED


def timed(fn, reps, warm=3, after=None):
    ts = []
    for k in range(warm + reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= warm:
            ts.append(a.elapsed_time(b) * 1e3)
        if after is not None:
            after()
            torch.cuda.synchronize()
    return statistics.median(ts)


def graph_of(fn, after=None):
    fn()
    if after is not None:
        after()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        fn()
    if after is not None:
        after()
    torch.cuda.synchronize()
    return g


class ExistsYardstick(object):
    """EXISTS on the paths of an AclPipeline through serve()."""

    def __init__(self, pipe):
        tree, n, dev = pipe.tree, pipe.batch, pipe.dev
        self.pipe = pipe
        r = pipe.rb
        self.rb = B.RequestBatch(
            n, torch.full((n,), consts.OP_CODES['EXISTS'], dtype=I32,
                          device=dev),
            r.xid, r.arg, r.path_off, r.path_len, r.data_off, r.data_len,
            r.acl_id, r.path_arena, r.data_arena, r.acl_off, r.acl_len,
            r.acl_arena)
        self.xt = B.XidTable(bits=max(20, (n - 1).bit_length() + 1),
                             device=dev)
        self.tx = torch.empty(pipe.tx.numel() + n, dtype=U8, device=dev)
        self.server = GpuServer(tree, n, n * (4 + 16 + 68) + 64,
                                window=pipe.server.window, seq_order=False)
        self.server.read_only = True
        self.rscanner = B.FrameScanner(n, dev,
                                       window=B.frame_window(4 + 16 + 68))
        self.reply = B.alloc_replies(n, dev)
        self.last = None

    def encode(self):
        tx, _, total, _ = B.encode_requests(self.rb, self.xt, out=self.tx)
        return tx, total

    def server_step(self, tx, total):
        return self.server.serve(tx, total)

    def step(self):
        tx, total = self.encode()
        rx, rtotal, rerr, _ = self.server_step(tx, total)
        ft = self.rscanner.scan(rx, rtotal)
        rep = B.decode_replies(rx, ft, self.xt, out=self.reply)
        self.last = (rep, rtotal, ft)

    def ok(self):
        rep, rtotal, ft = self.last
        n = self.pipe.batch
        return (int(ft.count[0].item()) == n and
                bool((rep.err[:n] == 0).all().item()) and
                int(rtotal.item()) == n * 88)


def bench_reads(a, dev):
    tree = GpuTree(a.nodes, 100, fanout=a.fanout, device=dev, acl_cap=2048)
    n = a.batch
    pipe = AclPipeline(tree, n)
    acc = pipe.step()
    torch.cuda.synchronize()
    if int(acc.item()) != n or int(pipe.bad.item()) != 0:
        print('get_acl CHECK FAILED %r' % (pipe.diagnose(),))
        return 1
    out_bytes = int(pipe.last[3].item())
    acc = torch.zeros(1, dtype=I64, device=dev)
    g_step = pipe.capture(acc)
    tx, total = pipe.encode()
    g_srv = graph_of(lambda: pipe.server_step(tx, total))
    ex = ExistsYardstick(pipe)
    ex.step()
    torch.cuda.synchronize()
    if not ex.ok():
        print('exists CHECK FAILED')
        return 1
    ex_bytes = int(ex.last[1].item())
    gx_step = graph_of(ex.step)
    etx, etotal = ex.encode()
    gx_srv = graph_of(lambda: ex.server_step(etx, etotal))
    # alternate the two paths so drift hits both alike
    t = {k: [] for k in ('srv', 'step', 'xsrv', 'xstep')}
    for _ in range(3):
        t['srv'].append(timed(g_srv.replay, a.reps))
        t['xsrv'].append(timed(gx_srv.replay, a.reps))
        t['step'].append(timed(g_step.replay, a.reps))
        t['xstep'].append(timed(gx_step.replay, a.reps))
    torch.cuda.synchronize()
    ok = int(pipe.bad.item()) == 0 and ex.ok()
    m = {k: statistics.median(v) for k, v in t.items()}
    print('get_acl requests=%d reply=%7.2f MB  server %8.1f us  step %8.1f us'
          '  (rounds: server %s step %s)'
          % (n, out_bytes / 1e6, m['srv'], m['step'],
             ' '.join('%.1f' % x for x in t['srv']),
             ' '.join('%.1f' % x for x in t['step'])), flush=True)
    print('exists  requests=%d reply=%7.2f MB  server %8.1f us  step %8.1f us'
          '  (rounds: server %s step %s)'
          % (n, ex_bytes / 1e6, m['xsrv'], m['xstep'],
             ' '.join('%.1f' % x for x in t['xsrv']),
             ' '.join('%.1f' % x for x in t['xstep'])), flush=True)
    print('get_acl / exists: server %.2f  step %.2f  reply bytes %.2f  %s'
          % (m['srv'] / m['xsrv'], m['step'] / m['xstep'],
             out_bytes / ex_bytes, 'ok' if ok else 'CHECK FAILED'),
          flush=True)
    return 0 if ok else 1


def many_acls(k):
    return [[{'perms': 1 + i % 31,
              'id': {'scheme': 'ip', 'id': '10.%d.%d.1' % (i >> 8, i & 255)}}]
            for i in range(k)]


def bench_creates(a, dev):
    n = a.batch
    ndirs = (a.nodes + a.fanout - 1) // a.fanout
    paths = ['/bench/d%06d/c%07d' % (i % ndirs, i) for i in range(n)]
    parena, poff, plen = _arena(paths, dev)
    maxpath = max(len(p) for p in paths)
    data = torch.full((16,), 0x61, dtype=U8, device=dev)
    rc = 0
    trees = {}
    for with_acl in (False, True):
        # room for the batch's nodes beside the static ones
        trees[with_acl] = GpuTree(a.nodes, 100, fanout=a.fanout, device=dev,
                                  spare=0.25 + n / a.nodes,
                                  acl_cap=2048 if with_acl else 0)
    for name, acls in (('1', [MIX_ACLS[1]]), ('2', list(MIX_ACLS)),
                       ('1024', many_acls(1024))):
        aarena, aoff, alen = _acl_table(acls, dev)
        amax = int(alen.max().item())
        frame = 4 + 8 + 4 + maxpath + 4 + 16 + amax + 4
        res = {}
        for with_acl in (False, True):
            tree = trees[with_acl]
            srv = GpuServer(tree, n, n * (4 + 16 + 4 + maxpath) + 64,
                            window=B.frame_window(frame), seq_order=False)
            xt = B.XidTable(bits=max(20, (n - 1).bit_length() + 1),
                            device=dev)
            rb = B.RequestBatch(
                n, torch.full((n,), consts.OP_CODES['CREATE'], dtype=I32,
                              device=dev),
                torch.arange(n, dtype=I32, device=dev),
                torch.full((n,), consts.CREATE_FLAGS['EPHEMERAL'], dtype=I32,
                           device=dev),
                poff, plen, torch.zeros(n, dtype=I64, device=dev),
                torch.full((n,), 16, dtype=I32, device=dev),
                (torch.arange(n, device=dev) % len(acls)).to(I32),
                parena, data, aoff, alen, aarena)
            tx = torch.empty(n * frame + 64, dtype=U8, device=dev)
            tx, _, total, _ = B.encode_requests(rb, xt, out=tx)

            def expire():
                tree.expire(SESSION)

            def serve():
                return srv.serve(tx, total, session=SESSION)

            serve()
            torch.cuda.synchronize()
            good = bool((srv.resp.err[:n] == 0).all().item())
            expire()
            g = graph_of(serve, after=expire)
            res[with_acl] = timed(g.replay, a.reps, after=expire)
            if with_acl:
                ft = srv.result[3]
                r = srv.resp
                serve()

                def record():
                    _lib.tree_acl_record(tree.acl, tx, ft.off, ft.length,
                                         ft.count, n, r.opcode, r.err, r.node,
                                         srv._acl_workspace())

                g_rec = graph_of(record)
                t_rec = timed(g_rec.replay, a.reps)
                expire()
                torch.cuda.synchronize()
                stats = srv.acl_stats()
            if not good:
                rc = 1
            del srv, g
        print('create  requests=%d acls=%-4s  serve %8.1f us  with table '
              '%8.1f us  (+%.1f us, x%.3f)  record pass alone %7.1f us  '
              'table: entries %d bytes %d lost %d  %s'
              % (n, name, res[False], res[True], res[True] - res[False],
                 res[True] / res[False], t_rec, stats[0], stats[1], stats[2],
                 'ok' if rc == 0 and stats[2] == 0 else 'CHECK FAILED'),
              flush=True)
        if stats[2] != 0:
            rc = 1
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--fanout', type=int, default=1000)
    ap.add_argument('--batch', type=int, default=512 * 1024)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--only', choices=('reads', 'creates'), default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    print('tree: %d znodes, batch %d, median of %d' % (a.nodes, a.batch,
                                                      a.reps), flush=True)
    rc = 0
    if a.only in (None, 'reads'):
        rc |= bench_reads(a, dev)
        torch.cuda.empty_cache()
    if a.only in (None, 'creates'):
        rc |= bench_creates(a, dev)
    return rc


if __name__ == '__main__':
    sys.exit(main())
