"""AUTH with digest identities in a session batch: what
GpuServer.serve_sessions_mixed(perms=AclIdentity(addrs, auth=AuthTable))
costs (csrc/kernels/tree_auth.hip), on sessions_mixed_bench's tree and
request mix.  Captured graphs in the same run (CUDA events, median after
warm-up replays).  Two figures a shape:

  no AUTH frame   the batch of S connections x r requests served with
                  ``perms`` alone (the launches of a tree without this file:
                  aclperm_check_k and aclperm_fix_k are untouched) and with
                  an AuthTable: three launches instead of one around the
                  check, each lane of the AUTH pass leaving at the opcode
                  word.  ``--acl-vector`` binds every node to a three-entry
                  vector whose first entry is a digest entry, so the check
                  walks the arena's bytes and, with the table, compares the
                  entry with the row's identities (each connection holds
                  one after the AUTH batch below);
  S AUTH frames   one batch of one AUTH frame a connection (``digest``,
                  ``user<s>:password<s>``): the parse, two SHA-1 blocks'
                  worth of rounds at most, base64, the claim and the record,
                  and the three passes' replies.  The graph replays on a
                  table that holds the identities (every frame is `known`);
                  the first, uncaptured serve of the batch — every frame
                  stores — is timed once by the wall clock around a
                  synchronize, launch latency included."""

import argparse
import os
import struct
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
import sessions_mixed_bench as B  # noqa: E402
from zkmi.server.engine import (AclIdentity, AuthTable,  # noqa: E402
                                GpuServer, SessionSegments)
from zkmi.server.tree import GpuTree  # noqa: E402

I64, I32 = torch.int64, torch.int32


def auth_frame(xid, cred):
    body = struct.pack('>iii', xid, 100, 0) + struct.pack('>i', 6) + \
        b'digest' + struct.pack('>i', len(cred)) + cred
    return struct.pack('>i', len(body)) + body


def segments(parts, S, dev):
    cuts = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    sids = [(1 << 56) | (s + 1) for s in range(S)]
    return SessionSegments(torch.tensor(cuts, dtype=I64, device=dev),
                           torch.tensor(sids, dtype=I64, device=dev),
                           torch.tensor([s % 64 for s in range(S)],
                                        dtype=I32, device=dev)), int(cuts[-1])


def shape(tree, S, r, a, dev):
    rng = np.random.default_rng(1000 * S + r)
    conns = [B.connection(rng, r, a.nodes, a.fanout, b'x' * 100)
             for _ in range(S)]
    parts = [c[0] for c in conns]
    segs, n = segments(parts, S, dev)
    rx = B.dev_bytes(b''.join(parts), dev)
    out_cap = S * r * 256 + sum(c[1] for c in conns) * (a.fanout * 20 + 256) \
        + (1 << 16)
    srv = GpuServer(tree, S * r, out_cap, seq_order=False)
    addrs = torch.tensor([0x0A010000 + (s & 0xFFFF) for s in range(S)],
                         dtype=I32, device=dev)
    tbl = AuthTable(S, dev)
    plain, withtbl = AclIdentity(addrs), AclIdentity(addrs, auth=tbl)
    # the AUTH batch first: each connection holds one identity afterwards
    aparts = [auth_frame(s + 1, b'user%d:password%d' % (s, s))
              for s in range(S)]
    asegs, an = segments(aparts, S, dev)
    arx = B.dev_bytes(b''.join(aparts), dev)
    asrv = GpuServer(tree, S * r, S * 64 + (1 << 16), seq_order=False)
    asrv.serve_sessions_mixed(arx, an, asegs, perms=plain)     # (buffers)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, total, err, _ = asrv.serve_sessions_mixed(arx, an, asegs,
                                                 perms=withtbl)
    torch.cuda.synchronize()
    first = (time.perf_counter() - t0) * 1e6
    assert int(err.item()) == 0 and int(total.item()) == 20 * S
    st = asrv.auth_stats()
    assert st['ok'] == S and st['answered_ok'] == S and st['failed'] == 0, st
    g = B.graph_of(lambda: asrv.serve_sessions_mixed(arx, an, asegs,
                                                     perms=withtbl))
    t_auth = B.timed(g.replay, a.reps)
    del g
    assert asrv.auth_stats()['full'] == 0
    res = {}
    for name, perms in (('perms', plain), ('perms+table', withtbl)):
        _, total, err, ft = srv.serve_sessions_mixed(rx, n, segs, perms=perms)
        torch.cuda.synchronize()
        assert int(err.item()) == 0 and int(ft.count.item()) == S * r
        res[name] = int(total.item())
        g = B.graph_of(lambda: srv.serve_sessions_mixed(rx, n, segs,
                                                        perms=perms))
        res[name] = (res[name],) + B.timed(g.replay, a.reps)
        del g
    assert res['perms'][0] == res['perms+table'][0]
    assert srv.acl_enforce_stats()['denied'] == 0
    print('S %5d x r %6d = %7d requests  ' % (S, r, S * r) + '  '.join(
        '%s %.1f us (min %.1f, max %.1f)' % ((k,) + v[1:])
        for k, v in res.items()) + '  the table costs %+.1f us' % (
            res['perms+table'][1] - res['perms'][1]))
    print('S %5d AUTH frames            known %.1f us (min %.1f, max %.1f)  '
          'the storing serve, uncaptured, once: %.0f us' % (
              (S,) + t_auth + (first,)), flush=True)
    del srv, asrv
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--fanout', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--shape', action='append',
                    help='SxR (default: %s)' % ', '.join(
                        '%dx%d' % s for s in B.SHAPES))
    ap.add_argument('--acl-vector', action='store_true',
                    help='every node carries a three-entry ACL vector')
    a = ap.parse_args()
    shapes = B.SHAPES if not a.shape else \
        [tuple(int(x) for x in s.split('x')) for s in a.shape]
    dev = torch.device('cuda', 0)
    tree = GpuTree(a.nodes, 100, fanout=a.fanout, device=dev,
                   acl_cap=1 << 12, watch_cap=1 << 16)
    print('tree: %d znodes, fanout %d; sessions_mixed_bench\'s mix; %s; '
          'captured graphs, median of %d' % (
              a.nodes, a.fanout, 'a three-entry vector a node'
              if a.acl_vector else 'the open ACL everywhere', a.reps),
          flush=True)
    if a.acl_vector:
        B.bind_vector(tree)
    for S, r in shapes:
        shape(tree, S, r, a, dev)
    return 0


if __name__ == '__main__':
    sys.exit(main())
