"""A tick of the GPU server's front end (zkmi/server/gpu.py) without its
sockets: S connections with f GET_DATA frames each pending, on a small tree,
through the very launches a tick makes — the upload, the cut
(csrc/kernels/front.hip front_cut + the scan of take[]), the pack
(front_gather), the serve (serve_sessions_mixed(resume=True, close=True)), the
TX assembly (front_tx_pieces + scan + front_gather) and the two copies back
(the report, tx[:total]).

Each phase is timed with device events recorded around it on the one stream;
the line gives the median of ``--reps`` ticks per phase in microseconds, and
the tick's wall time (the host's launch work included).  Every tick checks
that all S * f frames were taken and that the TX total is the replies'."""

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
from zkmi import consts, jute  # noqa: E402
from zkmi.server.engine import GpuServer, SessionSegments  # noqa: E402
from zkmi.server.tree import GpuTree  # noqa: E402
from zkmi.ops import _lib  # noqa: E402

I64, I32, U8 = torch.int64, torch.int32, torch.uint8
PHASES = ('upload', 'cut', 'pack', 'serve', 'assembly', 'copies')


def pending(S, f, nodes, fanout):
    """Connection s's f GET_DATA frames -> (bytes, raw_starts)."""
    parts = []
    for s in range(S):
        b = b''
        for j in range(f):
            i = (s * f + j) % nodes
            b += jute.frame(jute.encode_request({
                'opcode': 'GET_DATA', 'xid': 1 + j, 'watch': False,
                'path': '/bench/d%06d/n%09d' % (i // fanout, i)}))
        parts.append(b)
    cuts = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    return b''.join(parts), cuts.astype(np.int64)


def one(tree, S, f, a, dev):
    L = _lib.lib()
    raw, cuts = pending(S, f, a.nodes, a.fanout)
    n = len(raw)
    frames = S * f
    srv = GpuServer(tree, max(frames, 64), frames * 256 + (1 << 16))
    h_raw = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).pin_memory()
    h_starts = torch.from_numpy(cuts).pin_memory()
    d_raw = torch.zeros(n, dtype=U8, device=dev)
    d_rstarts = torch.zeros(S + 1, dtype=I64, device=dev)
    d_starts = torch.zeros(S + 1, dtype=I64, device=dev)
    rx = torch.zeros(n, dtype=U8, device=dev)
    take = torch.zeros(S, dtype=I64, device=dev)
    nfr = torch.zeros(S, dtype=I32, device=dev)
    flag = torch.zeros(S, dtype=I32, device=dev)
    fault = torch.zeros(1, dtype=I64, device=dev)
    over = torch.zeros(2, dtype=I64, device=dev)
    segs = SessionSegments(
        d_starts,
        torch.tensor([(1 << 56) | (s + 1) for s in range(S)], dtype=I64,
                     device=dev),
        torch.tensor([s if s < 64 else -1 for s in range(S)], dtype=I32,
                     device=dev))
    scan_ws = torch.empty(L.scan_workspace(4 * S), dtype=I64, device=dev)
    owner = torch.zeros(64, dtype=I64, device=dev)
    p_stream = torch.zeros(4 * S, dtype=I32, device=dev)
    p_src = torch.zeros(4 * S, dtype=I64, device=dev)
    p_len = torch.zeros(4 * S, dtype=I64, device=dev)
    p_off = torch.zeros(4 * S + 1, dtype=I64, device=dev)
    fstats = torch.zeros(8, dtype=I64, device=dev)
    tx_cap = frames * 256 + (1 << 20)
    d_tx = torch.zeros(tx_cap, dtype=U8, device=dev)
    h_tx = torch.zeros(tx_cap, dtype=U8).pin_memory()
    d_report = torch.zeros(3 * S + 2, dtype=I64, device=dev)
    h_report = torch.zeros(3 * S + 2, dtype=I64).pin_memory()
    quota = max(1, srv.cap_frames // S)

    def tick():
        ev = [torch.cuda.Event(enable_timing=True)
              for _ in range(len(PHASES) + 1)]
        t0 = time.perf_counter()
        ev[0].record()
        d_raw.copy_(h_raw, non_blocking=True)
        d_rstarts.copy_(h_starts, non_blocking=True)
        ev[1].record()
        _lib.front_cut(d_raw, n, d_rstarts, quota, consts.MAX_PACKET, take,
                       nfr, flag, fault)
        L.scan_excl(take, d_starts, d_starts[S:], scan_ws)
        ev[2].record()
        _lib.front_gather([d_raw], None, d_rstarts, d_starts, S, rx,
                          over[0:1])
        ev[3].record()
        out, _, err, _ = srv.serve_sessions_mixed(
            rx, d_starts[S:], segs, resume=True, close=True)
        ev[4].record()
        streams = [out, srv.resume_notif[0], srv.notif[0],
                   srv.close_notif[0]]
        _lib.front_tx_pieces(srv.seg.rep_off, segs.wslots,
                             srv.resume_slots[1], srv.notif_slots[1],
                             srv.close_slots[1], err,
                             [int(s.numel()) for s in streams], owner,
                             p_stream, p_src, p_len, fstats)
        L.scan_excl(p_len, p_off, p_off[4 * S:], scan_ws)
        _lib.front_gather(streams, p_stream, p_src, p_off, 4 * S, d_tx,
                          over[1:2])
        ev[5].record()
        torch.cat([take, flag.to(I64), p_off[0::4], fault], out=d_report)
        h_report.copy_(d_report, non_blocking=True)
        torch.cuda.synchronize()
        total = int(h_report[3 * S])
        h_tx[:total].copy_(d_tx[:total], non_blocking=True)
        ev[6].record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e6
        assert int(h_report[:S].sum()) == n and int(h_report[-1]) == 0
        assert total == int(srv.seg.rep_off[S].item()) and total > 0
        return [ev[k].elapsed_time(ev[k + 1]) * 1e3
                for k in range(len(PHASES))] + [wall]

    for _ in range(a.warmup):
        tick()
    ts = [tick() for _ in range(a.reps)]
    med = [statistics.median(t[k] for t in ts) for k in range(len(PHASES) + 1)]
    print('S %5d x f %4d = %7d frames, %8d bytes in: ' % (S, f, frames, n) +
          '  '.join('%s %.1f' % (p, med[k]) for k, p in enumerate(PHASES)) +
          '  | tick wall %.1f us' % med[-1], flush=True)
    del srv
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=2000)
    ap.add_argument('--fanout', type=int, default=100)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--shape', action='append',
                    help='S,f (default: 64,1 64,16 1024,1 1024,16 1024,64)')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    tree = GpuTree(a.nodes, 100, fanout=a.fanout, device=dev, watch_cap=4096,
                   acl_cap=64)
    print('tree: %d znodes, fanout %d, a watch table; S connections x f '
          'GET_DATA frames a tick; device events around each phase, the '
          'median of %d ticks (us)' % (a.nodes, a.fanout, a.reps), flush=True)
    shapes = a.shape or ['64,1', '64,16', '1024,1', '1024,16', '1024,64']
    for sh in shapes:
        S, f = (int(x) for x in sh.split(','))
        one(tree, S, f, a, dev)
    return 0


if __name__ == '__main__':
    sys.exit(main())
