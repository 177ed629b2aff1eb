"""The GPU server's session table (:class:`GpuSessionTable`)."""

import torch

from ..ops import _lib, batch as B
from .tree import _i64

I64, I32, U8 = torch.int64, torch.int32, torch.uint8


class GpuSessionTable(object):
    """The GPU server's session table in HBM and its handshake (K9 server
    side, csrc/kernels/session.hip): ConnectRequest frames in,
    ConnectResponse frames out, new / resumed / expired decided on the
    device.  Session ids are ``server_id << 56 | (index + 1)`` in allocation
    order, so the server's host side knows the id it handed out without a
    read-back."""

    MIN_TO, MAX_TO = 4000, 40000        # 2 and 20 ticks of 2 s

    def __init__(self, tree, cap=1 << 16, server_id=1, secret=0x5A4B1D,
                 members=1):
        dev = tree.device
        self.tree = tree
        self.dev = dev
        self.cap = cap
        self.server_id = server_id
        self.secret = secret
        # an ensemble of `members` servers replicates its session table:
        # member m's sessions live in slots (m - 1) * span ... (see
        # session.hip); one server's table has no partition
        self.span = cap // members if members > 1 else 0
        self.sid = torch.zeros(cap, dtype=I64, device=dev)
        self.passwd = torch.zeros(cap * 16, dtype=U8, device=dev)
        self.timeout = torch.zeros(cap, dtype=I32, device=dev)
        self.state = torch.zeros(cap, dtype=I32, device=dev)
        self.next = torch.zeros(1, dtype=I64, device=dev)
        self.allocated = 0              # host mirror of `next`
        self._tensors = [self.sid, self.passwd, self.timeout, self.state,
                         self.next]
        self.scanner = B.FrameScanner(64, dev, window=256)
        self.resp = torch.empty(64 * _lib.CR_RESP_BYTES, dtype=U8, device=dev)
        self.resp_sid = torch.empty(64, dtype=I64, device=dev)
        self.outcome = torch.empty(64, dtype=I32, device=dev)

    def sid_of(self, index):
        return (self.server_id << 56) | (index + 1)

    def connect(self, rx, nbytes, n_new):
        """Serve the ConnectRequest stream ``rx[:nbytes]`` (at most 64
        frames); ``n_new`` = how many of them ask for a new session (host
        bookkeeping of the allocation counter).  Returns (response stream
        [41 * frames], bound session ids, outcome codes)."""
        ft = self.scanner.scan(rx, nbytes)
        _lib.lib().session_connect(
            rx, ft.off, ft.length, ft.count, 64, self._tensors,
            self.server_id, _i64(self.secret), self.MIN_TO, self.MAX_TO,
            self.tree.counters[_lib.TC_ZXID:], self.resp, self.resp_sid,
            self.outcome, self.span)
        self.allocated += n_new
        return self.resp, self.resp_sid, self.outcome

    def close(self, sids):
        """Expire / close sessions (device int64 tensor of ids)."""
        _lib.lib().session_close(self._tensors, sids, self.server_id,
                                 self.span)

    def install(self, records):
        """Replicate other members' sessions into this table (device int64
        [k, 4]: sid, timeout, password bytes 0-7 and 8-15; this member's own
        records are skipped) — the receiving end of R3."""
        _lib.lib().session_install(self._tensors, records, self.server_id,
                                   self.span)
