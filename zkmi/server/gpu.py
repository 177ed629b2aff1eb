"""A TCP front end for the GPU server: :class:`GpuZKServer` gives
:class:`zkmi.Client` a ZooKeeper endpoint backed by the HBM tree
(:class:`zkmi.server.tree.GpuTree`).

It is an in-process server, as :class:`FakeZKServer` is, on a thread of its
own with a HIP stream of its own and non-blocking sockets on ``selectors``.
It owns one :class:`GpuServer` and one :class:`GpuSessionTable` and drives
them through their public entry points only: ``GpuSessionTable.connect`` for
the handshakes, ``serve_sessions_mixed(resume=True, close=True)`` for a tick's
requests, ``close_sessions`` for the sessions its timers expire.

A tick.  What every connection has received — byte for byte, partial trailing
frames included — is concatenated into a pinned buffer and uploaded as one raw
stream with a segment per connection.  On the device (csrc/kernels/front.hip;
the rules: zk_front.h) every segment is cut at a frame boundary, the cut
prefixes are packed into the dense batch the serve takes, and after the serve
every connection's bytes for its socket — its replies, then its watcher
slot's catch-up, write-fired and close-fired notifications — are assembled
into one TX buffer.  The host reads one small report and ``tx[:total]``: two
device-to-host synchronisations a tick, whatever the number of connections
and frames, and no per-connection or per-frame device read.

Known divergences from ZooKeeper:

* ``order_passes=0`` (the default): one write per connection per tick.  The
  unordered session batch has no in-batch ordering, so a connection's taken
  run is any number of reads or exactly one CREATE / DELETE / SET_DATA /
  CLOSE_SESSION; a pipelined connection's requests still take effect in
  order, a tick apart;
* ``order_passes=P``: a connection's pipelined writes are served in one tick,
  through the ordered session serve of ``P`` passes.  The taken run is cut
  where the engines' fixed sequence would differ from the connection's own
  order (no CREATE / DELETE / SET_DATA behind a list, GET_ACL or SET_WATCHES
  frame of the same run; a CLOSE_SESSION ends it).  A request that more than
  ``P - 1`` conflicting earlier requests of the tick precede is deferred with
  everything behind it on its connection and served in a later tick: a path
  contended by more than ``P`` requests drains ``P`` ranks a tick, in row
  order, so a low row can delay a high one (no fair rotation).  A deferred
  SEQUENTIAL create leaves a gap in its parent's cversion, as every refused
  numbered create does.  The zxids of a tick follow batch order, which is
  row order, not arrival order.  A read that a later write of the tick
  overtakes is answered from a snapshot in the tree's scratch tail, and so is
  a SET_DATA that a later write of the tick overtakes (its reply's Stat).
  When the tail is full such a request is answered SYSTEMERROR — a read
  without harm, but such a SET_DATA has been applied: a write that took
  effect is reported as failed.  ``stats()['order_scratch_full']`` counts the
  ticks in which that happened; size ``GpuTree(scratch=...)`` for
  ``cap_frames`` snapshots (a slot is 76 bytes and the node's data, rounded
  up to 16) and it cannot;
* inside a tick a connection's replies are sent before its notifications;
* 64 watcher slots: the 65th live session gets none, its watches arm nothing
  (``stats()['no_watcher_slot']``);
* a batch whose reply encode overflowed has applied its writes and lost its
  replies: its connections are dropped (``stats()['batches_lost']``);
* ``enforce_acl=True``: permission and existence are those of the tree as the
  tick finds it (a node created in a tick is protected from the next one on);
  ``world`` and ``ip`` entries match as in ZooKeeper, and a ``digest`` entry
  matches a connection after its AUTH (``Client.add_auth('digest',
  b'user:password')``; csrc/kernels/zk_auth.h).  The ``auth`` and ``sasl``
  schemes still match nobody: ZooKeeper rewrites an ``auth`` entry at CREATE
  into the creator's identities, which is not done here.  GET_ACL needs no
  permission (ZooKeeper 3.4 / 3.5); a node whose ACL found no room in the
  store denies every op that needs a permission;
* SET_ACL (``Client.set_acl``; served whenever the tree has an ACL table,
  ADMIN checked with ``enforce_acl``; csrc/kernels/zk_setacl.h): a SET_ACL
  frame is taken only as the first frame of its connection's run and ends
  the run behind itself, so a connection's GET_ACL sent before its SET_ACL is
  answered from the old ACL and one sent after from the new, a tick apart.
  ADMIN is judged on the ACL as the tick's pass finds it, before any SET_ACL
  of the tick took effect.  SET_ACLs of several connections on one node run
  in row order, one a round, 4 rounds a tick: a fifth one of a tick is
  answered SYSTEMERROR without effect (``stats()['setacl_unreached']``), not
  deferred.  Equal entries are not removed and an ``auth`` entry is not
  rewritten; the vector of a SET_ACL that fails BAD_VERSION stays in the
  store (nothing in it is reclaimed);
* AUTH (with ``enforce_acl``; without it an AUTH frame is answered
  BAD_ARGUMENTS): an identity holds for every frame of its connection in the
  tick that carries its AUTH frame, the frames ahead of the AUTH frame in the
  stream included.  A failed AUTH (any scheme but ``digest``, a malformed
  frame) is answered AUTH_FAILED and the connection stays open; ZooKeeper
  closes it.  At most 4 identities a connection and credentials of at most
  119 bytes: beyond either the answer is AUTH_FAILED.
"""

import heapq
import selectors
import socket
import struct
import threading
import time

import numpy as np
import torch

from .. import consts
from ..ops import _lib
from .engine import (AclIdentity, AuthTable, GpuServer, OrderDefer,
                     SessionSegments)
from .sessions import GpuSessionTable

I64, I32, U8 = torch.int64, torch.int32, torch.uint8
SLOTS = 64
_SS_ALIVE = 1                     # csrc/kernels/zk_session.h
_HS_MAX = 4096                    # a ConnectRequest frame's largest length
# the report's words behind the per-segment tables
(_R_FAULT, _R_OVER_RX, _R_OVER_TX, _R_ERR, _R_BAD, _R_DUP, _R_FRAMES,
 _R_CATCHUP, _R_N) = range(9)
# behind them with order_passes: frames deferred, write frames taken, the
# largest rank, the snapshot scratch's top
_R_DEFER, _R_NWR, _R_RANK, _R_SCRATCH, _R_NORD = range(_R_N, _R_N + 5)
# the flag column with order_passes: bit 0 the cut's flag, bit 1 something of
# what the cut took was deferred
_F_BAD, _F_DEFER = 1, 2


class _Sess(object):
    __slots__ = ('sid', 'idx', 'wslot', 'timeout', 'last', 'conn')

    def __init__(self, sid, idx, wslot, timeout, now):
        self.sid, self.idx, self.wslot = sid, idx, wslot
        self.timeout, self.last, self.conn = timeout, now, None


class _Conn(object):
    __slots__ = ('sock', 'row', 'inbuf', 'out', 'sess', 'live', 'closing',
                 'stalled', 'writing', 'dead')

    def __init__(self, sock, row):
        self.sock, self.row = sock, row
        self.inbuf = bytearray()      # received, not yet served
        self.out = bytearray()        # the unsent tail
        self.sess = None
        self.live = False             # the handshake is done
        self.closing = False          # close once `out` is flushed
        self.stalled = -1             # len(inbuf) a tick took nothing of
        self.writing = False
        self.dead = False


def peer_ipv4(addr):
    """The IPv4 address of a socket's peer (``accept()``'s or
    ``getpeername()``'s address tuple) as a host-order 32-bit word in int32
    range, the form :class:`AclIdentity` takes; for an IPv4-mapped IPv6 peer
    the mapped address; 0 for anything else (which no ``ip`` ACL entry
    matches)."""
    try:
        host = addr[0]
        if ':' in host:
            host = host.split('%', 1)[0]
            raw = socket.inet_pton(socket.AF_INET6, host)
            if raw[:12] != b'\0' * 10 + b'\xff\xff':
                return 0
            raw = raw[12:]
        else:
            raw = socket.inet_pton(socket.AF_INET, host)
    except (OSError, TypeError, IndexError, ValueError, AttributeError):
        return 0
    return struct.unpack('>i', raw)[0]


def _pinned(n, dtype, dev):
    t = torch.zeros(n, dtype=dtype)
    return t.pin_memory() if dev.type == 'cuda' else t


class GpuZKServer(object):
    """``GpuZKServer(tree, cap_frames=..., out_cap=...)`` listens on
    ``port`` (0: a free one) and serves ``tree``, a :class:`GpuTree` with a
    watch table (an ACL table is optional), to ZooKeeper clients.

    ``cap_frames``  frames a tick serves (the :class:`GpuServer`'s).  A tick's
                    quota a connection is ``cap_frames // active connections``;
                    with more active connections than that they take turns.
    ``out_cap``     bytes of the reply stream of one tick.  It must hold the
                    replies of ``cap_frames`` requests: a GET_DATA reply is 88
                    bytes and the node's data, a list reply 88 bytes and 4 +
                    the length of every child's name.  A tick whose replies do
                    not fit has applied its writes and lost its replies: the
                    batch's connections are dropped and it is counted in
                    ``stats()['batches_lost']``.
    ``max_conns``   connections, and rows of the segment table: it always has
                    this many, an idle connection is an empty segment.
    ``tick_ms``     how long an idle server sleeps in ``select`` before it
                    looks at its session timers (10 ms at least; a socket
                    wakes it at once, and a server with requests pending does
                    not sleep).
    ``table``       a :class:`GpuSessionTable` of one server (default: a new
                    one).
    ``raw_cap``     bytes a tick uploads; also the longest request frame.
    ``order_passes``  0: a connection's taken run holds one write at most.
                    ``P >= 1``: the ordered tick (the module's divergence
                    list) — the ordered cut, ``serve_sessions_mixed(ordered=
                    True, passes=P, defer=...)``, each connection advanced by
                    the bytes that were not deferred.  It needs a tree with a
                    scratch tail (``GpuTree(scratch=...)``; ``ValueError``
                    without one) and ``cap_frames <= 65536``, and costs
                    about 3 ``P`` + 8 launches a tick more.
    ``enforce_acl``  the ACLs the tree keeps are enforced (``GpuServer.
                    serve_sessions_mixed(perms=...)``; the rule:
                    csrc/kernels/zk_aclperm.h): a connection is its peer's
                    IPv4 address, taken at ``accept`` (none for a peer that
                    is not IPv4 or IPv4-mapped: no ``ip`` entry matches it),
                    and a request its node's or parent's ACL does not allow
                    is answered NO_AUTH.  The server keeps an
                    :class:`~zkmi.server.engine.AuthTable` of ``max_conns``
                    rows: an AUTH frame with the scheme ``digest`` adds an
                    identity to its connection, which ``digest`` entries
                    then match; a row is forgotten when its connection
                    closes and when a new one takes it.  It needs a tree
                    with an ACL table (``ValueError`` without one) and costs
                    four launches a tick.  Off, ACLs are stored and
                    returned, nothing more.

    ``.port``, ``.address``, ``.servers()`` and ``.shutdown()`` as
    :class:`FakeZKServer`'s; :meth:`call` runs a function on the server's
    thread between two ticks (the tree is the thread's while it runs),
    :meth:`stats` reports the counters."""

    def __init__(self, tree, cap_frames, out_cap, max_conns=1024, port=0,
                 tick_ms=1.0, table=None, host='127.0.0.1', raw_cap=1 << 20,
                 order_passes=0, enforce_acl=False):
        if tree.watch is None:
            raise ValueError('GpuZKServer: the tree needs a watch table')
        if table is not None and table.span != 0:
            raise ValueError('GpuZKServer: one server\'s session table')
        if max_conns < 1 or cap_frames < 1 or raw_cap < 4096:
            raise ValueError('GpuZKServer: max_conns, cap_frames >= 1, '
                             'raw_cap >= 4096')
        self.order_passes = P = int(order_passes)
        if P < 0 or P > 127:
            raise ValueError('GpuZKServer: order_passes in 0..127')
        if P >= 1 and cap_frames > 1 << 16:
            # (tree_order.hip ORD_MAX_GROUP: a larger group of conflicting
            # requests is refused wholesale, and deferring all of it every
            # tick would never drain it)
            raise ValueError('GpuZKServer: order_passes serves at most 65536 '
                             'frames a tick')
        if P >= 1 and tree.scratch is None:
            raise ValueError('GpuZKServer: order_passes needs a tree with a '
                             'scratch tail (GpuTree(scratch=...))')
        self.enforce_acl = bool(enforce_acl)
        if self.enforce_acl and tree.acl is None:
            raise ValueError('GpuZKServer: enforce_acl needs a tree with an '
                             'ACL table (GpuTree(acl_cap=...))')
        self.tree = tree
        self.dev = dev = tree.device
        self.cap_frames = int(cap_frames)
        self.max_conns = S = int(max_conns)
        self.raw_cap = int(raw_cap)
        # (an idle server wakes for its timers only: sockets wake select)
        self.tick_s = max(float(tick_ms), 10.0) / 1000.0
        self.gs = GpuServer(tree, self.cap_frames, int(out_cap))
        self.table = table if table is not None else GpuSessionTable(tree)
        self.stream = torch.cuda.Stream(dev)
        # -- the segment table: max_conns rows, allocated once ----------------
        self.h_rstarts = _pinned(S + 1, I64, dev)
        self.h_sessions = _pinned(S, I64, dev)
        self.h_wslots = _pinned(S, I32, dev)
        self.h_sidx = _pinned(S, I64, dev)
        self.h_wslots.fill_(-1)
        self.np_rstarts = self.h_rstarts.numpy()
        self.np_sessions = self.h_sessions.numpy()
        self.np_wslots = self.h_wslots.numpy()
        self.np_sidx = self.h_sidx.numpy()
        self.d_rstarts = torch.zeros(S + 1, dtype=I64, device=dev)
        self.d_starts = torch.zeros(S + 1, dtype=I64, device=dev)
        self.d_sessions = torch.zeros(S, dtype=I64, device=dev)
        self.d_wslots = torch.full((S,), -1, dtype=I32, device=dev)
        self.d_sidx = torch.zeros(S, dtype=I64, device=dev)
        self.segs = SessionSegments(self.d_starts, self.d_sessions,
                                    self.d_wslots)
        # each row's peer (peer_ipv4), for the ACL check
        self.h_addrs = _pinned(S, I32, dev)
        self.np_addrs = self.h_addrs.numpy()
        self.d_addrs = torch.zeros(S, dtype=I32, device=dev)
        # each row's digest identities (AUTH), and the rows to forget before
        # the next batch: a connection has closed or a new one was accepted
        self.auth = AuthTable(S, dev) if self.enforce_acl else None
        self._auth_clear = set()
        self.perms = AclIdentity(self.d_addrs, auth=self.auth) \
            if self.enforce_acl else None
        self.gs.auth_table = self.auth
        self._rows_dirty = True
        # -- the cut and the pack ---------------------------------------------
        self.h_raw = _pinned(self.raw_cap, U8, dev)
        self.mv_raw = memoryview(self.h_raw.numpy())
        self.d_raw = torch.zeros(self.raw_cap, dtype=U8, device=dev)
        self.d_rx = torch.zeros(self.raw_cap, dtype=U8, device=dev)
        self.d_take = torch.zeros(S, dtype=I64, device=dev)
        self.d_nfr = torch.zeros(S, dtype=I32, device=dev)
        self.d_flag = torch.zeros(S, dtype=I32, device=dev)
        self.d_fault = torch.zeros(1, dtype=I64, device=dev)
        self.d_over_rx = torch.zeros(1, dtype=I64, device=dev)
        L = _lib.lib()
        self.scan_ws = torch.empty(L.scan_workspace(4 * S), dtype=I64,
                                   device=dev)
        # -- the TX assembly --------------------------------------------------
        self.d_owner = torch.zeros(SLOTS, dtype=I64, device=dev)
        self.d_pstream = torch.zeros(4 * S, dtype=I32, device=dev)
        self.d_psrc = torch.zeros(4 * S, dtype=I64, device=dev)
        self.d_plen = torch.zeros(4 * S, dtype=I64, device=dev)
        self.d_poff = torch.zeros(4 * S + 1, dtype=I64, device=dev)
        self.d_fstats = torch.zeros(8, dtype=I64, device=dev)
        self.d_over_tx = torch.zeros(1, dtype=I64, device=dev)
        # a tick's bytes: its replies, the write-fired and the close-fired
        # notifications (notif_buf each) and the catch-up's (32 bytes of
        # frame around a listed path of at least 4 bytes of the requests)
        self.tx_cap = int(out_cap) + 2 * int(self.gs.notif_buf.numel()) + \
            10 * self.raw_cap + 4096
        self.d_tx = torch.zeros(self.tx_cap, dtype=U8, device=dev)
        self.h_tx = _pinned(self.tx_cap, U8, dev)
        self.mv_tx = memoryview(self.h_tx.numpy())
        # (with enforce_acl one word more, the last: replies answered NO_AUTH)
        # (on a tree with an ACL table one word before it: SET_ACL frames
        # their node's rounds did not reach)
        self.serve_setacl = tree.acl is not None
        self.nrep = 4 * S + 1 + (_R_NORD if P else _R_N) + \
            (1 if self.serve_setacl else 0) + (1 if self.enforce_acl else 0)
        # the ordered tick: the cut's write counts, what the serve deferred;
        # a connection advances by `used`, not by `take`
        self.d_nwr = torch.zeros(S, dtype=I32, device=dev)
        self.defer = OrderDefer(S, dev) if P else None
        self.d_adv = self.defer.used if P else self.d_take
        self.d_report = torch.zeros(self.nrep, dtype=I64, device=dev)
        self.h_report = _pinned(self.nrep, I64, dev)
        self.np_report = self.h_report.numpy()
        self.d_none = torch.zeros(1, dtype=I64, device=dev)
        self.d_empty = torch.empty(0, dtype=U8, device=dev)
        # -- host state ---------------------------------------------------------
        self.rows = [None] * S
        self.free_rows = list(range(S))
        self.free_slots = list(range(SLOTS))
        self.sessions = {}                # sid -> _Sess
        self.new = []                     # connections before their handshake
        self._rot = 0
        self._stats = dict.fromkeys(
            ('ticks', 'frames', 'bytes_in', 'bytes_out', 'connections',
             'bad_length', 'no_watcher_slot', 'dup_slot', 'batches_lost',
             'bad_batches', 'catchup_events', 'expiry_passes',
             'sessions_expired', 'sessions_closed', 'handshakes',
             'host_reads', 'max_reads_per_tick', 'deferred_frames',
             'max_writes_per_tick', 'order_max_rank', 'order_scratch_full',
             'acl_denied', 'setacl_unreached'),
            0)
        self._calls = []
        self._lock = threading.Lock()
        self._stop = False
        self.error = None
        self.host = host
        self.lsock = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
        self.lsock.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        self.lsock.bind((host, port))
        self.lsock.listen(512)
        self.lsock.setblocking(False)
        self.port = self.lsock.getsockname()[1]
        self.wake_r, self.wake_w = socket.socketpair()
        self.wake_r.setblocking(False)
        self.wake_w.setblocking(False)
        self.sel = selectors.DefaultSelector()
        self.sel.register(self.lsock, selectors.EVENT_READ, 'accept')
        self.sel.register(self.wake_r, selectors.EVENT_READ, 'wake')
        torch.cuda.synchronize(dev)
        self.thread = threading.Thread(target=self._run, name='gpu-zk',
                                       daemon=True)
        self.thread.start()

    # -- the surface ------------------------------------------------------------

    @property
    def address(self):
        return {'address': self.host, 'port': self.port}

    def servers(self):
        return [self.address]

    def call(self, fn, timeout=10.0):
        """Run ``fn()`` on the server's thread between two ticks, on the
        server's stream, and return its result (or raise what it raised)."""
        if threading.current_thread() is self.thread:
            return fn()
        if self.error is not None:
            raise RuntimeError('GpuZKServer: the server thread failed') \
                from self.error
        box = {'ev': threading.Event()}
        with self._lock:
            self._calls.append((fn, box))
        self._wake()
        if not box['ev'].wait(timeout):
            raise TimeoutError('GpuZKServer.call: the server did not answer')
        if 'err' in box:
            raise box['err']
        return box['val']

    def stats(self):
        """The front end's counters — ``ticks``, ``frames``, ``bytes_in``,
        ``bytes_out``, ``connections`` (open now), ``bad_length``
        (connections dropped for one), ``no_watcher_slot`` (sessions that
        found the 64 slots taken), ``watcher_slots`` (taken now),
        ``dup_slot``, ``batches_lost`` (ticks whose reply or TX encode
        overflowed: the writes are applied, the replies lost, the batch's
        connections dropped), ``bad_batches`` (ticks the serve refused:
        ``session_stats()['bad']`` was not 0), ``catchup_events``,
        ``sessions_expired``, ``sessions_closed``, ``max_reads_per_tick``
        (device-to-host synchronisations of the costliest tick); with
        ``order_passes``: ``deferred_frames`` (frames a tick took and left
        for a later one; they are not in ``frames``), ``max_writes_per_tick``
        (write frames the costliest tick's cut took, deferred ones included),
        ``order_max_rank`` (the longest chain of conflicting requests a tick
        saw; ``>= order_passes``: it deferred) and ``order_scratch_full``
        (ticks in which a snapshot found no room in the tree's scratch tail:
        the request was answered SYSTEMERROR, a SET_DATA among them after it
        was applied); on a tree with an ACL table: ``setacl_unreached``
        (SET_ACL frames answered SYSTEMERROR because their node's rounds of
        the tick ran out, as of the last tick's report); with
        ``enforce_acl``: ``acl_denied`` (requests
        answered NO_AUTH, as of the last tick's report) — and the last batch's
        ``session_stats``, ``watch_stats``, ``resume_stats`` and
        ``close_stats``, each read once; with ``enforce_acl`` also
        ``auth_stats`` (``GpuServer.auth_stats``: the AUTH frames served since
        the server started), read the same way."""
        def go():
            st = dict(self._stats)
            st['connections'] = sum(1 for c in self.rows if c is not None)
            st['sessions'] = len(self.sessions)
            st['watcher_slots'] = SLOTS - len(self.free_slots)
            for name in ('session_stats', 'watch_stats', 'resume_stats',
                         'close_stats'):
                try:
                    st[name] = getattr(self.gs, name)()
                except ValueError:
                    st[name] = None
            if self.enforce_acl:
                st['auth_stats'] = self.gs.auth_stats()
            return st
        return self.call(go)

    def disconnect(self, sid):
        """Close session ``sid``'s connection from the server side (the
        session stays); on the server's thread (:meth:`call`).  True when
        there was one."""
        s = self.sessions.get(sid)
        if s is None or s.conn is None:
            return False
        self._close_conn(s.conn)
        return True

    def shutdown(self):
        """Stop the thread, join it within 5 s and close every socket."""
        self._stop = True
        self._wake()
        self.thread.join(5.0)
        for c in list(self.rows) + list(self.new):
            if c is not None:
                self._close_sock(c.sock)
        for s in (self.lsock, self.wake_r, self.wake_w):
            self._close_sock(s)
        try:
            self.sel.close()
        except (OSError, ValueError):
            pass

    # -- the thread -------------------------------------------------------------

    def _wake(self):
        try:
            self.wake_w.send(b'x')
        except (BlockingIOError, OSError):
            pass

    @staticmethod
    def _close_sock(sock):
        try:
            sock.close()
        except OSError:
            pass

    def _run(self):
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            while not self._stop:
                try:
                    self._turn()
                except Exception as e:              # noqa: BLE001
                    if not self._stop:
                        self.error = e              # call() reports it
                    break
            self.stream.synchronize()
        with self._lock:
            calls, self._calls = self._calls, []
        for _, box in calls:
            box['err'] = RuntimeError('GpuZKServer: the server stopped')
            box['ev'].set()

    def _turn(self):
        busy = self._pending()
        for key, mask in self.sel.select(0 if busy else self.tick_s):
            what = key.data
            if what == 'accept':
                self._accept()
            elif what == 'wake':
                try:
                    self.wake_r.recv(4096)
                except (BlockingIOError, OSError):
                    pass
            else:
                if mask & selectors.EVENT_READ and not what.dead:
                    self._read(what)
                if mask & selectors.EVENT_WRITE and not what.dead:
                    self._flush(what)
        with self._lock:
            calls, self._calls = self._calls, []
        for fn, box in calls:
            try:
                box['val'] = fn()
            except Exception as e:                  # noqa: BLE001
                box['err'] = e
            box['ev'].set()
        if self._stop:
            return
        self._handshakes()
        self._expire()
        self._tick()

    def _pending(self):
        return any(c is not None and c.live and not c.closing and
                   len(c.inbuf) >= 4 and len(c.inbuf) != c.stalled
                   for c in self.rows)

    # -- sockets ----------------------------------------------------------------

    def _accept(self):
        for _ in range(64):
            try:
                sock, peer = self.lsock.accept()
            except (BlockingIOError, OSError):
                return
            if not self.free_rows:
                self._close_sock(sock)
                continue
            sock.setblocking(False)
            sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
            c = _Conn(sock, heapq.heappop(self.free_rows))
            self.rows[c.row] = c
            self.np_addrs[c.row] = peer_ipv4(peer)
            self._auth_clear.add(c.row)
            self._rows_dirty = True
            self.new.append(c)
            self.sel.register(sock, selectors.EVENT_READ, c)

    def _read(self, c):
        try:
            b = c.sock.recv(1 << 18)
        except (BlockingIOError, InterruptedError):
            return
        except OSError:
            b = b''
        if not b:
            self._close_conn(c)
            return
        if c.closing:
            return                                  # nothing of it is served
        c.inbuf += b
        if c.sess is not None:
            c.sess.last = time.monotonic()

    def _send(self, c, data):
        """``data`` (bytes-like) to the socket: one send, the unsent tail is
        kept and retried when the socket is writable."""
        if c.dead or len(data) == 0:
            return
        if not c.out:
            try:
                n = c.sock.send(data)
            except (BlockingIOError, InterruptedError):
                n = 0
            except OSError:
                self._close_conn(c)
                return
            self._stats['bytes_out'] += n
            if n == len(data):
                return
            data = data[n:]
        c.out += data
        self._want_write(c, True)

    def _flush(self, c):
        if c.out:
            try:
                n = c.sock.send(c.out)
            except (BlockingIOError, InterruptedError):
                n = 0
            except OSError:
                self._close_conn(c)
                return
            self._stats['bytes_out'] += n
            del c.out[:n]
        if not c.out:
            self._want_write(c, False)
            if c.closing:
                self._close_conn(c)

    def _want_write(self, c, on):
        if c.dead or c.writing == on:
            return
        c.writing = on
        ev = selectors.EVENT_READ | (selectors.EVENT_WRITE if on else 0)
        try:
            self.sel.modify(c.sock, ev, c)
        except (KeyError, ValueError, OSError):
            pass

    def _close_after_send(self, c):
        """Close once what is queued for the socket has gone out."""
        if c.dead:
            return
        c.closing = True
        c.inbuf.clear()
        if not c.out:
            self._close_conn(c)

    def _close_conn(self, c):
        """Close the connection now.  Its session, if any, stays (until its
        timer or its CLOSE_SESSION ends it) and loses its watches, as
        ZooKeeper keeps them on the connection."""
        if c.dead:
            return
        c.dead = True
        try:
            self.sel.unregister(c.sock)
        except (KeyError, ValueError, OSError):
            pass
        self._close_sock(c.sock)
        if c in self.new:
            self.new.remove(c)
        s = c.sess
        if s is not None and s.conn is c:
            s.conn = None
            if s.wslot >= 0:
                self.tree.watch_drop(s.wslot)
        c.sess = None
        r = c.row
        self.rows[r] = None
        self.np_sessions[r] = 0
        self.np_wslots[r] = -1
        self.np_sidx[r] = 0
        self.np_addrs[r] = 0
        self._auth_clear.add(r)
        self._rows_dirty = True
        heapq.heappush(self.free_rows, r)

    def _end_session(self, s):
        """The session is over on the device: its slot and bookkeeping."""
        if self.sessions.pop(s.sid, None) is None:
            return
        if s.wslot >= 0:
            heapq.heappush(self.free_slots, s.wslot)
            s.wslot = -1
        c, s.conn = s.conn, None
        if c is not None:
            c.sess = None
            self._close_after_send(c)

    # -- new connections --------------------------------------------------------

    def _handshakes(self):
        """A new connection's first frame is its ConnectRequest: the host
        cuts this one frame (one length word a connection) and the frames go
        to the session table in groups of at most 64."""
        ready = []
        for c in list(self.new):
            if len(c.inbuf) < 4:
                continue
            n = struct.unpack_from('>i', c.inbuf, 0)[0]
            if n < 0 or n > _HS_MAX:
                self._close_conn(c)
            elif len(c.inbuf) >= 4 + n:
                frame = bytes(c.inbuf[:4 + n])
                del c.inbuf[:4 + n]
                self.new.remove(c)
                ready.append((c, frame))
        for k in range(0, len(ready), 64):
            self._connect_group(ready[k:k + 64])

    def _connect_group(self, group):
        k = len(group)
        raw = b''.join(f for _, f in group)
        n_new = sum(1 for _, f in group
                    if len(f) >= 28 and f[20:28] == b'\0' * 8)
        rx = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(self.dev)
        resp, rsid, oc = self.table.connect(rx, len(raw), n_new)
        nb = _lib.CR_RESP_BYTES * k
        # the answers, the bound ids and the outcomes: one read a group
        h = torch.cat([rsid[:k], oc[:k].to(I64),
                       resp[:nb].to(I64)]).cpu().numpy()
        self._stats['host_reads'] += 1
        self._stats['handshakes'] += k
        body = h[2 * k:].astype(np.uint8).tobytes()
        now = time.monotonic()
        for i, (c, _) in enumerate(group):
            ans = body[41 * i:41 * i + 41]
            sid, outcome = int(h[i]), int(h[k + i])
            if c.dead:
                continue
            if sid == 0 or outcome not in (_lib.SC_NEW, _lib.SC_RESUMED):
                # expired or unknown: its answer, then a close
                self._send(c, ans)
                self._close_after_send(c)
                continue
            self._bind(c, sid, struct.unpack_from('>i', ans, 8)[0], now)
            self._send(c, ans)

    def _bind(self, c, sid, timeout, now):
        s = self.sessions.get(sid)
        if s is None:
            wslot = -1
            if self.free_slots:
                wslot = heapq.heappop(self.free_slots)
            else:
                self._stats['no_watcher_slot'] += 1
            s = _Sess(sid, (sid & 0x00ffffffffffffff) - 1, wslot, timeout,
                      now)
            self.sessions[sid] = s
        elif s.conn is not None and s.conn is not c:
            # the session moves: the older connection is closed first and
            # nothing more of it is served
            self._close_conn(s.conn)
        s.timeout, s.last, s.conn = timeout, now, c
        c.sess, c.live = s, True
        r = c.row
        self.np_sessions[r] = sid
        self.np_wslots[r] = s.wslot
        self.np_sidx[r] = s.idx
        self._rows_dirty = True

    # -- a tick -------------------------------------------------------------------

    def _upload_rows(self):
        if self._rows_dirty:
            self.d_sessions.copy_(self.h_sessions, non_blocking=True)
            self.d_wslots.copy_(self.h_wslots, non_blocking=True)
            self.d_sidx.copy_(self.h_sidx, non_blocking=True)
            if self.enforce_acl:
                self.d_addrs.copy_(self.h_addrs, non_blocking=True)
                if self._auth_clear:
                    rows = torch.tensor(sorted(self._auth_clear), dtype=I64)
                    self.auth.clear(rows.to(self.dev))
                    self._auth_clear.clear()
            self._rows_dirty = False

    def _assemble(self, rep_off, out, err, resume, notif, close,
                  rep_end=None):
        """The TX assembly on the device: the pieces, the scan, the gather.
        ``resume`` / ``notif`` / ``close``: (stream, slot_off) or None;
        ``rep_end``: where the connections' replies end (the ordered tick)."""
        S = self.max_conns
        pairs = (resume, notif, close)
        streams = [out if out is not None else self.d_empty] + \
            [p[0] if p is not None else self.d_empty for p in pairs]
        offs = [p[1] if p is not None else None for p in pairs]
        _lib.front_tx_pieces(rep_off, self.d_wslots, offs[0], offs[1],
                             offs[2], err, [int(s.numel()) for s in streams],
                             self.d_owner, self.d_pstream, self.d_psrc,
                             self.d_plen, self.d_fstats, rep_end)
        _lib.lib().scan_excl(self.d_plen, self.d_poff, self.d_poff[4 * S:],
                             self.scan_ws)
        _lib.front_gather(streams, self.d_pstream, self.d_psrc, self.d_poff,
                          4 * S, self.d_tx, self.d_over_tx)

    def _report(self, words):
        """The report and ``tx[:total]`` to pinned memory: two reads.
        Returns (report, total)."""
        S = self.max_conns
        flag = self.d_flag
        if self.order_passes:
            flag = flag + (self.d_adv < self.d_take) * _F_DEFER
        torch.cat([self.d_adv, flag.to(I64),
                   self.table.state.index_select(0, self.d_sidx).to(I64),
                   self.d_poff[0::4]] + words, out=self.d_report)
        self.h_report.copy_(self.d_report, non_blocking=True)
        self.stream.synchronize()
        rep = self.np_report
        reads = 1
        total = int(rep[4 * S])
        if rep[4 * S + 1 + _R_OVER_TX] != 0:
            total = 0
        if total > 0:
            self.h_tx[:total].copy_(self.d_tx[:total], non_blocking=True)
            self.stream.synchronize()
            reads += 1
        self._stats['host_reads'] += reads
        self._stats['max_reads_per_tick'] = max(
            self._stats['max_reads_per_tick'], reads)
        return rep, total

    def _deliver(self, rep, total):
        """One send a connection from the pinned TX buffer."""
        S = self.max_conns
        if total <= 0:
            return
        txo = rep[3 * S:4 * S + 1]
        for r in np.nonzero(np.diff(txo))[0].tolist():
            c = self.rows[r]
            if c is not None:
                self._send(c, self.mv_tx[int(txo[r]):int(txo[r + 1])])

    def _tick(self):
        S = self.max_conns
        act = [c for c in self.rows
               if c is not None and c.live and not c.closing and
               len(c.inbuf) >= 4 and len(c.inbuf) != c.stalled]
        if not act:
            return                                  # nothing is launched
        if len(act) > self.cap_frames:
            # more active connections than frames: they take turns
            k = self._rot % len(act)
            act = (act[k:] + act[:k])[:self.cap_frames]
            self._rot += self.cap_frames
        quota = max(1, self.cap_frames // len(act))
        room = self.raw_cap
        lens = np.zeros(S, dtype=np.int64)
        for c in act:
            n = min(len(c.inbuf), room)
            lens[c.row] = n
            room -= n
        self.np_rstarts[0] = 0
        np.cumsum(lens, out=self.np_rstarts[1:])
        nup = int(self.np_rstarts[S])
        for c in act:
            n = int(lens[c.row])
            if n:
                a = int(self.np_rstarts[c.row])
                self.mv_raw[a:a + n] = c.inbuf[:n]
        # the batch's buffer: a view of a few sizes, so that the buffers the
        # serve sizes from it settle
        cover = 4096
        while cover < nup:
            cover <<= 1
        rx = self.d_rx[:min(cover, self.raw_cap)]
        gs = self.gs
        self.d_raw[:nup].copy_(self.h_raw[:nup], non_blocking=True)
        self.d_rstarts.copy_(self.h_rstarts, non_blocking=True)
        self._upload_rows()
        P = self.order_passes
        _lib.front_cut(self.d_raw, nup, self.d_rstarts, quota,
                       consts.MAX_PACKET, self.d_take, self.d_nfr,
                       self.d_flag, self.d_fault,
                       mode=(1 if P else 0) + (2 if self.serve_setacl else 0),
                       has_acl=self.tree.acl is not None,
                       nwr=self.d_nwr if P else None)
        _lib.lib().scan_excl(self.d_take, self.d_starts, self.d_starts[S:],
                             self.scan_ws)
        _lib.front_gather([self.d_raw], None, self.d_rstarts, self.d_starts,
                          S, rx, self.d_over_rx)
        if P:
            out, _, err, _ = gs.serve_sessions_mixed(
                rx, self.d_starts[S:], self.segs, table=self.table,
                resume=True, close=True, ordered=True, passes=P,
                defer=self.defer, perms=self.perms,
                setacl=self.serve_setacl)
        else:
            out, _, err, _ = gs.serve_sessions_mixed(
                rx, self.d_starts[S:], self.segs, table=self.table,
                resume=True, close=True, perms=self.perms,
                setacl=self.serve_setacl)
        self._assemble(gs.seg.rep_off, out, err,
                       (gs.resume_notif[0], gs.resume_slots[1]),
                       (gs.notif[0], gs.notif_slots[1]),
                       (gs.close_notif[0], gs.close_slots[1]),
                       self.defer.rep_end if P else None)
        words = [
            self.d_fault, self.d_over_rx, self.d_over_tx,
            err.reshape(-1)[:1].to(I64), gs.seg.bad[0:1],
            self.d_fstats[0:1], self.d_nfr.sum().reshape(1),
            gs.resume_counters()[0:1]]
        if P:
            words += [self.defer.deferred, self.d_nwr.sum().reshape(1),
                      gs.order_counters()]
        if self.serve_setacl:
            words += [gs.setacl_counters()[4:5]]
        if self.enforce_acl:
            words += [gs.acl_enforce_counters()[3:4]]
        rep, total = self._report(words)
        st = self._stats
        st['ticks'] += 1
        words = rep[4 * S + 1:]
        st['frames'] += int(words[_R_FRAMES])
        if P:
            st['frames'] -= int(words[_R_DEFER])
            st['deferred_frames'] += int(words[_R_DEFER])
            st['max_writes_per_tick'] = max(st['max_writes_per_tick'],
                                            int(words[_R_NWR]))
            st['order_max_rank'] = max(st['order_max_rank'],
                                       int(words[_R_RANK]))
            if words[_R_SCRATCH] > self.tree.scratch.numel():
                st['order_scratch_full'] += 1
        if self.serve_setacl:                       # (the server's own sum)
            st['setacl_unreached'] = int(words[_R_NORD if P else _R_N])
        if self.enforce_acl:
            st['acl_denied'] = int(words[-1])       # (the server's own sum)
        st['dup_slot'] += int(words[_R_DUP])
        st['catchup_events'] += int(words[_R_CATCHUP])
        if words[_R_BAD] != 0:
            st['bad_batches'] += 1
        self._deliver(rep, total)
        lost = words[_R_ERR] != 0 or words[_R_OVER_TX] != 0 or \
            words[_R_FAULT] != 0 or words[_R_OVER_RX] != 0
        if lost:
            st['batches_lost'] += 1
        take, flag, state = rep[0:S], rep[S:2 * S], rep[2 * S:3 * S]
        for c in act:
            if c.dead:
                continue
            r = c.row
            t = int(take[r])
            st['bytes_in'] += t
            if lost:
                self._close_conn(c)
                continue
            del c.inbuf[:t]
            c.stalled = -1
            s = c.sess
            if s is not None and state[r] != _SS_ALIVE:
                # its CLOSE_SESSION was served (or the table no longer holds
                # it): the reply is on its way, then the connection closes
                st['sessions_closed'] += 1
                self._end_session(s)
            elif flag[r] & _F_DEFER:
                pass                                # the rest: the next tick
            elif flag[r] & _F_BAD:
                st['bad_length'] += 1
                self._close_after_send(c)
            elif t == 0:
                if lens[r] >= self.raw_cap:
                    self._close_conn(c)             # a frame no tick can hold
                elif lens[r] == len(c.inbuf):
                    c.stalled = len(c.inbuf)        # until more arrives

    # -- expiry -----------------------------------------------------------------

    def _expire(self):
        """Sessions past their negotiated timeout since they were last heard
        from: one close_sessions call, its close_notif slices to the watchers
        with the same TX assembly (only the close stream is present)."""
        if not self.sessions:
            return
        now = time.monotonic()
        due = [s for s in self.sessions.values()
               if (now - s.last) * 1000.0 > s.timeout]
        if not due:
            return
        due = due[:self.max_conns]
        gs = self.gs
        dev = self.dev
        sids = torch.tensor([s.sid for s in due], dtype=I64, device=dev)
        wsl = torch.tensor([s.wslot for s in due], dtype=I32, device=dev)
        self._upload_rows()
        gs.close_sessions(sids, wsl, table=self.table)
        self.d_take.zero_()
        if self.order_passes:
            self.d_adv.zero_()
        self.d_flag.zero_()
        self._assemble(None, None, None, None, None,
                       (gs.close_notif[0], gs.close_slots[1]))
        rep, total = self._report([
            self.d_none, self.d_none, self.d_over_tx, self.d_none,
            self.d_none, self.d_fstats[0:1], self.d_none, self.d_none] +
            [self.d_none] * ((4 if self.order_passes else 0) +
                             (1 if self.serve_setacl else 0) +
                             (1 if self.enforce_acl else 0)))
        self._stats['expiry_passes'] += 1
        self._stats['sessions_expired'] += len(due)
        self._deliver(rep, total)
        for s in due:
            self._end_session(s)
