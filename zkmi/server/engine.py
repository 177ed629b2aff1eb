"""The GPU server's serve engine: :class:`GpuServer` scans and decodes a
request stream, applies it to a :class:`~zkmi.server.tree.GpuTree` and
encodes the replies and the watchers' notifications, all on the device."""

import time
from types import SimpleNamespace

import torch

from .. import consts
from ..ops import _lib, batch as B

I64, I32, U8 = torch.int64, torch.int32, torch.uint8

# the largest batch tree_seq_order numbers
_SEQ_MAX = 1 << 24


class _SubFrames(object):
    """One engine's class of a mixed batch: the compacted frame table the
    split wrote (``off``, ``length``) and its device ``count``."""

    def __init__(self, off, length, count):
        self.off, self.length, self.count = off, length, count


class SessionSegments(object):
    """The segment table of a session batch (:meth:`GpuServer.
    serve_sessions`; the rule: csrc/kernels/zk_sess.h): the batch is the
    whole frames of ``S`` connections, concatenated; connection s's bytes are
    ``rx[starts[s]:starts[s + 1]]``, its EPHEMERAL creates belong to
    ``sessions[s]`` and its reads arm watcher slot ``wslots[s]`` (-1: none).
    Device tensors: ``starts`` int64 [S + 1] (non-decreasing, ``starts[0]``
    0), ``sessions`` int64 [S], ``wslots`` int32 [S]."""

    def __init__(self, starts, sessions, wslots):
        S = int(sessions.numel())
        if S < 1 or int(starts.numel()) != S + 1 or int(wslots.numel()) != S:
            raise ValueError('SessionSegments: starts [S + 1], sessions [S] '
                             'and wslots [S] with S >= 1')
        self.starts, self.sessions, self.wslots = starts, sessions, wslots
        self.S = S


class AclIdentity(object):
    """Who the connections of a session batch are, for the ACL check of
    ``serve_sessions_mixed(perms=...)`` (the rule: csrc/kernels/
    zk_aclperm.h): ``addrs``, a device int32 [S] tensor, segment s's peer
    IPv4 address as a host-order 32-bit word (10.1.2.9 is ``0x0A010209``; a
    value past 2^31 as its two's complement) or 0 for a peer without one,
    which no ``ip`` entry matches.  ``auth`` (an :class:`AuthTable` of at
    least S rows, or None): the batch's AUTH frames are served and a
    ``digest`` entry matches a connection that holds its id."""

    def __init__(self, addrs, auth=None):
        if addrs.dtype != I32 or addrs.dim() != 1 or addrs.numel() < 1:
            raise ValueError('AclIdentity: addrs is an int32 [S] tensor')
        self.addrs = addrs
        self.S = int(addrs.numel())
        if auth is not None and (not isinstance(auth, AuthTable) or
                                 auth.S < self.S):
            raise ValueError('AclIdentity: auth is an AuthTable of at least '
                             'S rows')
        self.auth = auth


class AuthTable(object):
    """The ``digest`` identities the connections of a session batch hold
    after AUTH (csrc/kernels/tree_auth.hip; the rule and the record layout:
    zk_auth.h).  ZooKeeper keeps authentication per connection, not per
    session, so row s belongs to segment s.  Device tensors: ``recs`` uint8
    [S, 4 * 160] (four records a row: the id's length as a native int32, then
    up to 148 id bytes), ``cnt`` int32 [S] (records claimed; a reader clamps
    it to 4) and ``stats`` int64 [8] (``_lib.AUTH_STATS``)."""

    def __init__(self, S, device):
        self.S = int(S)
        if self.S < 1:
            raise ValueError('AuthTable: S >= 1')
        self.recs = torch.zeros(self.S, _lib.AUTH_K * _lib.AUTH_REC,
                                dtype=U8, device=device)
        self.cnt = torch.zeros(self.S, dtype=I32, device=device)
        self.stats = torch.zeros(8, dtype=I64, device=device)
        self.tensors = [self.recs, self.cnt, self.stats]

    def clear(self, rows):
        """Forget the identities of ``rows`` (a device int64 index tensor):
        a connection has gone or a new one takes the row.  The counts and
        the records are zeroed (a record is written once between two
        clears, which the store relies on); no host read."""
        self.cnt.index_fill_(0, rows, 0)
        self.recs.index_fill_(0, rows, 0)

    def identities(self):
        """Per row the identities stored, as ``bytes`` (host reads: for
        tests and tools)."""
        cnt = self.cnt.cpu().tolist()
        recs = self.recs.cpu().numpy()
        out = []
        for s in range(self.S):
            row = []
            for k in range(min(max(cnt[s], 0), _lib.AUTH_K)):
                rec = recs[s, k * _lib.AUTH_REC:(k + 1) * _lib.AUTH_REC]
                n = int(rec[:4].view('<i4')[0])
                row.append(bytes(rec[4:4 + n]))
            out.append(row)
        return out


class OrderDefer(object):
    """Where ``serve_sessions_mixed(ordered=True, defer=...)`` leaves what it
    deferred, for a table of ``S`` segments; all device tensors, nothing is
    read back:

    ``clipf``     int64 [S]: the first deferred frame of segment s, an index
                  in the whole batch's frame table (``cap_frames``: none);
    ``rep_end``   int64 [S]: connection s's replies are ``out[rep_off[s]:
                  rep_end[s]]`` (the placeholders of its deferred frames lie
                  behind and are never sent);
    ``used``      int64 [S]: the request bytes of segment s that were
                  consumed; the rest, from its first deferred frame on, is to
                  be sent again in the next batch;
    ``deferred``  int64 [1]: the frames deferred."""

    def __init__(self, S, device):
        self.S = int(S)
        self.clipf = torch.zeros(self.S, dtype=I64, device=device)
        self.rep_end = torch.zeros(self.S, dtype=I64, device=device)
        self.used = torch.zeros(self.S, dtype=I64, device=device)
        self.deferred = torch.zeros(1, dtype=I64, device=device)


class _SegState(object):
    """What :meth:`GpuServer.serve_sessions` leaves on the device about the
    last session batch's segments."""

    def __init__(self, cap_frames, S, dev):
        self.S = S
        self.f_seg = torch.zeros(cap_frames, dtype=I32, device=dev)
        self.first = torch.zeros(S + 1, dtype=I64, device=dev)
        self.rep_off = torch.zeros(S + 1, dtype=I64, device=dev)
        self.state = torch.zeros(S, dtype=I32, device=dev)
        self.bad = torch.zeros(2, dtype=I64, device=dev)
        self.f_seg_c = None               # per engine class (lazy)

    def class_tables(self):
        """``f_seg`` through the split of a batch of any op mix
        (:meth:`GpuServer.serve_sessions_mixed`): three int32 [cap_frames]
        tables, class c's frame -> segment; allocated on first use."""
        if self.f_seg_c is None:
            cap = int(self.f_seg.numel())
            buf = torch.zeros(3 * cap, dtype=I32, device=self.f_seg.device)
            self.f_seg_c = [buf[c * cap:(c + 1) * cap] for c in range(3)]
        return self.f_seg_c

    def table(self, segs, cls=None):
        """The segment table as the session ops take it, ``[f_seg, sessions,
        wslots, seg_state, bad]``, of :class:`SessionSegments` ``segs``: the
        whole batch's, or with ``cls`` engine class ``cls``'s."""
        f_seg = self.f_seg if cls is None else self.class_tables()[cls]
        return [f_seg, segs.sessions, segs.wslots, self.state, self.bad]


def _table_args(table):
    """The keywords through which a session op takes a
    :class:`GpuSessionTable` (or none)."""
    if table is None:
        return {'table': None, 'server_id': 0, 'span': 0}
    return {'table': table._tensors, 'server_id': table.server_id,
            'span': table.span}


def _notif_batch(poff, plen, arena, ntype, count, cap, dev):
    """ResponseBatch of `cap` notification records (xid -1, zxid -1)."""
    return B.ResponseBatch(
        torch.full((cap,), consts.OP_CODES['NOTIFICATION'], dtype=I32,
                   device=dev),
        torch.full((cap,), consts.XID_NOTIFICATION, dtype=I32, device=dev),
        torch.zeros(cap, dtype=I32, device=dev),
        torch.full((cap,), -1, dtype=I64, device=dev),
        torch.full((cap,), -1, dtype=I64, device=dev),
        poff, plen, arena, ntype, count)


class _NotifStream(object):
    """One notification stream of a :class:`GpuServer`, on the device:
    ``ecap`` event records [watcher slot, type, path offset, path length] —
    ``ev`` as they were found, ``g`` grouped by watcher slot —, ``ev_total``
    ([events written (<= ecap), events found]), their K13 encode in ``buf``
    as xid -1 frames (``NOTIFICATION``, state SyncConnected; paths in
    ``arena``) and ``slots = (first, off)``, both [65]: watcher w's frames
    are ``buf[off[w]:off[w + 1]]`` once :func:`_lib.sess_ranges` ran.

    ``ws_words``: the int64 words the kernel that groups the records needs.
    Without it only the raw half is allocated (uninitialised: written before
    it is read), with a batch of its own; :meth:`group_half` adds the rest."""

    def __init__(self, ecap, buf_bytes, arena, dev, ws_words=None):
        self.ecap, self.arena, self.dev = ecap, arena, dev
        self.ev_total = torch.zeros(2, dtype=I64, device=dev)
        self.buf = torch.empty(buf_bytes, dtype=U8, device=dev)
        self.g = self.raw = None
        if ws_words is None:
            self.ev = self._records(torch.empty)
            self.raw = self._batch(self.ev)
        else:
            self.ev = self._records(torch.zeros)
            self.group_half(ws_words)

    def _records(self, fill):
        return [fill(self.ecap, dtype=t, device=self.dev)
                for t in (I32, I32, I64, I32)]

    def _batch(self, rec):
        return _notif_batch(rec[2], rec[3], self.arena, rec[1],
                            self.ev_total[0:1], self.ecap, self.dev)

    def group_half(self, ws_words):
        dev = self.dev
        self.g = self._records(torch.zeros)
        self.ws = torch.empty(ws_words, dtype=I64, device=dev)
        self.first = torch.zeros(_lib.SESS_SLOTS + 1, dtype=I64, device=dev)
        self.off = torch.zeros(_lib.SESS_SLOTS + 1, dtype=I64, device=dev)
        self.total_err = B._total_err(dev)
        self.rec_off = torch.zeros(self.ecap, dtype=I64, device=dev)
        self.resp = self._batch(self.g)
        self.slots = (self.first, self.off)

    def events(self, op, err, count, cap, fired, wbsum):
        """``count`` requests' fired masks -> ``ev``, in request order."""
        e = self.ev
        _lib.lib().watch_events(op, err, count, cap, fired, wbsum, e[0], e[1],
                                e[2], e[3], self.ev_total)

    def group(self):
        """``ev`` -> ``g`` (tree_sess.hip; request order inside a slot)."""
        e, g = self.ev, self.g
        _lib.sess_group_events(e[0], e[1], e[2], e[3], self.ev_total, self.ws,
                               g[0], g[1], g[2], g[3], self.first)

    def encode(self, store, grouped=True):
        """K13 over ``g`` (or ``ev``) into ``buf``: leaves ``self.notif =
        (buf, bytes, slot per frame, events)`` and returns the frame starts
        and the encoder's error flag."""
        kw = {'total_err': self.total_err, 'rec_off': self.rec_off} \
            if grouped else {}
        out, rec_off, total, err = B.encode_responses(
            self.resp if grouped else self.raw, store, self.buf.numel(),
            out=self.buf, **kw)
        self.notif = (out, total, (self.g if grouped else self.ev)[0],
                      self.ev_total[0:1])
        return rec_off, err

    def ranges(self):
        """The slot half of :func:`_lib.sess_ranges`' arguments."""
        return (self.first, self.rec_off, self.ev_total[0:1],
                self.total_err[0], self.total_err[1], self.off)


class GpuServer(object):
    """Server half of the pipeline: frame-scan + decode requests, apply them
    to a :class:`GpuTree`, encode replies."""

    def __init__(self, tree, cap_frames, out_cap, window=2048,
                 seq_order=True, group=1, fused_rows=False):
        self.tree = tree
        # fused_rows: :meth:`serve` scans the requests with K1's rows pass
        # deferred and the serve kernel reads the scan's tile lists (one
        # launch less; csrc/kernels/zk_frame_rows.h).  Only where the serve
        # is the frame table's first reader: unordered, no SEQUENTIAL
        # numbering, no ACL table, no watch resume.
        if fused_rows and (tree.acl is not None or
                           (seq_order and cap_frames <= _SEQ_MAX)):
            raise ValueError('fused_rows: the serve must be the first '
                             'reader of the frame table (no seq_order, no '
                             'ACL table)')
        self.fused_rows = fused_rows
        self.window = window              # K1 entry window of the requests
        # SEQUENTIAL creates numbered in stream order before each serve
        # (csrc/kernels/tree_seq.hip: five launches); a server whose
        # batches never carry one (the GET pipeline, the write mixes
        # without SEQUENTIAL) skips them.  Off, a SEQUENTIAL create still
        # gets a unique number, in arrival order.
        self.seq_order = seq_order and cap_frames <= _SEQ_MAX
        self.seq_ws = None
        self.seqno = None
        # batches of GET_DATA / EXISTS only (the GET pipeline): the serve's
        # read-only instance (no claim / free / dirty-parent barriers; any
        # other op is refused UNIMPLEMENTED)
        self.read_only = False
        dev = tree.device
        self.rt = B.alloc_request_table(cap_frames, dev)
        # CREATE replies carry the created path from the tree's arena
        # (a SEQUENTIAL name differs from the requested one)
        self.resp = B.ResponseBatch(
            torch.empty(cap_frames, dtype=I32, device=dev),
            torch.empty(cap_frames, dtype=I32, device=dev),
            torch.empty(cap_frames, dtype=I32, device=dev),
            torch.empty(cap_frames, dtype=I64, device=dev),
            torch.empty(cap_frames, dtype=I64, device=dev),
            torch.zeros(cap_frames, dtype=I64, device=dev),
            torch.zeros(cap_frames, dtype=I32, device=dev),
            tree.path_arena,
            torch.zeros(cap_frames, dtype=I32, device=dev), None,
            torch.empty(cap_frames, dtype=I64, device=dev))
        # the serve kernel sizes the replies itself (presized K13 encode)
        self.presized = B.response_workspace(cap_frames, dev)
        self.out = torch.empty(out_cap, dtype=U8, device=dev)
        self.cap_frames = cap_frames
        self.scanner = B.FrameScanner(cap_frames, dev, window=window,
                                      group=group)
        self.ows = None                   # ordered-serve workspace (lazy)
        self.total_err = B._total_err(dev)  # the reply encode's scalars
        self.notif = None
        self.seg = None                   # the last session batch's segments
        self.notif_slots = None           # (slot_first, slot_off) of its
        self._fired = None                # notifications (a _NotifStream)
        self.resume_notif = None          # the last SET_WATCHES catch-up
        self.resume_slots = None          # (slot_first, slot_off) of a
        self._caught = self._rs_stats = None  # session batch's (lazy)
        self.close_notif = None           # what the last close pass fired
        self.close_slots = None           # (slot_first, slot_off) of it
        self._cl = None                # (its buffers and stream: lazy)
        # the read engines' and the mix's buffers (lazy)
        self.list_want = self.list_ws = self.list_rec_off = None
        self.list_total_err = self.acl_rec_off = self.acl_total_err = None
        self.mix_cls = self.mix_sub = self.mix_foff = None
        self.mix_flen = self.mix_counts = self.mix_frames = None
        self.mix_split_ws = self.mix_merge_ws = self.mix_rec_off = None
        self.mix_total_err = self.mix_scratch = self.mix_out = None
        # the ACL check's verdicts and counters (lazy)
        self.acl_deny = self.acl_enf = None
        self.auth_res = self.auth_table = None
        # the SET_ACL pass's claim words, counters and workspace (lazy)
        self.setacl_claim = self.setacl_ctr = self.setacl_ws = None
        if tree.watch is not None:
            self._init_watch(cap_frames, dev)

    # -- watches --------------------------------------------------------------

    def _init_watch(self, cap, dev):
        """Buffers of the watch events of one batch: the masks each write
        fired (5 words per request) and the stream of their events."""
        self.ecap = ecap = 3 * cap + 64
        self.fired = torch.zeros(5 * cap, dtype=I64, device=dev)
        self.wbsum = torch.empty((cap + 255) // 256, dtype=I64, device=dev)
        # [events written, re-armed, events, listed paths dropped]
        self.rs_out = torch.zeros(4, dtype=I64, device=dev)
        # K13's error flag of the last notification / catch-up encode
        self.notif_err = self.resume_err = None
        self.exp_rec = None               # expiry records (lazy)
        # notification frame: 4 + 16 header + type + state + path
        self.maxpath = int(self.tree.node_path_len.max().item()) + 16
        w = _NotifStream(ecap, ecap * (28 + 4 + self.maxpath) + 64,
                         self.tree.path_arena, dev)
        self._fired, self.ev_slot, self.ev_total = w, w.ev[0], w.ev_total
        self.notif_buf = w.buf

    def _notify(self, op=None, err=None, count=None, fired=None,
                grouped=False):
        """Expand the fired masks of the last serve (or the records of an
        expiry: ``op`` .. ``fired``) into events (request order) and encode
        them: ``self.notif = (stream, bytes, slot per frame, events)`` — the
        watchers' notification frames, all on the device.  Events past
        ``self.ecap`` are not written (their watches are spent all the
        same) and the encoder's error flag is kept: :meth:`watch_stats`
        reports both.  ``grouped`` (a session batch): the events are grouped
        by watcher slot before K13 encodes them, so ``self.notif`` is
        slot-major and every watcher's notifications are one slice of it:
        ``self.notif_slots``, once :func:`_lib.sess_ranges` ran."""
        if op is None:
            r = self.resp
            op, err, count, fired = r.opcode, r.err, r.count, self.fired
        w = self._fired
        w.events(op, err, count, self.cap_frames, fired, self.wbsum)
        if grouped:
            if w.g is None:
                w.group_half(_lib.sess_group_workspace(self.ecap))
            w.group()
            self.notif_slots = w.slots
        self.notif_rec_off, self.notif_err = w.encode(self.tree.store, grouped)
        self.notif = w.notif

    def expire(self, session, wslot=None, removed=None):
        """Expire ``session``: its ephemerals are removed as one txn
        (:meth:`GpuTree.expire`) and, on a tree with a watch table, the
        watches the removals fire become ``self.notif`` as a served batch's
        do (NodeDeleted to the data and child watchers of each removed node,
        one a watcher; NodeChildrenChanged to its parent's), in no
        particular order.  ``wslot``: the expired session's watcher slot;
        its own watches are dropped first (:meth:`GpuTree.watch_drop`), as
        ZooKeeper drops a closed session's, so it is told nothing and the
        slot's next session inherits nothing.  Returns ``removed``.

        Room for ``cap_frames`` removals that fire a watch; more are counted
        in :meth:`watch_stats` and their events lost."""
        tree = self.tree
        if tree.watch is None:
            return tree.expire(session, removed)
        dev = tree.device
        if wslot is not None:
            tree.watch_drop(wslot)
        if self.exp_rec is None:
            cap = self.cap_frames
            self.exp_rec = torch.zeros(8 + 5 * cap, dtype=I64, device=dev)
            self.exp_op = torch.full((cap,), consts.OP_CODES['DELETE'],
                                     dtype=I32, device=dev)
            self.exp_err = torch.zeros(cap, dtype=I32, device=dev)
        removed = tree.expire(session, removed, rec=self.exp_rec)
        self._notify(self.exp_op, self.exp_err, self.exp_rec[0:1],
                     self.exp_rec[8:])
        return removed

    def watch_stats(self):
        """The watch path's loss counters (one host read), all 0 on a
        server that lost nothing:

        ``lost_arms``       watches that found no entry in a full table since
                            the tree was built (:meth:`GpuTree.watch_rehash`
                            is the remedy); their watchers will not be told
        ``events_fired``,   of the last serve / expiry: more fired than
        ``events_written``  written means ``ecap`` overflowed and the rest
                            were dropped, their watches spent
        ``encode_err``      the notification encoder's error flag of the last
                            serve / expiry (2: ``notif_buf`` too small)
        ``expiry_dropped``  removals of the last :meth:`expire` whose fired
                            watches found no record
        ``resume_dropped``, paths of the last SET_WATCHES catch-up that were
        ``resume_err``      neither answered nor re-armed; its encoder's flag
        """
        wh = self.tree.watch_hcap
        ev = self.ev_total.cpu().tolist()
        st = {'lost_arms':
              int(self.tree.watch[1][2 * wh + _lib.WS_LOST].item()),
              'events_fired': ev[1], 'events_written': ev[0],
              'encode_err': 0 if self.notif_err is None
              else int(self.notif_err.item()),
              'expiry_dropped': 0, 'resume_dropped': 0, 'resume_err': 0}
        if self.exp_rec is not None:
            st['expiry_dropped'] = max(
                0, int(self.exp_rec[0].item()) - self.cap_frames)
        if self.resume_err is not None:
            rs = self.rs_out.cpu().tolist()
            st['resume_dropped'] = rs[3] + rs[2] - rs[0]
            st['resume_err'] = int(self.resume_err.item())
        return st

    def _resume(self, rx, ft, wslot):
        """SET_WATCHES catch-up of the batch's SET_WATCHES frames for
        watcher ``wslot`` (csrc/kernels/tree_watch.hip wt_resume_k): events for
        what changed after relZxid, encoded with the request bytes as path
        arena; the other watches are re-armed."""
        L = _lib.lib()
        dev = self.tree.device
        # a listed path takes at least the 4 bytes of its length in its
        # frame: no list of this stream is longer than its bytes / 4
        cap = max(self.ecap, int(rx.numel()) // 4)
        ev_type = torch.empty(cap, dtype=I32, device=dev)
        ev_poff = torch.empty(cap, dtype=I64, device=dev)
        ev_plen = torch.empty(cap, dtype=I32, device=dev)
        ent = torch.empty(cap, dtype=I64, device=dev)
        L.watch_resume(self.tree.tensors, rx, ft.off, ft.length, ft.count,
                       self.cap_frames, wslot, ent, ev_type, ev_poff, ev_plen,
                       self.rs_out)
        nb = _notif_batch(ev_poff, ev_plen, rx, ev_type, self.rs_out[0:1],
                          cap, dev)
        # paths of a SET_WATCHES are bounded by its frame: ZooKeeper paths
        buf = torch.empty(cap * 32 + int(rx.numel()) + 64, dtype=U8,
                          device=dev)
        out, _, total, rerr = B.encode_responses(nb, self.tree.store,
                                                 buf.numel(), out=buf)
        self.resume_err = rerr
        self.resume_notif = (out, total, self.rs_out)

    def serve(self, rx, n, session=0, terminate=False, ordered=False,
              passes=4, wslot=-1, resume=False):
        """Serve the request stream ``rx[:n]`` for ``session`` (the owner of
        any EPHEMERAL node it creates).  ``n`` is a host length or the
        request encoder's device total (no host read).  Returns the reply
        stream buffer, its device total, the encoder error flag and the
        request frame table.

        ``ordered``: requests on one path are applied in stream order when
        one of them writes it (``passes`` launches; a path with more than
        ``passes`` requests in the batch has the excess answered
        SYSTEMERROR, see :meth:`order_stats`).  Reads and sets followed by
        a write to their path snapshot their reply into the tree's
        ``scratch``.  Without it requests of a batch are concurrent.

        On a tree with an ACL table (``GpuTree(acl_cap=...)``) every
        successful CREATE's ACL is recorded after the serve (two launches,
        csrc/kernels/tree_acl.hip).  A GET_ACL in the batch is answered
        UNIMPLEMENTED here: GET_ACL batches go through :meth:`serve_acl`,
        batches that mix it (or the list ops) with these through
        :meth:`serve_mixed`."""
        for _ in self.serve_steps(rx, n, session, terminate, ordered, passes,
                                  wslot, resume):
            pass
        return self.result

    def serve_steps(self, rx, n, session=0, terminate=False, ordered=False,
                    passes=4, wslot=-1, resume=False, frames=None):
        """:meth:`serve` as a generator yielding once, between the request
        decode and the tree; the return tuple lands in ``self.result`` (a
        pipelined caller interleaves another connection's work there).

        ``frames``: a frame table of ``rx`` to serve instead of scanning
        ``rx[:n]`` (``off``, ``length`` and a device ``count``:
        :meth:`serve_mixed` passes the serve's class of the batch); the
        reply frame starts then go to ``self.mix_rec_off[0]``."""
        L = _lib.lib()
        if self.fused_rows and (ordered or resume or self.seq_order or
                                self.tree.acl is not None or
                                frames is not None):
            raise ValueError('fused_rows: the serve must be the first '
                             'reader of the frame table (not ordered, no '
                             'seq_order, no ACL table, no watch resume)')
        if frames is not None:
            ft, tiles = frames, None
        else:
            ft = self.scanner.scan(rx, n, rows=not self.fused_rows)
            # (None for a request stream of one tile at most: the plain serve)
            tiles = self.scanner.pending
        # ordered serving ranks the batch from K12's request table; the
        # plain serve parses each frame in registers instead
        rt = B.decode_requests(rx, ft, out=self.rt) if ordered else None
        yield
        r = self.resp
        r.count = ft.count
        out = [r.opcode, r.xid, r.err, r.node, r.zxid, r.path_off,
               r.path_len, r.slot, self.presized[0], self.presized[1]]
        now = int(time.time() * 1000)
        seqno = self._seq_order(rx, ft) if self.seq_order else None
        if ordered:
            if self.ows is None:
                self.ows = torch.empty(
                    L.tree_order_workspace(self.cap_frames), dtype=U8,
                    device=self.tree.device)
            L.tree_serve_ordered(self.tree.tensors, rx, rt.tensors(),
                                 ft.count, self.cap_frames, out, session,
                                 now, self.ows, passes, self.tree.scratch,
                                 wslot, self.fired if self.tree.watch
                                 is not None else None, seqno)
        else:
            fired = self.fired if self.tree.watch is not None else None
            if tiles is not None:
                # the rows-deferred scan's consumer: it writes ft's rows
                L.tree_serve_tiles(self.tree.tensors, rx, tiles.n_dev,
                                   tiles.ncap, tiles.ws, ft.off, ft.length,
                                   ft.count, self.cap_frames, out, session,
                                   now, wslot, fired, seqno, self.read_only)
                tiles.consumed()
            else:
                L.tree_serve_frames(self.tree.tensors, rx, ft.off, ft.length,
                                    ft.count, self.cap_frames, out, session,
                                    now, wslot, fired, seqno, self.read_only)
            # the finish and K13's block-sum scan: one launch
            L.tree_finish_scan(self.tree.tensors, ft.count, 0, True,
                               self.cap_frames, self.presized[1],
                               self.total_err[0])
        if self.tree.acl is not None and not self.read_only:
            # the batch's successful CREATEs bind their ACLs
            _lib.tree_acl_record(self.tree.acl, rx, ft.off, ft.length,
                                 ft.count, self.cap_frames, r.opcode, r.err,
                                 r.node, self._acl_workspace())
        out, rec_off, total, err = B.encode_responses(
            r, self.tree.store, self.out.numel(), out=self.out,
            presized=self.presized, terminate=terminate,
            total_err=self.total_err, prescanned=not ordered,
            rec_off=self.mix_rec_off[0] if frames is not None else None)
        if self.tree.compact_free:
            self.tree.free_compact()
        self.last_rec_off = rec_off         # reply frame starts (R2 splits)
        self.result = (out, total, err, ft)
        if self.tree.watch is not None:
            self._notify()
            if resume:
                if wslot < 0:
                    raise ValueError('resume needs the watcher slot')
                self._resume(rx, ft, wslot)

    # -- session batches ------------------------------------------------------

    def _resume_sessions(self, rx, ft, seg_table, rec_off, total, err):
        """The SET_WATCHES catch-up of the session batch just served
        (csrc/kernels/tree_resume.hip; the rules: zk_resume.h): every
        SET_WATCHES frame of ``ft`` for its own segment's watcher slot,
        against the tree as the batch left it.  Leaves ``self.resume_notif``
        and ``self.resume_slots``; nothing is read back.  The buffers are
        allocated on first use and grown when a larger ``rx`` comes."""
        dev = self.tree.device
        sg = self.seg
        # a listed path takes at least the 4 bytes of its length in its
        # frame: no batch lists more paths than its bytes / 4, so the entry
        # and the event room (ecap of each) cannot overflow
        need = max(1, int(rx.numel()) // 4)
        b = self._caught
        if b is None or b.ecap < need:
            # as _resume sizes the buffer: 32 bytes of frame around a path,
            # and the paths are the request's own bytes (rx <= 4 ecap + 3)
            b = self._caught = _NotifStream(
                need, need * 32 + 4 * need + 4 + 64, rx, dev,
                _lib.watch_resume_sessions_workspace(self.cap_frames, need))
            self._rs_stats = torch.zeros(8, dtype=I64, device=dev)
        b.resp.path_arena = rx              # the encode arena: the requests
        _lib.watch_resume_sessions(
            self.tree.tensors, rx, ft.off, ft.length, ft.count,
            self.cap_frames, seg_table, b.ws, b.ev, b.ev_total, b.g, b.first,
            self._rs_stats)
        b.encode(self.tree.store)
        _lib.sess_ranges(sg.first, rec_off, ft.count, self.cap_frames, total,
                         err, sg.rep_off, *b.ranges())
        self.resume_notif, self.resume_slots = b.notif, b.slots

    def resume_stats(self):
        """Of the last session batch served with ``resume=True`` (one host
        read): ``events`` the catch-up found and ``events_written`` (fewer:
        the event room overflowed), watches ``rearmed``, paths ``listed`` by
        the frames that were caught up, ``dropped`` (listed paths past the
        entry room, neither answered nor re-armed), ``no_slot`` (paths of
        live SET_WATCHES frames whose segment's watcher slot is outside
        0..63) and ``encode_err`` (the catch-up encoder's flag; 2:
        the notification buffer is too small)."""
        if self._caught is None:
            raise ValueError('resume_stats: no session batch was resumed')
        v = torch.cat([self._rs_stats[:len(_lib.RESUME_STATS)],
                       self._caught.total_err[1].to(I64)]).cpu().tolist()
        st = dict(zip(_lib.RESUME_STATS, v))
        st['encode_err'] = v[-1]
        return st

    def resume_counters(self):
        """The device counters :meth:`resume_stats` reads (int64 [8], in
        ``_lib.RESUME_STATS`` order), for a caller that folds them into a
        read of its own (the front end's report); no host read."""
        if self._caught is None:
            raise ValueError('resume_counters: no session batch was resumed')
        return self._rs_stats

    def serve_sessions(self, rx, n, segs, ordered=False, passes=4,
                       terminate=False, table=None, resume=False,
                       close=False):
        """Serve ``rx[:n]``, the concatenated whole frames of the
        ``segs.S`` connections of :class:`SessionSegments` ``segs``, as ONE
        batch: one K1 scan and one serve (``passes`` of them when
        ``ordered``), each frame for its own segment's session and watcher
        slot (csrc/kernels/tree_sess.hip, the serve's MS instances).  ``n``
        is a host length or a device total; nothing is read back and the
        call is capturable where :meth:`serve` is.  Returns ``(out, total,
        err, frame table)`` like :meth:`serve`, and leaves

        ``self.seg``          ``.f_seg`` (segment per frame), ``.first``
                              (first frame per segment, [S + 1]),
                              ``.rep_off`` ([S + 1]: connection s's replies
                              are ``out[rep_off[s]:rep_off[s + 1]]``),
                              ``.state`` ([S]: 1 = session not alive) and
                              ``.bad`` ([2]);
        ``self.notif``        as :meth:`serve` does, but slot-major;
        ``self.notif_slots``  ``(slot_first, slot_off)``, both [65]: watcher
                              w's notifications are ``notif_buf[slot_off[w]:
                              slot_off[w + 1]]``, in request order.

        A frame that crosses a segment boundary, a ``starts`` that does not
        begin at 0 or descends: every request of the batch is answered
        SYSTEMERROR and nothing is touched (:meth:`session_stats`).
        ``table``: a :class:`GpuSessionTable`; a segment whose session (other
        than 0) it does not hold alive has its requests answered
        SESSION_EXPIRED, without effect.  (A SEQUENTIAL create refused this
        way leaves a gap in its parent's cversion, as any failed numbered
        create does.)

        The list ops and GET_ACL are not served here (UNIMPLEMENTED): a
        session batch that mixes them in goes through
        :meth:`serve_sessions_mixed` (``ordered`` there as here, for the
        serve's class).  How a connection's notification slices are
        interleaved with its reply slice on the socket is the front end's
        business.

        ``resume``: the SET_WATCHES catch-up (csrc/kernels/tree_resume.hip),
        on a tree with a watch table (``ValueError`` without one).  Off, a
        SET_WATCHES frame gets its header-only reply and nothing else.  On,
        the reply is the same and every SET_WATCHES frame of the batch is
        caught up for its own segment's watcher slot ``wslots[s]`` by the
        session rule of :meth:`serve`'s ``resume`` (a listed data watch:
        node gone NodeDeleted, mzxid > relZxid NodeDataChanged, else
        re-armed; an exist watch: node there NodeCreated, else re-armed; a
        child watch: node gone NodeDeleted, pzxid > relZxid
        NodeChildrenChanged, else re-armed), each frame with its own
        relZxid, any number of them anywhere in a segment.  The catch-up
        reads the tree as the batch leaves it: it is as if every SET_WATCHES
        frame of the batch came after all its other frames, in stream order
        among themselves — so a write by another connection of the batch to
        a listed path is an event of the catch-up when its zxid is past the
        frame's relZxid, and never fires the re-armed watch (as
        ``serve(resume=True)`` treats the writes of its own batch).  Nothing
        is caught up, re-armed or sent for a refused batch, a segment whose
        session is not alive, a frame of no segment, a segment whose
        ``wslots`` value is outside 0..63 (its paths are counted ``no_slot``)
        or a frame that is not a well-formed SET_WATCHES.  It leaves, with no
        host read,

        ``self.resume_notif``  ``(buf, total, slots, count)``: the catch-up's
                               xid -1 frames grouped by watcher slot, inside
                               a slot in stream order (frame order, then the
                               data, exist and child lists, then list
                               order); the paths are the request's own bytes.
                               Apart from ``self.notif``, which stays the
                               batch's write-fired events;
        ``self.resume_slots``  ``(slot_first, slot_off)``, both [65]: watcher
                               w's catch-up is ``buf[slot_off[w]:slot_off[w +
                               1]]``.  A front end writes that slice before
                               the slot's slice of ``self.notif``: what the
                               catch-up reports happened before the batch's
                               re-armed watches could fire;

        and :meth:`resume_stats` reads its counters.  Its buffers are sized
        from ``rx.numel()``, allocated on first use and grown when a larger
        ``rx`` comes; a call that does not grow them is capturable where the
        call without ``resume`` is.

        ``close``: serve the batch's CLOSE_SESSION frames
        (csrc/kernels/tree_close.hip; the rules: zk_close.h).  Off, such a
        frame is answered UNIMPLEMENTED and nothing else.  On, a
        CLOSE_SESSION frame of a live segment of a sound table is answered OK
        (the same 20 bytes, its own xid) and closes its segment: the
        segment's session and watcher slot join the list of one
        :meth:`close_sessions` pass that runs after the serve, and after the
        ``resume`` catch-up when both are set — as if every CLOSE_SESSION
        frame of the batch came after all its other frames, in segment order
        among themselves (the k-th closing segment's removals carry zxid
        base + k + 1, base the counter after the batch's own zxids).  So
        frames of a segment after its CLOSE_SESSION are served (the
        reference client sends it only when nothing is outstanding);
        ephemerals the closing connection creates in the same batch go with
        it, while another connection's read in that batch still sees them;
        the batch's write-fired notifications addressed to a closing watcher
        stay in ``self.notif``, but nothing of the close pass is addressed
        to one, and what the catch-up re-armed for it is dropped.  A refused
        frame closes nothing: an unsound table (SYSTEMERROR), a segment
        whose session is not alive (SESSION_EXPIRED), a body shorter than 8
        bytes (BAD_ARGUMENTS).  With ``table`` the closed sessions' entries
        die: their next batch is answered SESSION_EXPIRED.  It leaves
        ``self.close_notif`` / ``self.close_slots`` as
        :meth:`close_sessions` does (a front end writes a watcher's
        ``resume_notif`` slice, then its ``notif`` slice, then its
        ``close_notif`` slice), ``self.close_removed`` (int64 [S]: nodes
        removed for the k-th closing segment) and the counters of
        :meth:`close_stats`; nothing is read back."""
        if self.fused_rows or self.read_only:
            raise ValueError('serve_sessions: no session form of the '
                             'read-only or the fused-rows serve')
        if not isinstance(segs, SessionSegments):
            raise TypeError('serve_sessions: segs is a SessionSegments')
        tree = self.tree
        if resume and tree.watch is None:
            raise ValueError('serve_sessions: resume needs a watch table')
        if self.seg is None or self.seg.S != segs.S:
            self.seg = _SegState(self.cap_frames, segs.S, tree.device)
        sg = self.seg
        ft = self.scanner.scan(rx, n)
        _lib.sess_assign(ft.off, ft.length, ft.count, self.cap_frames,
                         segs.starts, segs.sessions, sg.f_seg, sg.first,
                         sg.state, sg.bad, **_table_args(table))
        out, rec_off, total, err = self._serve_class(
            rx, ft, sg.table(segs), segs, ordered, passes, None, close, None,
            terminate, None)
        self.last_rec_off = rec_off
        self.result = (out, total, err, ft)
        self._sessions_tail(rx, ft, segs, rec_off, total, err, table, resume,
                            close, None)
        return self.result

    def _serve_class(self, rx, frames, seg_table, segs, ordered, passes,
                     defer, close, rec_off, terminate, denied, auth=None):
        """The serve of one class of a session batch's frames through to its
        reply encode: ``frames`` with their segment table ``seg_table``
        (:meth:`_SegState.table` of ``segs``) — the whole batch
        (:meth:`serve_sessions`) or the serve's class
        (:meth:`serve_sessions_mixed`).  ``defer``: the deferral's tables for
        ``tree_serve_ordered_sessions`` or None; ``rec_off``: where the
        encode leaves the frame starts (None: its own); ``denied``: the
        whole batch's frame count when the ACL check ran over it (its
        fix-up goes between the serve and the encode) or None; ``auth``: the
        :class:`AuthTable` when the batch's AUTH frames were served (their
        fix-up follows the ACL check's) or None.  Returns what
        ``encode_responses`` returns."""
        L = _lib.lib()
        tree = self.tree
        cap = self.cap_frames
        r = self.resp
        r.count = frames.count
        out = [r.opcode, r.xid, r.err, r.node, r.zxid, r.path_off,
               r.path_len, r.slot, self.presized[0], self.presized[1]]
        now = int(time.time() * 1000)
        seqno = self._seq_order(rx, frames) if self.seq_order else None
        fired = self.fired if tree.watch is not None else None
        if ordered:
            rt = B.decode_requests(rx, frames, out=self.rt)
            if self.ows is None:
                self.ows = torch.empty(L.tree_order_workspace(cap), dtype=U8,
                                       device=tree.device)
            _lib.tree_serve_ordered_sessions(
                tree.tensors, rx, rt.tensors(), frames.count, cap, out, now,
                self.ows, passes, tree.scratch, fired, seqno, seg_table,
                defer)
        else:
            _lib.tree_serve_frames_sessions(
                tree.tensors, rx, frames.off, frames.length, frames.count,
                cap, out, now, fired, seqno, seg_table)
            L.tree_finish_scan(tree.tensors, frames.count, 0, True, cap,
                               self.presized[1], self.total_err[0])
        if tree.acl is not None:
            _lib.tree_acl_record(tree.acl, rx, frames.off, frames.length,
                                 frames.count, cap, r.opcode, r.err, r.node,
                                 self._acl_workspace())
        if close:
            self._close_frames(rx, frames, seg_table, segs.S)
        if denied is not None:
            _lib.aclperm_fix(self.acl_deny, self.mix_cls, self.mix_sub,
                             denied, cap, r.err, self.acl_enf)
        if auth is not None:
            _lib.auth_fix(self.auth_res, self.mix_cls, self.mix_sub, denied,
                          cap, r.err, auth.stats)
        enc = B.encode_responses(
            r, tree.store, self.out.numel(), out=self.out,
            presized=self.presized, terminate=terminate,
            total_err=self.total_err, prescanned=not ordered,
            rec_off=rec_off)
        if tree.compact_free:
            tree.free_compact()
        return enc

    def _sessions_tail(self, rx, ft, segs, rec_off, total, err, table,
                       resume, close, defer):
        """What follows a session batch's replies (``rec_off`` / ``total`` /
        ``err``: the whole batch's reply stream over frame table ``ft``): the
        write-fired events, the reply and notification ranges, the
        SET_WATCHES catch-up, the deferral's ranges (``defer``: the
        :class:`OrderDefer` or None) and the close pass."""
        sg, cap = self.seg, self.cap_frames
        if self.tree.watch is not None:
            self._notify(grouped=True)
            _lib.sess_ranges(sg.first, rec_off, ft.count, cap, total, err,
                             sg.rep_off, *self._fired.ranges())
            if resume:
                self._resume_sessions(rx, ft, sg.table(segs), rec_off, total,
                                      err)
        else:
            _lib.sess_ranges(sg.first, rec_off, ft.count, cap, total, err,
                             sg.rep_off)
        if defer is not None:
            _lib.order_clip_ranges(defer.clipf, sg.rep_off, rec_off, ft.off,
                                   segs.starts, ft.count, cap, defer.rep_end,
                                   defer.used)
        if close:
            self._close_batch(segs, table)

    def session_stats(self):
        """Of the last :meth:`serve_sessions` or
        :meth:`serve_sessions_mixed` (one host read): ``bad`` (torn
        frames + faults of the segment table; not 0: the batch was refused),
        ``first_bad_segment`` (-1: none) and ``expired_segments`` (segments
        whose session the table did not hold alive)."""
        if self.seg is None:
            raise ValueError('session_stats: no session batch was served')
        sg = self.seg
        v = torch.cat([sg.bad, (sg.state == 1).sum().view(1)]).cpu().tolist()
        return {'bad': v[0], 'first_bad_segment': v[1],
                'expired_segments': v[2]}

    # -- closing many sessions ------------------------------------------------

    def _close_buffers(self, S):
        """The close passes' buffers for lists of up to ``S`` sessions
        (csrc/kernels/tree_close.hip), allocated on first use and grown when
        a longer list comes; on a tree with a watch table also those of the
        events the removals fire, apart from the batch's own (``self.notif``
        keeps what the batch's writes fired)."""
        tree, cap = self.tree, self.cap_frames
        dev = tree.device
        need = _lib.close_workspace(cap, S, tree.cap)
        c = self._cl
        if c is None:
            c = self._cl = SimpleNamespace(
                ws=None, removed=None, st=None,
                stats=torch.zeros(8, dtype=I64, device=dev))
            if tree.watch is not None:
                c.st = _NotifStream(self.ecap, self.notif_buf.numel(),
                                    tree.path_arena, dev,
                                    _lib.sess_group_workspace(self.ecap))
                # every record is a removal: a DELETE that succeeded
                c.op = torch.full((cap,), consts.OP_CODES['DELETE'],
                                  dtype=I32, device=dev)
                c.err = torch.zeros(cap, dtype=I32, device=dev)
                # sess_ranges' reply half: one segment without a frame
                c.nil = (torch.zeros(2, dtype=I64, device=dev),
                         torch.zeros(1, dtype=I64, device=dev),
                         torch.zeros(1, dtype=I32, device=dev),
                         torch.zeros(2, dtype=I64, device=dev))
        if c.ws is None or c.ws.numel() < need:
            c.ws = torch.empty(need, dtype=I64, device=dev)
        if c.removed is None or c.removed.numel() < S:
            c.removed = torch.zeros(S, dtype=I64, device=dev)
        return c

    def _close_frames(self, rx, frames, seg_table, S):
        """Pass 1 of a session batch served with ``close``: between the serve
        of ``frames`` and the encode of its replies."""
        c = self._close_buffers(S)
        _lib.close_frames(self.tree.tensors, rx, frames.off, frames.length,
                          frames.count, self.cap_frames, seg_table,
                          self.resp.err, self.cap_frames, c.ws, c.stats)

    def _close_batch(self, segs, table):
        """Passes 2-7 of a session batch served with ``close``, over the list
        :meth:`_close_frames` left on the device."""
        c = self._close_buffers(segs.S)
        self.close_removed = c.removed[:segs.S]
        self.close_removed.zero_()
        self._close_pass(segs.S, None, None, table, self.close_removed)

    def _close_pass(self, S, sids, wslots, table, removed):
        """Passes 2-7 and, on a tree with a watch table, the events: the
        records of the removals' fired watches expanded, grouped by watcher
        slot and encoded, as :meth:`_notify` does a session batch's."""
        tree, cap = self.tree, self.cap_frames
        c = self._close_buffers(S)
        _lib.close_sessions(
            tree.tensors, sids, wslots, S, cap, c.ws, removed, c.stats,
            **_table_args(table))
        if tree.watch is None:
            return
        rec = c.ws[:8 + 5 * cap]
        c.st.events(c.op, c.err, rec[0:1], cap, rec[8:], self.wbsum)
        c.st.group()
        c.st.encode(tree.store)
        nil = c.nil
        _lib.sess_ranges(nil[0], nil[1], nil[1], 1, nil[1], nil[2], nil[3],
                         *c.st.ranges())
        self.close_notif, self.close_slots = c.st.notif, c.st.slots

    def close_sessions(self, sids, wslots=None, table=None, removed=None):
        """End the sessions ``sids`` (device int64 [K]) in ONE pass
        (csrc/kernels/tree_close.hip; the rules: zk_close.h): the sessions a
        front end's timer expired, or that it closes for reasons of its own.
        What K calls of :meth:`expire` (and one of
        :meth:`GpuSessionTable.close`) do with K sweeps of the node table
        and of the watch table, in one sweep of each; no host read.

        Session ``sids[k]``'s ephemerals are removed as its own closeSession
        txn, zxid base + k + 1, and the zxid counter moves by K: the tree is
        the one ``expire(sids[0]) ... expire(sids[K - 1])`` leaves.  An id
        listed twice removes at its first position, id 0 and an id that owns
        nothing remove nothing; each still takes its zxid.  Returns
        ``removed`` (device int64 [K], accumulated): the nodes removed for
        each listed session.

        ``wslots`` (device int32 [K]): the sessions' watcher slots.  On a
        tree with a watch table their bits are dropped from every mask
        before anything is removed (a value outside 0..63 drops nothing), so
        a closing session is told nothing and the next session bound to its
        slot inherits nothing; the watches the removals fire for the others
        are left in

        ``self.close_notif``  ``(buf, total, slots, count)``: the xid -1
                              frames grouped by watcher slot, in no defined
                              order inside a slot (as :meth:`expire`'s);
        ``self.close_slots``  ``(slot_first, slot_off)``, both [65]: watcher
                              w's are ``buf[slot_off[w]:slot_off[w + 1]]``.

        Room for ``cap_frames`` removals that fire a watch; more are counted
        by :meth:`close_stats` and their events lost.  ``table``: a
        :class:`GpuSessionTable`; the listed ids' entries close (an id it
        does not hold touches nothing)."""
        K = int(sids.numel())
        dev = self.tree.device
        if removed is None:
            removed = torch.zeros(K, dtype=I64, device=dev)
        if K == 0:
            return removed
        self._close_pass(K, sids, wslots, table, removed)
        return removed

    def close_stats(self):
        """Of the last close pass (:meth:`close_sessions`, or a session batch
        served with ``close=True``), one host read: ``frames`` (closing
        CLOSE_SESSION frames; 0 for the direct form), ``sessions`` (K),
        ``removed`` (nodes, all sessions), ``events_fired`` /
        ``events_written`` (fewer written: the event room overflowed),
        ``records_dropped`` (removals whose fired watches found no record:
        past ``cap_frames``) and ``encode_err`` (the events' encoder's flag;
        2: the notification buffer is too small)."""
        c = self._cl
        if c is None:
            raise ValueError('close_stats: no close pass has run')
        parts = [c.stats[:3]]
        if c.st is not None:
            parts += [c.st.ev_total, c.ws[0:1], c.st.total_err[1].to(I64)]
        v = torch.cat(parts).cpu().tolist() + [0, 0, 0, 0]
        return dict(zip(_lib.CLOSE_STATS,
                        [v[0], v[1], v[2], v[4], v[3],
                         max(0, v[5] - self.cap_frames), v[6]]))

    def serve_list(self, rx, n, wslot=-1, terminate=False, max_frame=None,
                   out=None):
        """Serve a batch of list requests — GET_CHILDREN / GET_CHILDREN2
        frames only, ``rx[:n]`` (``n`` a host length or a device total) —
        from the tree (csrc/kernels/tree_list.hip: two sweeps of the node
        table per batch, no child links).  Returns ``(out, total, err,
        frame_table)`` like :meth:`serve`; the replies are in request order.

        Any other op in the batch is answered UNIMPLEMENTED, a truncated
        frame BAD_ARGUMENTS, a missing path NO_NODE — ``/`` included, which
        has no node in this tree (every op on it is NO_NODE).  The order of
        the names inside a reply is unspecified, as ZooKeeper's is.  A
        request with ``watch`` set that finds its node arms the child watch
        of watcher slot ``wslot`` (0..63; needs a tree with a watch table);
        a NO_NODE arms nothing.  A reply frame longer than ``max_frame``
        bytes (default: K1's 16 MiB cap) is answered SYSTEMERROR.  ``err``
        2 with ``total`` 0: the replies did not fit ``out`` (default: the
        server's reply buffer) and nothing was written.  Mixed batches go
        through :meth:`serve_mixed`.

        A sharded tree (``shard`` with world > 1) raises: its parents count
        children it does not index."""
        tree = self.tree
        if tree.shard is not None and tree.shard[1] > 1:
            raise ValueError('serve_list: a sharded tree does not index '
                             'every child of its parents')
        self._list_buffers()
        if out is None:
            out = self.out
        if max_frame is None:
            max_frame = consts.MAX_PACKET
        ft = self.scanner.scan(rx, n)
        total, err = self.list_total_err
        _lib.tree_list(tree.tensors, rx, ft.off, ft.length, ft.count,
                       self.cap_frames, wslot, max_frame, self.list_want,
                       self.list_ws, out, out.numel(), self.list_rec_off,
                       total, err, terminate)
        self.last_rec_off = self.list_rec_off
        self.result = (out, total, err, ft)
        return self.result

    def _list_buffers(self):
        """The list engine's buffers, allocated on first use."""
        if self.list_want is not None:
            return
        dev = self.tree.device
        self.list_want = torch.full((self.tree.cap,), _lib.LIST_IDLE,
                                    dtype=I32, device=dev)
        self.list_ws = torch.empty(
            _lib.tree_list_workspace(self.cap_frames), dtype=U8, device=dev)
        self.list_rec_off = torch.empty(self.cap_frames, dtype=I64,
                                        device=dev)
        self.list_total_err = B._total_err(dev)

    def _acl_buffers(self):
        """The GET_ACL engine's buffers, allocated on first use."""
        if self.acl_rec_off is not None:
            return
        dev = self.tree.device
        self.acl_rec_off = torch.empty(self.cap_frames, dtype=I64,
                                       device=dev)
        self.acl_total_err = B._total_err(dev)

    def _acl_workspace(self):
        # (no attribute until then: a server that recorded no ACL has none)
        if getattr(self, 'acl_ws', None) is None:
            self.acl_ws = torch.empty(
                _lib.tree_acl_workspace(self.cap_frames), dtype=U8,
                device=self.tree.device)
        return self.acl_ws

    def serve_acl(self, rx, n, terminate=False, out=None):
        """Serve a batch of GET_ACL frames, ``rx[:n]`` (``n`` a host length
        or a device total), from the tree and its ACL table
        (csrc/kernels/tree_acl.hip).  Returns ``(out, total, err,
        frame_table)`` like :meth:`serve`; the replies are in request order:
        the node's ACL as its CREATE sent it (the open ACL for the static
        nodes), then its Stat.

        Any other op in the batch is answered UNIMPLEMENTED, a truncated
        frame BAD_ARGUMENTS, a missing path NO_NODE (``/`` included: it has
        no node in this tree), and a node whose ACL found no room in the
        table SYSTEMERROR (see :meth:`acl_stats`); all header only.  ``err``
        2 with ``total`` 0: the replies did not fit ``out`` (default: the
        server's reply buffer) and nothing was written.  Mixed batches go
        through :meth:`serve_mixed`.

        Raises ``ValueError`` on a tree without an ACL table."""
        tree = self.tree
        if tree.acl is None:
            raise ValueError('serve_acl: the tree keeps no ACL table '
                             '(GpuTree(acl_cap=...))')
        self._acl_buffers()
        if out is None:
            out = self.out
        ft = self.scanner.scan(rx, n)
        total, err = self.acl_total_err
        _lib.tree_acl_get(tree.tensors, tree.acl, rx, ft.off, ft.length,
                          ft.count, self.cap_frames, self._acl_workspace(),
                          out, out.numel(), self.acl_rec_off, total, err,
                          terminate)
        self.last_rec_off = self.acl_rec_off
        self.result = (out, total, err, ft)
        return self.result

    def _mix_buffers(self):
        """The split's and the merge's buffers and the two engines' scratch
        streams, allocated on first use."""
        if self.mix_cls is not None:
            return
        dev = self.tree.device
        cap = self.cap_frames
        self.mix_cls = torch.empty(cap, dtype=I32, device=dev)
        self.mix_sub = torch.empty(cap, dtype=I32, device=dev)
        self.mix_foff = torch.empty(3 * cap, dtype=I64, device=dev)
        self.mix_flen = torch.empty(3 * cap, dtype=I32, device=dev)
        self.mix_counts = torch.zeros(3, dtype=I64, device=dev)
        self.mix_frames = [
            _SubFrames(self.mix_foff[c * cap:(c + 1) * cap],
                       self.mix_flen[c * cap:(c + 1) * cap],
                       self.mix_counts[c:c + 1]) for c in range(3)]
        self.mix_split_ws = torch.empty(
            max(_lib.tree_mix_split_workspace(cap), 16), dtype=U8, device=dev)
        self.mix_merge_ws = torch.empty(
            max(_lib.tree_mix_merge_workspace(cap), 16), dtype=U8, device=dev)
        self._list_buffers()
        self._acl_buffers()
        # the serve's frame starts, then the merged ones
        self.mix_rec_off = (torch.empty(cap, dtype=I64, device=dev),
                            torch.empty(cap, dtype=I64, device=dev))
        self.mix_total_err = B._total_err(dev)
        # (a tree without an ACL table: the GET_ACL class stays empty)
        self.acl_total_err[0].zero_()
        self.acl_total_err[1].zero_()
        self.mix_scratch = (
            torch.empty(self.out.numel(), dtype=U8, device=dev)
            if self.tree.acl is not None else None,
            torch.empty(self.out.numel(), dtype=U8, device=dev))
        self.mix_out = torch.empty(self.out.numel(), dtype=U8, device=dev)

    def serve_mixed(self, rx, n, session=0, terminate=False, wslot=-1,
                    resume=False, max_frame=None, out=None):
        """Serve the request stream ``rx[:n]`` (``n`` a host length or a
        device total) whatever ops it mixes — what a session pipelines on one
        connection, what ``Client.bulk`` encodes — into one reply stream in
        request order.  Returns ``(out, total, err, frame_table)`` like
        :meth:`serve`, with the whole batch's frame table; ``out`` defaults
        to a buffer of the server's reply capacity (``self.mix_out``, not
        ``self.out``: the serve's own stream lands there).

        One K1 scan, then the split of the frame table by engine
        (csrc/kernels/tree_mix.hip): GET_CHILDREN / GET_CHILDREN2 to the
        list engine, GET_ACL to the ACL engine (on a tree with an ACL table),
        everything else — unknown opcodes, frames without an opcode word and
        GET_ACL on a tree without an ACL table included — to the fused serve,
        each answering as :meth:`serve_list`, :meth:`serve_acl` and
        :meth:`serve` (unordered) do.  The merge puts the three reply
        streams back into request order; ``self.last_rec_off`` holds the
        merged frame starts.

        The batch contract: the engines run in the fixed order serve,
        GET_ACL, list, each over its requests in request order.  So the
        writes of a batch are concurrent as in :meth:`serve` (``session``,
        ``wslot`` and ``resume`` as there; ``self.notif`` is what the
        batch's writes fired), and a GET_ACL or a list of a batch sees the
        tree after all of that batch's writes: a list of a parent shows the
        child created in the same batch and misses the one deleted in it, a
        GET_ACL returns the ACL of a node created in the same batch.  A
        ``watch=1`` list arms the child watch of slot ``wslot`` after the
        batch's writes: they do not fire it, the next batch's do.  In-batch
        ordering (``serve(ordered=True)``) is not offered.

        ``max_frame``: as in :meth:`serve_list`.  ``err`` is the first
        non-zero one of the serve's, the ACL engine's and the list engine's
        encoders (each stream has the server's reply capacity), else 2 when
        the merged stream does not fit ``out``; then ``total`` is 0 and
        ``out`` is untouched.

        A class without a member still costs its engine's launches: nothing
        is read back that could skip them.  After the first call has
        allocated the buffers a call without ``resume`` reads nothing back
        and allocates nothing; it can be captured in a HIP graph on one
        stream.

        Raises ``ValueError`` on a ``fused_rows`` server (the split must be
        the frame table's first reader) and on a sharded tree (``shard``
        with world > 1), as :meth:`serve_list` does."""
        tree = self.tree
        if self.fused_rows:
            raise ValueError('serve_mixed: a fused_rows server defers the '
                             'frame table\'s rows to the serve; the split '
                             'must be their first reader')
        if tree.shard is not None and tree.shard[1] > 1:
            raise ValueError('serve_mixed: a sharded tree does not index '
                             'every child of its parents')
        self._mix_buffers()
        cap = self.cap_frames
        if out is None:
            out = self.mix_out
        if max_frame is None:
            max_frame = consts.MAX_PACKET
        ft = self.scanner.scan(rx, n)
        _lib.tree_mix_split(rx, ft.off, ft.length, ft.count, cap,
                            tree.acl is not None, self.mix_cls, self.mix_sub,
                            self.mix_foff, self.mix_flen, self.mix_counts,
                            self.mix_split_ws)
        fa, fc, fl = self.mix_frames
        for _ in self.serve_steps(rx, n, session, False, False, 4, wslot,
                                  resume, frames=fa):
            pass
        a_out, a_total, a_err, _ = self.result
        c_out, l_out = self.mix_scratch
        c_total, c_err = self.acl_total_err
        if tree.acl is not None:
            _lib.tree_acl_get(tree.tensors, tree.acl, rx, fc.off, fc.length,
                              fc.count, cap, self._acl_workspace(), c_out,
                              c_out.numel(), self.acl_rec_off, c_total,
                              c_err, False)
        else:
            c_out = l_out
        l_total, l_err = self.list_total_err
        _lib.tree_list(tree.tensors, rx, fl.off, fl.length, fl.count, cap,
                       wslot, max_frame, self.list_want, self.list_ws, l_out,
                       l_out.numel(), self.list_rec_off, l_total, l_err,
                       False)
        total, err = self.mix_total_err
        _lib.tree_mix_merge(
            self.mix_cls, self.mix_sub, ft.count, self.mix_counts, cap,
            [a_out, c_out, l_out],
            [self.mix_rec_off[0], self.acl_rec_off, self.list_rec_off],
            [a_total, c_total, l_total], [a_err, c_err, l_err], out,
            out.numel(), self.mix_rec_off[1], total, err, self.mix_merge_ws,
            terminate)
        self.last_rec_off = self.mix_rec_off[1]
        self.result = (out, total, err, ft)
        return self.result

    def serve_sessions_mixed(self, rx, n, segs, terminate=False, table=None,
                             max_frame=None, out=None, resume=False,
                             close=False, ordered=False, passes=4,
                             defer=None, perms=None, setacl=False,
                             setacl_passes=4):
        """Serve ``rx[:n]``, the concatenated whole frames of the ``segs.S``
        connections of :class:`SessionSegments` ``segs``, whatever ops they
        mix, as ONE batch: :meth:`serve_sessions` for every op of
        :meth:`serve_mixed`.  ``rx``, ``n``, ``segs`` and ``table`` as in
        :meth:`serve_sessions`; ``max_frame`` and ``out`` (default
        ``self.mix_out``) as in :meth:`serve_mixed`.  Returns ``(out, total,
        err, frame table)`` with the whole batch's frame table, and leaves
        ``self.seg`` (``f_seg``, ``first``, ``rep_off``, ``state``, ``bad``),
        ``self.notif``, ``self.notif_slots`` and ``self.last_rec_off`` (the
        merged frame starts) as those two do.  Nothing is read back, nothing
        is allocated after the first call (of a segment count), and the call
        can be captured on one stream where :meth:`serve_mixed` can.

        The batch contract.  One K1 scan and one segment assign over the
        whole frame table; the split of :meth:`serve_mixed`, the frames'
        segments carried through it (csrc/kernels/tree_sess.hip
        sess_split_seg_k); the engines in :meth:`serve_mixed`'s fixed order —
        serve (unordered), GET_ACL, list — each over its class's frames in
        request order, each frame for its own segment's session and watcher
        slot.  So a list or a GET_ACL from any connection sees the tree
        after all writes of the batch, from every connection.  A ``watch=1``
        list arms the child watch of its own segment's ``wslots[s]``, after
        the batch's writes (they do not fire it); a value outside 0..63 arms
        nothing.  ``self.seg.rep_off[s]`` slices the merged stream:
        connection s's replies are ``out[rep_off[s]:rep_off[s + 1]]``;
        ``notif_buf[slot_off[w]:slot_off[w + 1]]`` is watcher w's
        notifications, in request order.

        Refusals.  An unsound table (``bad != 0``: a torn frame, a
        ``starts`` that does not begin at 0 or descends) answers every
        request of the batch SYSTEMERROR, list and GET_ACL frames included;
        a segment whose session ``table`` does not hold alive has all its
        requests answered SESSION_EXPIRED.  For the list and ACL engines
        both are header-only replies with the xid the engine parsed: a
        refused frame looks nothing up, claims no parent and arms nothing.
        Refusal takes precedence over BAD_ARGUMENTS and UNIMPLEMENTED, as in
        the serve.

        ``err`` and overflow follow :meth:`serve_mixed`'s rule: the first
        non-zero one of the three engines' encoders, else 2 when the merged
        stream does not fit ``out``; then ``total`` is 0, ``out`` is
        untouched and ``rep_off`` is all zero.  On a tree without an ACL
        table GET_ACL goes to the serve (UNIMPLEMENTED), as in
        :meth:`serve_mixed`.

        ``resume``: the SET_WATCHES catch-up, as in :meth:`serve_sessions`
        (``self.resume_notif``, ``self.resume_slots``, :meth:`resume_stats`;
        ``ValueError`` on a tree without a watch table).  It runs once over
        the whole frame table and its segments, after the three engines: the
        tree it reads is the one the whole batch leaves, a listed path that
        any connection of the batch wrote is an event of the catch-up and
        never hits the re-armed watch, and a ``watch=1`` list of the batch is
        armed before it.  Off, a SET_WATCHES frame gets its header-only
        reply and nothing else; on, the replies are the same.

        ``close``: the batch's CLOSE_SESSION frames are served, as in
        :meth:`serve_sessions` (``self.close_notif``, ``self.close_slots``,
        ``self.close_removed``, :meth:`close_stats`).  The frame is of the
        serve's class; the close pass runs once, after the three engines and
        after the ``resume`` catch-up, so a list or a GET_ACL of the batch
        still sees a closing connection's ephemerals.

        ``ordered``: the serve's class goes through the ordered session serve
        (``serve_sessions(ordered=True)``: K12's request table over the
        class's frames, the ranking, ``passes`` serve launches), so requests
        of the serve's class that conflict (zk_tree_serve_ordered's rule: the
        same path with a writer among them, a create / delete and its
        parent's path) are applied as a serial execution in batch order
        would, whichever segments they come from; a read that a later write
        of the batch overtakes is answered from a snapshot (a tree with a
        scratch tail).  GET_ACL and the list ops still run after the serve,
        over the tree as all the batch's writes leave it, and the catch-up
        and the close pass keep their place: in-batch order covers the
        serve's class only.  :meth:`order_stats` works after the call.  A
        request whose rank is >= ``passes`` is answered SYSTEMERROR, without
        effect, as in :meth:`serve_sessions`.

        ``defer`` (an :class:`OrderDefer` of ``segs.S`` segments; only with
        ``ordered``): deferral instead of that refusal.  The frame whose rank
        the passes cannot reach and every later frame of its segment, of any
        class, leave the batch before the first pass: they are frames of no
        segment, so nothing of them is parsed, looked up, claimed, armed,
        fired, closed or caught up, and their SYSTEMERROR placeholders lie
        behind ``defer.rep_end[s]`` in the segment's slice.  The caller
        sends ``out[rep_off[s]:rep_end[s]]`` and serves the segment's bytes
        from ``defer.used[s]`` on again in a later batch.  The frames that
        stay are served as if the deferred ones had not been sent.  (A
        deferred SEQUENTIAL create has taken its number, which stays out of
        use: a gap in the parent's cversion, as every refused numbered create
        leaves — the serve's instance for these passes does not hand a
        deferred frame's number back as a batch refused as a whole does, so
        the name it gets in a later batch is past every name of this one.  A
        batch whose table is unsound is refused as a whole and defers
        nothing.)

        ``perms`` (an :class:`AclIdentity` of ``segs.S`` peers): the ACLs the
        tree keeps are enforced (csrc/kernels/tree_aclperm.hip; the rule:
        zk_aclperm.h).  None: every launch and every byte of the call are
        what they are without the argument.  With it one launch after the
        segment assign checks every frame whose segment is served, whose
        body parses and whose target exists: GET_DATA and the list ops need
        READ and SET_DATA WRITE on the node, CREATE needs CREATE on the
        parent, DELETE needs DELETE on the parent and only when the node
        itself exists; every other op needs nothing.  An entry grants when
        it carries the bit and is ``world:anyone`` or an ``ip`` entry
        (``a.b.c.d`` or ``a.b.c.d/bits``) that covers the segment's
        address; every other scheme matches nobody.  The open ACL grants
        without a read of the store; a node whose ACL found no room in it
        (:meth:`acl_stats`) denies every op that needs a permission.  A
        denied frame is answered NO_AUTH, header only, with its xid, and is
        otherwise no request of the batch: it is looked up, claimed, armed,
        fired, numbered (a denied SEQUENTIAL create takes no number), ranked
        and deferred by nothing, under the unordered serve, ``ordered`` and
        ``defer`` alike; a second launch, between the serve and its reply
        encode, writes the code.  :meth:`acl_enforce_stats` reads the
        counters.  Three points of the batch contract:

        * permission and existence are those of the tree as the batch finds
          it.  A node created in the batch is not protected before the next
          batch — the moment its ACL is bound —, and a node deleted in it
          still decides;
        * NO_AUTH comes before NODE_EXISTS, BAD_VERSION and NOT_EMPTY and
          after NO_NODE, as in ZooKeeper;
        * the opcode words of the denied frames in the caller's ``rx`` are
          overwritten (with an opcode of no request).

        Raises ``ValueError`` on a tree without an ACL table and when
        ``perms.addrs`` is not ``[segs.S]``.

        ``perms.auth`` (an :class:`AuthTable`; None: every launch and every
        byte are what they are with ``perms`` alone): the batch's AUTH
        frames (opcode 100) are served (csrc/kernels/tree_auth.hip; the
        rule: zk_auth.h).  One more launch after the segment assign takes
        every AUTH frame of a served segment: the scheme ``digest`` with
        credentials of at most 119 bytes stores the identity
        ``user:base64(SHA1(credentials))`` in the segment's row — unless
        the row holds it from an earlier batch — and is answered OK; a
        malformed frame, any other scheme, longer credentials and a fifth
        identity of a row are answered AUTH_FAILED (-115).  Both replies
        are header only, with the frame's own xid; a third launch, behind
        the ACL check's fix-up, writes the code.  The ACL check then lets a
        ``digest`` entry grant to a connection that holds its id; ``auth``,
        ``sasl`` and every other scheme still match nobody.  An identity
        holds for every frame of its connection in the batch that carries
        its AUTH frame, the frames ahead of it included.  Two equal AUTH
        frames of one connection in one batch may take two of its four
        slots.  A refused segment's AUTH frame stores nothing and keeps its
        refusal; a deferred one comes back, finds its identity stored and
        is answered OK then.  :meth:`auth_stats` reads the counters.

        ``setacl`` (off: the call launches what it launches without the
        argument): the batch's SET_ACL frames (opcode 7) are served
        (csrc/kernels/tree_setacl.hip; the rule: zk_setacl.h).  The split
        sends them to the ACL engine's class, and a pass over that class's
        frame table runs before its GET_ACL frames are sized — after the
        batch's serve-class writes and after the batch's creates have had
        their ACLs bound.  A frame is answered, in this order, BAD_ARGUMENTS
        (a body that is no whole SET_ACL request), INVALID_ACL (an empty
        vector, or one of 16 MiB or more), NO_NODE, NO_AUTH (with ``perms``:
        the node's ACL does not grant ADMIN to the segment's address and,
        with ``perms.auth``, its identities; without ``perms`` nothing is
        checked, as nothing else is), BAD_VERSION (``version`` is neither -1
        nor the node's ``aversion``), or OK with the node's Stat, whose
        ``aversion`` is the one this frame produced: a frame of 4 + 84
        bytes; every failure is header only.  The batch contract:

        * ADMIN is judged on the ACL as the pass finds it: a SET_ACL of the
          batch does not take the permission from a later one of it;
        * on one node the batch's SET_ACLs run in frame order, whichever
          segments they come from, one a round, ``setacl_passes`` rounds: a
          frame its node's rounds do not reach is answered SYSTEMERROR
          without effect (the convention of ``ordered`` and ``passes``);
          different nodes proceed in parallel;
        * the batch's serve-class requests were all judged (``perms``) and
          served before any SET_ACL of it took effect, and every GET_ACL of
          the batch sees the ACLs all its SET_ACLs leave;
        * every frame that reached its version check takes a zxid, failed
          ones included, unique and increasing in frame order, above those
          of the batch's serve-class writes.

        Only a frame past every check but the version has its vector
        interned, so a client without ADMIN cannot fill the store; the
        vector of a frame that then fails BAD_VERSION stays interned
        (nothing in the store is reclaimed).  A vector the store has no room
        for fails its frame with SYSTEMERROR and leaves the node's ACL as it
        is.  No scheme or id is validated, equal entries are not removed and
        an ``auth`` entry is stored as sent (it matches nobody), as for
        CREATE.  A refused or deferred segment's SET_ACL frame does nothing
        and keeps its placeholder.  :meth:`setacl_stats` reads the counters.
        Raises ``ValueError`` on a tree without an ACL table.

        Raises ``ValueError`` on a ``fused_rows`` or ``read_only`` server
        and on a sharded tree, as the two entry points do."""
        tree = self.tree
        if setacl and tree.acl is None:
            raise ValueError('serve_sessions_mixed: setacl needs a tree '
                             'with an ACL table (GpuTree(acl_cap=...))')
        if self.fused_rows or self.read_only:
            raise ValueError('serve_sessions_mixed: no session form of the '
                             'read-only or the fused-rows serve')
        if tree.shard is not None and tree.shard[1] > 1:
            raise ValueError('serve_sessions_mixed: a sharded tree does not '
                             'index every child of its parents')
        if not isinstance(segs, SessionSegments):
            raise TypeError('serve_sessions_mixed: segs is a SessionSegments')
        if resume and tree.watch is None:
            raise ValueError('serve_sessions_mixed: resume needs a watch '
                             'table')
        if defer is not None:
            if not ordered:
                raise ValueError('serve_sessions_mixed: defer needs ordered')
            if not isinstance(defer, OrderDefer) or defer.S != segs.S:
                raise ValueError('serve_sessions_mixed: defer is an '
                                 'OrderDefer of segs.S segments')
        if perms is not None:
            if tree.acl is None:
                raise ValueError('serve_sessions_mixed: perms needs a tree '
                                 'with an ACL table (GpuTree(acl_cap=...))')
            if not isinstance(perms, AclIdentity) or perms.S != segs.S:
                raise ValueError('serve_sessions_mixed: perms is an '
                                 'AclIdentity of segs.S addresses')
        self._mix_buffers()
        cap = self.cap_frames
        if self.seg is None or self.seg.S != segs.S:
            self.seg = _SegState(cap, segs.S, tree.device)
        sg = self.seg
        seg_c = sg.class_tables()
        if out is None:
            out = self.mix_out
        if max_frame is None:
            max_frame = consts.MAX_PACKET
        ft = self.scanner.scan(rx, n)
        _lib.sess_assign(ft.off, ft.length, ft.count, cap, segs.starts,
                         segs.sessions, sg.f_seg, sg.first, sg.state, sg.bad,
                         **_table_args(table))
        if perms is not None:
            # (before the split: a denied frame is of the serve's class)
            self._acl_enforce_buffers()
            auth = perms.auth
            if auth is None:
                _lib.aclperm_check(tree.tensors, tree.acl, rx, ft.off,
                                   ft.length, ft.count, cap, sg.table(segs),
                                   perms.addrs, self.acl_deny, self.acl_enf)
            else:
                if self.auth_res is None:
                    self.auth_res = torch.zeros(cap, dtype=I32,
                                                device=tree.device)
                self.auth_table = auth
                _lib.auth_frames(rx, ft.off, ft.length, ft.count, cap,
                                 sg.table(segs), auth.tensors, self.auth_res)
                _lib.aclperm_check_auth(
                    tree.tensors, tree.acl, rx, ft.off, ft.length, ft.count,
                    cap, sg.table(segs), perms.addrs, auth.tensors,
                    self.acl_deny, self.acl_enf)
        split = _lib.tree_mix_split_setacl if setacl else _lib.tree_mix_split
        split(rx, ft.off, ft.length, ft.count, cap, tree.acl is not None,
              self.mix_cls, self.mix_sub, self.mix_foff, self.mix_flen,
              self.mix_counts, self.mix_split_ws)
        _lib.sess_split_segments(sg.f_seg, self.mix_cls, self.mix_sub,
                                 ft.count, cap, seg_c)
        fa, fc, fl = self.mix_frames
        # the serve's class, as serve_sessions serves a batch
        clip = None if defer is None else [
            self.mix_cls, self.mix_sub, ft.count, sg.f_seg, *seg_c,
            defer.clipf, defer.deferred]
        a_out, _, a_total, a_err = self._serve_class(
            rx, fa, sg.table(segs, 0), segs, ordered, passes, clip, close,
            self.mix_rec_off[0], False,
            ft.count if perms is not None else None,
            perms.auth if perms is not None else None)
        # the two read engines, after the batch's writes
        c_out, l_out = self.mix_scratch
        c_total, c_err = self.acl_total_err
        if setacl:
            self._setacl_buffers()
            _lib.tree_acl_setacl_sessions(
                tree.tensors, tree.acl, rx, fc.off, fc.length, fc.count, cap,
                sg.table(segs, 1),
                perms.addrs if perms is not None else None,
                perms.auth.tensors if perms is not None and
                perms.auth is not None else None,
                setacl_passes, self.setacl_claim, self.setacl_ctr,
                self._acl_workspace(), self.setacl_ws, c_out, c_out.numel(),
                self.acl_rec_off, c_total, c_err, False)
        elif tree.acl is not None:
            _lib.tree_acl_get_sessions(
                tree.tensors, tree.acl, rx, fc.off, fc.length, fc.count, cap,
                sg.table(segs, 1), self._acl_workspace(), c_out,
                c_out.numel(), self.acl_rec_off, c_total, c_err, False)
        else:
            c_out = l_out
        l_total, l_err = self.list_total_err
        _lib.tree_list_sessions(
            tree.tensors, rx, fl.off, fl.length, fl.count, cap,
            sg.table(segs, 2), max_frame, self.list_want, self.list_ws, l_out,
            l_out.numel(), self.list_rec_off, l_total, l_err, False)
        total, err = self.mix_total_err
        _lib.tree_mix_merge(
            self.mix_cls, self.mix_sub, ft.count, self.mix_counts, cap,
            [a_out, c_out, l_out],
            [self.mix_rec_off[0], self.acl_rec_off, self.list_rec_off],
            [a_total, c_total, l_total], [a_err, c_err, l_err], out,
            out.numel(), self.mix_rec_off[1], total, err, self.mix_merge_ws,
            terminate)
        rec_off = self.mix_rec_off[1]
        self.last_rec_off = rec_off
        self.result = (out, total, err, ft)
        self._sessions_tail(rx, ft, segs, rec_off, total, err, table, resume,
                            close, defer)
        return self.result

    def acl_stats(self):
        """(entries, arena bytes used, lost) of the tree's ACL table: the
        distinct ACLs stored (the open one included), the bytes they take
        (the whole arena once a vector did not fit: the arena is a bump
        allocator), and the created nodes whose ACL found no room (they
        answer GET_ACL with SYSTEMERROR).  One host read."""
        acl = self.tree.acl
        if acl is None:
            raise ValueError('acl_stats: the tree keeps no ACL table')
        c = acl[4].cpu().tolist()
        return (c[_lib.AC_ENT], min(c[_lib.AC_TOP], acl[1].numel()),
                c[_lib.AC_LOST])

    def _setacl_buffers(self):
        """The SET_ACL pass's claim words (one a node, idle), counters and
        workspace, allocated on first use."""
        if self.setacl_claim is None:
            dev = self.tree.device
            # (node_acl covers the node store: the ops check it)
            nodes = self.tree.acl[0].numel()
            self.setacl_claim = torch.full((nodes,), _lib.SETACL_IDLE,
                                           dtype=I32, device=dev)
            self.setacl_ctr = torch.zeros(8, dtype=I64, device=dev)
            self.setacl_ws = torch.empty(
                _lib.tree_setacl_workspace(self.cap_frames), dtype=U8,
                device=dev)

    def setacl_stats(self):
        """What the SET_ACL frames of ``serve_sessions_mixed(setacl=True)``
        came to since the server was built (one host read): frames
        ``applied``, refused ``bad_version``, ``denied`` (NO_AUTH),
        ``invalid`` (INVALID_ACL), ``unreached`` (their node's rounds ran
        out: SYSTEMERROR) and ``store_full`` (the vector found no room:
        SYSTEMERROR).  All 0 on a server that never served one."""
        if self.setacl_ctr is None:
            return dict.fromkeys(_lib.SETACL_STATS, 0)
        return dict(zip(_lib.SETACL_STATS, self.setacl_ctr.cpu().tolist()))

    def setacl_counters(self):
        """The device counters :meth:`setacl_stats` reads (int64 [8], in
        ``_lib.SETACL_STATS`` order), for a caller that folds them into a
        read of its own; no host read."""
        self._setacl_buffers()
        return self.setacl_ctr

    def _acl_enforce_buffers(self):
        """The ACL check's verdicts and counters, allocated on first use."""
        if self.acl_deny is None:
            dev = self.tree.device
            self.acl_deny = torch.zeros(self.cap_frames, dtype=I32,
                                        device=dev)
            self.acl_enf = torch.zeros(8, dtype=I64, device=dev)

    def acl_enforce_stats(self):
        """What ``serve_sessions_mixed(perms=...)`` has decided since the
        server was built (one host read): frames ``checked`` (a verdict was
        reached: the segment served, the body parsed, the target there),
        frames ``denied`` (answered NO_AUTH) and, of those, ``denied_lost``
        (the target's ACL found no room in the store: closed).  All 0 on a
        server that never enforced.  The counts are the check's: a denied
        frame that ``defer`` takes out of its batch is checked, and counted,
        again in the batch that serves it."""
        if self.acl_enf is None:
            return dict.fromkeys(_lib.ACLPERM_STATS, 0)
        return dict(zip(_lib.ACLPERM_STATS, self.acl_enf.cpu().tolist()))

    def auth_stats(self):
        """What the AUTH frames of ``serve_sessions_mixed(perms=
        AclIdentity(addrs, auth=...))`` came to, from the counters of the
        :class:`AuthTable` the last such call used (one host read): frames
        ``ok`` and ``failed``, of the failed those that found their row
        ``full``, of the ok those whose identity the row already held
        (``known``), and the replies written, ``answered_ok`` and
        ``answered_failed`` (a deferred frame is counted by the first four in
        every batch that carries it, by the last two once).  All 0 on a
        server that never served one."""
        if self.auth_table is None:
            return dict.fromkeys(_lib.AUTH_STATS, 0)
        return dict(zip(_lib.AUTH_STATS,
                        self.auth_table.stats.cpu().tolist()))

    def acl_enforce_counters(self):
        """The device counters :meth:`acl_enforce_stats` reads (int64 [8], in
        ``_lib.ACLPERM_STATS`` order, then the replies answered NO_AUTH: a
        deferred frame is not among them before it is served), for a caller
        that folds them into a read of its own (the front end's report); no
        host read."""
        self._acl_enforce_buffers()
        return self.acl_enf

    def _seq_order(self, rx, ft):
        """Number the batch's SEQUENTIAL creates in stream order (parent's
        cversion before the batch + rank among its sequential creates
        here): returns the int64 [cap_frames] words for the serve (parent
        node << 32 | number; -1 none)."""
        L = _lib.lib()
        dev = self.tree.device
        if self.seq_ws is None:
            n = self.cap_frames
            self.seq_ws = torch.empty(L.tree_seq_workspace(n), dtype=U8,
                                      device=dev)
            self.seq_ws[:L.tree_seq_zeroed(n)].zero_()
            self.seqno = torch.empty(n, dtype=I64, device=dev)
        L.tree_seq_order(self.tree.tensors, rx, ft.off, ft.length, ft.count,
                         self.cap_frames, self.seq_ws, self.seqno)
        return self.seqno

    def order_counters(self):
        """The device words :meth:`order_stats` reads — int64 [2]: the
        largest rank, the scratch bytes asked for (more than the scratch
        tail holds: a snapshot found no room) — for a caller that folds them
        into a read of its own (the front end's report); no host read."""
        if self.ows is None:
            raise ValueError('order_counters: no ordered serve has run')
        o = _lib.lib().tree_order_stats_offset(self.cap_frames)
        return self.ows[o:o + 16].view(torch.int64)

    def order_stats(self):
        """(largest same-path rank, scratch bytes used) of the last ordered
        serve (host read).  A rank >= the passes used means refusals."""
        v = self.order_counters().cpu().tolist()
        return v[0], v[1]
