"""A model of the GPU server's watches (csrc/kernels/zk_tree.h wt_*, the arm
and fire block of tree.hip's serve, tree_watch.hip, GpuServer._notify /
_resume / expire) on top of tests/treemodel.py: one object drives the tree,
the fake server's database and the watchers.  Sessions carry a connection
that records the (type, path) of every notification the fake server sends
and are bound to a watcher slot; every call decodes what the GPU server sent
(``srv.notif``, ``srv.resume_notif``) into per-slot lists and compares the
two by :func:`check_events`, then runs the tree audit.

The comparison rule (a plain function, tested without a GPU):

* every batch, per watcher: the multiset of (type, path) equals the model's;
* ordered batches, per watcher: the events other than NodeChildrenChanged
  come in the model's order, and each NodeChildrenChanged of a parent P sits
  where some successful CREATE / DELETE of a child of P of that batch puts
  it (the children of one parent commute in the ordered serve, so which
  sibling takes the parent's mask is the batch's business);
* unordered batches and expiries (one txn): the multiset only.
"""

import collections

from treemodel import TreeModel, _decode, _parent, _stream, dev_bytes

from zkmi import jute
from zkmi.ops import _lib

CC = 'CHILDREN_CHANGED'


# ---- request helpers (watch flags; treemodel's read helpers set none) -------

def wget(path, watch=True):
    return {'opcode': 'GET_DATA', 'path': path, 'watch': bool(watch)}


def wexists(path, watch=True):
    return {'opcode': 'EXISTS', 'path': path, 'watch': bool(watch)}


def ls(path, watch=True, stat=True):
    return {'opcode': 'GET_CHILDREN2' if stat else 'GET_CHILDREN',
            'path': path, 'watch': bool(watch)}


def set_watches(rel, data=(), exist=(), child=()):
    """``rel``: the (tree zxid, model zxid) pair of :meth:`WatchModel.mark`."""
    return {'opcode': 'SET_WATCHES', 'relZxid': rel[0], '_rel_db': rel[1],
            'events': {'dataChanged': list(data),
                       'createdOrDestroyed': list(exist),
                       'childrenChanged': list(child)}}


# ---- the comparison rule ----------------------------------------------------

def check_events(got, want, ordered, writes=()):
    """Compare one batch's notifications.

    ``got``: {watcher slot: [(type, path), ...]} as the GPU server sent
    them, in stream order.  ``want``: the model's events in its order,
    [(request index, slot, type, path), ...].  ``writes``: [(request index,
    path)] of the batch's successful CREATEs and DELETEs.  Returns None when
    ``got`` is acceptable, else a string saying why not."""
    by_slot = collections.defaultdict(list)
    for i, slot, t, path in want:
        by_slot[slot].append((i, t, path))
    for slot in sorted(set(got) | set(by_slot)):
        g = list(got.get(slot, ()))
        w = by_slot.get(slot, [])
        cg = collections.Counter(g)
        cw = collections.Counter((t, p) for _, t, p in w)
        if cg != cw:
            return 'slot %d: multiset differs: extra %r, missing %r' % (
                slot, sorted((cg - cw).elements()),
                sorted((cw - cg).elements()))
        if not ordered:
            continue
        wn = [(i, t, p) for i, t, p in w if t != CC]
        gn = [e for e in g if e[0] != CC]
        if gn != [(t, p) for _, t, p in wn]:
            return 'slot %d: order differs: got %r, want %r' % (
                slot, gn, [(t, p) for _, t, p in wn])
        # each NodeChildrenChanged of P between the neighbours a child write
        # of P allows: a <= j < b for the request indices a, b of the events
        # (other than NodeChildrenChanged) before and after it — a request's
        # own NodeDeleted / NodeCreated precedes its parent's event
        k = 0                           # events of wn seen so far in g
        for e in g:
            if e[0] != CC:
                k += 1
                continue
            a = wn[k - 1][0] if k > 0 else -1
            b = wn[k][0] if k < len(wn) else float('inf')
            js = [j for j, p in writes if _parent(p) == e[1]]
            if not any(a <= j < b for j in js):
                return ('slot %d: %r between requests %r and %r, the '
                        'parent\'s child writes are at %r' % (slot, e, a, b,
                                                              js))
    return None


def first_events(want, n):
    """The model's first ``n`` events (the prefix an overflowing batch
    writes)."""
    return list(want[:n])


# ---- the model --------------------------------------------------------------

class _Conn(object):
    def __init__(self):
        self.got = []

    def send_notification(self, evtype, path):
        self.got.append((evtype, path))

    def close_from_server(self):
        pass


def decode_notifications(buf, total, count):
    """[(type, path)] of the ``count`` xid -1 frames in ``buf[:total]``."""
    raw = bytes(buf[:int(total)].cpu().numpy().tobytes())
    frames, used, bad = jute.scan_frames(raw)
    assert bad < 0 and used == len(raw) and len(frames) == count, \
        (bad, used, len(raw), len(frames), count)
    out = []
    for o, ln in frames:
        pkt = jute.decode_response(raw[o:o + ln], {})
        assert pkt['xid'] == -1 and pkt['state'] == 'SYNC_CONNECTED', pkt
        assert pkt['zxid'] == -1 and pkt['err'] == 'OK', pkt
        out.append((pkt['type'], pkt['path']))
    return out


class WatchModel(TreeModel):
    """:class:`TreeModel` with watchers.  :meth:`serve`, :meth:`expire`
    compare replies, notifications and (through the audit) the tree."""

    def __init__(self, tree, srv, dev):
        self.conns = {}         # watcher slot -> its session's connection
        self.slot_sid = {}      # watcher slot -> session
        self.batches = 0
        self.events = 0         # model events so far
        self.kinds = collections.Counter()
        self.zxids_ok = True
        self.last_sent = {}
        super().__init__(tree, srv, dev)

    def session(self, wslot=-1):
        """A new session; ``wslot`` >= 0 binds it to that watcher slot."""
        s = self.db.new_session(30000)
        if wslot >= 0:
            assert wslot not in self.slot_sid
            s.conn = self.conns[wslot] = _Conn()
            self.slot_sid[wslot] = s.sid
        return s.sid

    def mark(self):
        """(tree zxid, model zxid) now: the relZxid of a later resume."""
        return self.counter(_lib.TC_ZXID), self.db.zxid

    def stats(self):
        return self.srv.watch_stats()

    # -- the GPU's notifications ----------------------------------------------

    def _sent(self):
        """{slot: [(type, path)]} of ``srv.notif``, in stream order."""
        buf, total, slots, count = self.srv.notif
        n = int(count.item())
        ev = decode_notifications(buf, total.item(), n)
        out = collections.defaultdict(list)
        for s, e in zip(slots[:n].cpu().tolist(), ev):
            out[s].append(e)
        return dict(out)

    def _lens(self):
        return {s: len(c.got) for s, c in self.conns.items()}

    def _since(self, lens, i, into):
        for s, c in self.conns.items():
            for t, p in c.got[lens.get(s, 0):]:
                into.append((i, s, t, p))

    # -- the calls ------------------------------------------------------------

    def serve(self, pk, sid=0, wslot=-1, ordered=False, how='serve',
              audit=True, zxids=None, lost_ok=False, overflow=False,
              missing=None, **kw):
        """One batch from session ``sid`` (watcher slot ``wslot``) on the
        server and on the model.  ``how``: 'serve', 'mixed' (serve_mixed) or
        'list' (serve_list: list requests only; sends no notifications).
        SET_WATCHES requests (:func:`set_watches`) make it a resume; their
        events are compared with ``srv.resume_notif``, in order.
        ``overflow``: the batch fires more events than the server has room
        for; the written ones are the model's first ``srv.ecap``.
        ``lost_ok``: the watch table may have lost arms (a full table);
        ``missing``: that many of the model's events are not sent (their
        arms were lost), the others once each (``self.last_sent`` holds
        what was).  Returns (replies, model events [(request, slot, type,
        path)])."""
        srv = self.srv
        for p in pk:
            p['xid'] = self.xid
            self.xid += 1
        resume = any(p['opcode'] == 'SET_WATCHES' for p in pk)
        # (the zxids of a mixed or an ordered batch are not modelled: once
        # one was served the Stats' zxids are no longer compared)
        if how == 'mixed' or ordered:
            self.zxids_ok = False
        if zxids is None:
            zxids = how == 'serve' and not resume and self.zxids_ok
        if sid and wslot >= 0:
            assert self.slot_sid[wslot] == sid
        base = self.counter(_lib.TC_ZXID)
        s = _stream([{k: v for k, v in p.items() if k != '_rel_db'}
                     for p in pk])
        rx = dev_bytes(s, self.dev)
        if how == 'list':
            assert not resume and not ordered
            out, total, err, _ = srv.serve_list(rx, len(s), wslot=wslot)
        elif how == 'mixed':
            assert not ordered
            out, total, err, _ = srv.serve_mixed(rx, len(s), session=sid,
                                                 wslot=wslot, resume=resume)
        else:
            out, total, err, _ = srv.serve(rx, len(s), session=sid,
                                           wslot=wslot, ordered=ordered,
                                           resume=resume, **kw)
        assert int(err.item()) == 0
        reps = _decode(out, total, pk)
        sent = {} if how == 'list' else self._sent()
        ev_total = srv.ev_total.cpu().tolist() if how != 'list' else [0, 0]
        st = srv.watch_stats() if how != 'list' else None
        resumed = None
        if resume:
            buf, rtotal, res = srv.resume_notif
            res = res.cpu().tolist()
            resumed = (decode_notifications(buf, rtotal.item(), res[0]), res)
        # the model, request by request
        want, rwant, writes, keys = [], [], [], []
        listed = 0
        for i, p in enumerate(pk):
            lens = self._lens()
            if p['opcode'] == 'SET_WATCHES':
                q = dict(p, relZxid=p['_rel_db'])
                rep = self.db.handle(q, sid or None)
                assert rep['err'] == 'OK'
                keys.append((p['xid'], 'OK'))
                self._since(lens, i, rwant)
                listed += sum(len(v) for v in p['events'].values())
                continue
            k = self._apply(p, sid or None, base + i + 1, zxids)
            if p['opcode'].startswith('GET_CHILDREN') and k[1] == 'OK':
                k = k + (tuple(sorted(self.db.nodes[p['path']].children)),)
            keys.append(k)
            if k[1] == 'OK' and p['opcode'] in ('CREATE', 'DELETE'):
                writes.append((i, k[2] if p['opcode'] == 'CREATE'
                               else p['path']))
            self._since(lens, i, want)
        got = []
        for r in reps:
            k = self._reply_key(r, zxids)
            if r['err'] == 'OK' and r['opcode'].startswith('GET_CHILDREN'):
                k = k + (tuple(sorted(r['children'])),)
            got.append(k)
        for i, (g, w) in enumerate(zip(got, keys)):
            assert g == w, 'request %d of %d, %r: got %r, want %r' % (
                i, len(pk), {k: v for k, v in pk[i].items() if k != 'acl'},
                g, w)
        self.batches += 1
        self.events += len(want) + len(rwant)
        for _, _, t, _ in want + rwant:
            self.kinds[t] += 1
        # notifications: the model's count first, then the GPU's
        if overflow:
            assert len(want) > srv.ecap
            assert ev_total == [srv.ecap, len(want)], ev_total
            assert st['events_fired'] == len(want) and \
                st['events_written'] == srv.ecap
            want = first_events(want, srv.ecap)
        else:
            assert len(want) <= srv.ecap, len(want)
            assert ev_total[1] == ev_total[0] == len(want) - (missing or 0), \
                (ev_total, len(want), missing)
        if st is not None:
            assert st['encode_err'] == 0, st
            if not lost_ok:
                assert st['lost_arms'] == 0, st
        self.last_sent = sent
        if missing is None:
            bad = check_events(sent, want, ordered, writes)
            assert bad is None, bad
        else:
            for slot, ev in sent.items():
                extra = collections.Counter(ev) - collections.Counter(
                    (t, p) for _, s_, t, p in want if s_ == slot)
                assert not extra, (slot, extra)
        if resume:
            ev, res = resumed
            assert ev == [(t, p) for _, _, t, p in rwant], (ev[:5],
                                                            rwant[:5])
            assert res[0] == res[2] == len(rwant), res
            assert res[1] == listed - len(rwant), (res, listed)
            assert res[3] == 0, res
            assert st['resume_dropped'] == 0 and st['resume_err'] == 0, st
        if audit:
            self.audit(zxids=self.zxids_ok)
        return reps, want

    def _apply(self, p, sid, z, zxids):
        if p['opcode'].startswith('GET_CHILDREN'):
            rep = self.db.handle(dict(p), sid)
            k = (p['xid'], rep['err'])
            if rep['err'] == 'OK' and p['opcode'] == 'GET_CHILDREN2':
                k += (self._stat_key(p['path'], zxids),)
            return k
        return super()._apply(p, sid, z, zxids)

    def audit(self, zxids=True):
        return super().audit(zxids=zxids and self.zxids_ok)

    def _expire_on_gpu(self, sid):
        wslot = self._exp_wslot
        removed = int(self.srv.expire(sid, wslot=wslot).item())
        self._exp_sent = self._sent()
        self._exp_total = self.srv.ev_total.cpu().tolist()
        self._exp_stats = self.srv.watch_stats()
        return removed

    def expire(self, sid, audit=True):
        """Expire ``sid`` on both (one txn): the watchers' events compared
        as multisets; the session's slot, if it has one, is unbound and its
        own watches go."""
        wslot = None
        for s, x in self.slot_sid.items():
            if x == sid:
                wslot = s
        self._exp_wslot = wslot
        lens = self._lens()
        removed = super().expire(sid, audit=audit)
        want = []
        self._since(lens, 0, want)
        if wslot is not None:
            assert not [e for e in want if e[1] == wslot]
            del self.slot_sid[wslot]
            del self.conns[wslot]
        self.events += len(want)
        for _, _, t, _ in want:
            self.kinds[t] += 1
        assert len(want) <= self.srv.ecap
        assert self._exp_total == [len(want), len(want)], (self._exp_total,
                                                           len(want))
        st = self._exp_stats
        assert st['encode_err'] == 0 and st['expiry_dropped'] == 0, st
        bad = check_events(self._exp_sent, want, False)
        assert bad is None, bad
        return removed, want
