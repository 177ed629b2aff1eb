"""A model of the GPU tree (csrc/kernels/zk_tree.h, tree.hip) for the churn
tests: the fake server's database applied request by request, the zxids the
tree's documented rule predicts, the set of dead paths, and an audit that
reads every znode back after each mutating call.

Also the host side of two things the kernels compute: the home slot of a
path in the hash index (names chosen to crowd one window of the table) and
the in-batch ranks of the ordered serve (tree_order.hip's header)."""

import functools
import random

import numpy as np
import torch

from zkmi import jute
from zkmi.ops import _lib
from zkmi.server.fakezk import ZKDatabase

NODE_FREE = -2          # node_parent of a free node (zk_tree.h)
EN_PATH = 40            # path bytes held in a hash entry (zk_tree.h)
_M64 = (1 << 64) - 1
_MUL = 0xFF51AFD7ED558CCD


class _Loop(object):
    """Just enough of an event loop for ZKDatabase (no expiry ticks run)."""

    class _H(object):
        def cancel(self):
            pass

    def call_later(self, ms, fn):
        return self._H()

    def time_ms(self):
        return 0


def _parent(path):
    return path[:path.rfind('/')]


# ---- the hash index on the host ---------------------------------------------

def home_slot(path, hcap):
    """The first entry the probe for ``path`` looks at (zk_tree.h
    tree_lookup: key & mask, key = path_hash | 1)."""
    return _lib.acl_hash(path.encode()) & (hcap - 1)


@functools.lru_cache(maxsize=None)
def window_names(count, hcap, fmt='/bench/d000000/c%07d', half=8):
    """``count`` names ``fmt % k`` whose home slot lies in the 2 * ``half``
    entries straddling the table end, [hcap - half, hcap) and [0, half):
    probe chains over them are long, wrap around, and hold tombstones
    between live entries of other keys."""
    out = []
    k = 0
    while len(out) < count:
        p = fmt % k
        s = home_slot(p, hcap)
        if s >= hcap - half or s < half:
            out.append(p)
        k += 1
    return tuple(out)


def _step(h, w):
    h = ((h ^ w) * _MUL) & _M64
    return h ^ (h >> 32)


def hash_twin(path, k, seed=0):
    """Another path of the same length and the same 64-bit path hash that
    differs from ``path`` in its 8-byte words ``k`` and ``k + 1`` only (the
    index tells the two apart by comparing the bytes, zk_tree.h ent_is).
    path_hash folds a word as h = f((h ^ w) * M): any other word k is made
    up for by the word after it."""
    b = path.encode()
    assert 8 * (k + 2) <= len(b)
    h = 0x9E3779B97F4A7C15 ^ len(b)
    for i in range(k):
        h = _step(h, int.from_bytes(b[8 * i:8 * i + 8], 'little'))
    w1 = int.from_bytes(b[8 * k:8 * k + 8], 'little')
    w2 = int.from_bytes(b[8 * k + 8:8 * k + 16], 'little')
    t = _step(h, w1) ^ w2
    rng = random.Random(seed)
    abc = b'abcdefghijklmnopqrstuvwxyz0123456789'
    while True:
        c1 = bytes(rng.choice(abc) for _ in range(8))
        c2 = (_step(h, int.from_bytes(c1, 'little')) ^ t).to_bytes(8,
                                                                   'little')
        if all(0x21 <= x <= 0x7e and x != 0x2f for x in c2) and \
                c1 != b[8 * k:8 * k + 8]:
            twin = (b[:8 * k] + c1 + c2 + b[8 * k + 16:]).decode()
            assert _lib.acl_hash(twin.encode()) == _lib.acl_hash(b)
            return twin


# ---- the ordered serve's ranks on the host ----------------------------------

def host_ranks(pk):
    """The rank of every request of the batch ``pk`` by the rule in
    tree_order.hip's header: every request is an A member of its own path's
    group, a CREATE / DELETE a C member of its parent's group (a SEQUENTIAL
    create only that; a child of the root has no parent group); edges run
    from the earlier to the later request of a group, A-A when the group has
    an A writer anywhere in the batch, A-C and C-A always, C-C never; the
    rank is the longest chain of edges ending at the request."""
    aw = set()
    for p in pk:
        if p['opcode'] in ('CREATE', 'DELETE', 'SET_DATA') and \
                'SEQUENTIAL' not in p.get('flags', ()):
            aw.add(p['path'])
    max_a, max_c = {}, {}       # group -> largest rank of an earlier member
    ranks = []
    for p in pk:
        op, path = p['opcode'], p['path']
        seq = op == 'CREATE' and 'SEQUENTIAL' in p.get('flags', ())
        par = None
        if op in ('CREATE', 'DELETE') and path.rfind('/') > 0:
            par = _parent(path)
        r = 0
        if not seq:
            r = max(r, max_c.get(path, -1) + 1)
            if path in aw:
                r = max(r, max_a.get(path, -1) + 1)
        if par is not None:
            r = max(r, max_a.get(par, -1) + 1)
        if not seq:
            max_a[path] = max(max_a.get(path, -1), r)
        if par is not None:
            max_c[par] = max(max_c.get(par, -1), r)
        ranks.append(r)
    return ranks


# ---- wire helpers -----------------------------------------------------------

def dev_bytes(b, dev):
    a = np.frombuffer(bytes(b) if b else b'\0', np.uint8).copy()
    return torch.from_numpy(a).to(dev)


def _decode(out, total, pk):
    raw = bytes(out[:int(total.item())].cpu().numpy().tobytes())
    frames, used, bad = jute.scan_frames(raw)
    assert bad < 0 and used == len(raw) and len(frames) == len(pk), \
        (bad, used, len(raw), len(frames), len(pk))
    xmap = {p['xid']: p['opcode'] for p in pk}
    reps = [jute.decode_response(raw[o:o + ln], xmap) for o, ln in frames]
    assert [r['xid'] for r in reps] == [p['xid'] for p in pk]
    return reps


def _stream(pk):
    return b''.join(jute.frame(jute.encode_request(p)) for p in pk)


def create(path, data=b'', flags=()):
    return {'opcode': 'CREATE', 'path': path, 'data': data,
            'acl': jute.DEFAULT_ACL, 'flags': list(flags)}


def set_data(path, data, version=-1):
    return {'opcode': 'SET_DATA', 'path': path, 'data': data,
            'version': version}


def delete(path, version=-1):
    return {'opcode': 'DELETE', 'path': path, 'version': version}


def get(path):
    return {'opcode': 'GET_DATA', 'path': path, 'watch': False}


def exists(path):
    return {'opcode': 'EXISTS', 'path': path, 'watch': False}


# ---- the model --------------------------------------------------------------

class TreeModel(object):
    """``tree`` / ``srv`` and the fake server's database holding the same
    znodes.  :meth:`serve` sends one batch to both and compares the replies,
    :meth:`expire` one session expiry; both end with :meth:`audit`."""

    def __init__(self, tree, srv, dev):
        self.tree, self.srv, self.dev = tree, srv, dev
        self.db = ZKDatabase(_Loop())
        self.zx = {}            # path -> [czxid, mzxid, pzxid] (tree's rule)
        self.dead = set()       # every path that existed and does not now
        self.touched = set()    # parents written under since the last audit
        self.xid = 0
        self.audits = 0
        nodes = self._node_table()
        for v in range(tree.n_static):          # node v: czxid v + 1
            path = nodes['paths'][v]
            data, _ = tree.node_slot_host(v)
            self.db.create(path, data or b'', [self.db._world()], [], None)
            self.zx[path] = [v + 1, v + 1, v + 1]
        self.node_of = {}
        self.slot_cap = None
        self.audit()

    def session(self):
        return self.db.new_session(30000).sid

    def live(self):
        return [p for p in self.db.nodes if p not in ('/', '/zookeeper')]

    def counter(self, k):
        return int(self.tree.counters[k].item())

    # -- one request on the model ---------------------------------------------

    def _stat_key(self, path, zxids):
        st = self.db.nodes[path].stat
        k = (st.version, st.dataLength, st.numChildren, st.cversion,
             st.ephemeralOwner)
        return k + tuple(self.zx[path]) if zxids else k

    def _apply(self, p, sid, z, zxids):
        """Apply request ``p`` (the batch's write number ``z``) to the
        model; returns what the reply must show."""
        op, path = p['opcode'], p['path']
        if op == 'SET_DATA' and path in self.db.nodes:
            # the tree's divergence from ZooKeeper: data that does not fit
            # the node's slot is refused, before the version is looked at
            v = self.node_of.get(path)
            if v is not None and len(p['data']) > int(self.slot_cap[v]):
                return (p['xid'], 'BAD_ARGUMENTS')
        rep = self.db.handle(dict(p), sid)
        k = [p['xid'], rep['err']]
        if rep['err'] != 'OK':
            return tuple(k)
        if op == 'CREATE':
            new = rep['path']
            k.append(new)
            self.zx[new] = [z, z, z]
            self.dead.discard(new)
            par = _parent(new)
            self.zx[par][2] = max(self.zx[par][2], z)
            self.touched.add(par)
        elif op == 'DELETE':
            del self.zx[path]
            self.dead.add(path)
            par = _parent(path)
            self.zx[par][2] = max(self.zx[par][2], z)
            self.touched.add(par)
        elif op == 'SET_DATA':
            self.zx[path][1] = z
            k.append(self._stat_key(path, zxids))
        elif op == 'GET_DATA':
            k += [bytes(rep['data'] or b''), self._stat_key(path, zxids)]
        elif op == 'EXISTS':
            k.append(self._stat_key(path, zxids))
        return tuple(k)

    @staticmethod
    def _reply_key(rep, zxids):
        k = [rep['xid'], rep['err']]
        if rep['err'] != 'OK':
            return tuple(k)
        if rep['opcode'] == 'CREATE':
            k.append(rep['path'])
        if rep['opcode'] == 'GET_DATA':
            k.append(bytes(rep['data'] or b''))
        st = rep.get('stat')
        if st is not None:
            s = (st.version, st.dataLength, st.numChildren, st.cversion,
                 st.ephemeralOwner)
            if zxids:
                s += (st.czxid, st.mzxid, st.pzxid)
            k.append(s)
        return tuple(k)

    # -- the calls ------------------------------------------------------------

    def serve(self, pk, sid=0, audit=True, zxids=True, **kw):
        """One batch on the tree and on the model (request by request, in
        batch order).  Returns (replies, wanted keys); the two are compared
        here.  ``zxids``: compare the Stat's three zxids and the reply
        headers' (the unordered rule: write i carries the counter + i + 1,
        a read the counter).  ``kw`` goes to ``GpuServer.serve``."""
        for p in pk:
            p['xid'] = self.xid
            self.xid += 1
        base = self.counter(_lib.TC_ZXID)
        s = _stream(pk)
        out, total, err, _ = self.srv.serve(dev_bytes(s, self.dev), len(s),
                                            session=sid, **kw)
        assert int(err.item()) == 0
        reps = _decode(out, total, pk)
        want = [self._apply(p, sid or None, base + i + 1, zxids)
                for i, p in enumerate(pk)]
        got = [self._reply_key(r, zxids) for r in reps]
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, 'request %d of %d, %r: got %r, want %r' % (
                i, len(pk), {k: v for k, v in pk[i].items() if k != 'acl'},
                g, w)
        if zxids:
            for i, (p, r) in enumerate(zip(pk, reps)):
                wr = p['opcode'] in ('CREATE', 'SET_DATA', 'DELETE')
                assert r['zxid'] == (base + i + 1 if wr else base), (i, r)
        assert self.counter(_lib.TC_ZXID) == base + len(pk)
        if audit:
            self.audit(zxids=zxids)
        return reps, want

    def serve_full_index(self, pk):
        """Serve the creates ``pk`` of new names on an index with fewer
        empty entries than requests: every reply is OK or SYSTEM_ERROR
        (which of the concurrent creates find an entry is the batch's
        business); the model applies the ones that succeeded, their numbers
        kept, and the audit checks that the failed ones left nothing.
        Returns the error names."""
        for p in pk:
            p['xid'] = self.xid
            self.xid += 1
            assert p['opcode'] == 'CREATE' and p['path'] not in self.db.nodes
        base = self.counter(_lib.TC_ZXID)
        s = _stream(pk)
        out, total, err, _ = self.srv.serve(dev_bytes(s, self.dev), len(s))
        assert int(err.item()) == 0
        reps = _decode(out, total, pk)
        got = [r['err'] for r in reps]
        assert set(got) <= {'OK', 'SYSTEM_ERROR'}, set(got)
        for i, (p, r) in enumerate(zip(pk, reps)):
            if r['err'] == 'OK':
                assert r['path'] == p['path']
                assert self._apply(p, None, base + i + 1, True)[1] == 'OK'
        self.audit()
        return got

    def expire(self, sid, audit=True):
        """Expire session ``sid`` on both; returns the number removed (the
        tree's, checked against the model's).  All removals carry the
        counter + 1."""
        z = self.counter(_lib.TC_ZXID) + 1
        s = self.db.sessions.get(sid)
        gone = sorted(s.ephemerals) if s is not None else []
        for path in gone:
            assert path in self.db.nodes
            par = _parent(path)
            self.zx[par][2] = max(self.zx[par][2], z)
            self.touched.add(par)
            del self.zx[path]
            self.dead.add(path)
        self.db.expire_session(sid)
        removed = self._expire_on_gpu(sid)
        assert removed == len(gone)
        assert self.counter(_lib.TC_ZXID) == z
        if audit:
            self.audit()
        return removed

    def _expire_on_gpu(self, sid):
        return int(self.tree.expire(sid).item())

    # -- the audit ------------------------------------------------------------

    def _node_table(self):
        t = self.tree
        c = t.counters.cpu().tolist()
        n = min(c[_lib.TC_NODES], t.cap)
        par = t.node_parent[:n].cpu().numpy()
        pw = t.node_pw[:n].cpu().numpy()
        arena = t.path_arena.cpu().numpy().tobytes()
        off, ln = pw >> 24, pw & 0xFFFFFF
        paths = [arena[off[v]:off[v] + ln[v]].decode('latin-1')
                 if par[v] != NODE_FREE else None for v in range(n)]
        return {'counters': c, 'n': n, 'parent': par, 'paths': paths}

    def _read(self, pk):
        for p in pk:
            p['xid'] = self.xid
            self.xid += 1
        reps = []
        cap = self.srv.cap_frames
        for o in range(0, len(pk), cap):
            part = pk[o:o + cap]
            s = _stream(part)
            out, total, err, _ = self.srv.serve(dev_bytes(s, self.dev),
                                                len(s))
            assert int(err.item()) == 0
            reps += _decode(out, total, part)
        return reps

    def audit(self, zxids=True):
        """Every live znode answers its bytes and Stat, every dead path
        NO_NODE; the digest's counts, the lists of the parents written
        under, and the free ring agree with the model."""
        t = self.tree
        self.audits += 1
        live = sorted(self.live())
        dead = sorted(self.dead)
        assert not (set(live) & self.dead)
        # read-back through the index: an entry lost, duplicated or bound to
        # a recycled node of another path shows here
        pk = [get(p) for p in live] + [exists(p) for p in dead]
        reps = self._read(pk)
        for p, r in zip(pk, reps):
            path = p['path']
            if p['opcode'] == 'EXISTS':
                assert r['err'] == 'NO_NODE', ('dead path answers', path, r)
                continue
            assert r['err'] == 'OK', ('live path lost', path, r)
            node = self.db.nodes[path]
            got = self._reply_key(r, zxids)[2:]
            want = (bytes(node.data or b''), self._stat_key(path, zxids))
            assert got == want, (path, got, want)
        # the digest's counts
        _, nlive, used, tomb = t.digest()
        assert nlive == len(live), (nlive, len(live))
        assert used - tomb == nlive, (used, tomb, nlive)
        assert used <= t.hcap
        # the node table: exactly the model's paths, each at one node
        nt = self._node_table()
        node_of = {}
        for v, path in enumerate(nt['paths']):
            if path is not None:
                assert path not in node_of, ('two nodes of one path', path)
                node_of[path] = v
        assert sorted(node_of) == live
        for path, v in node_of.items():
            pp = _parent(path)
            assert nt['parent'][v] == (node_of[pp] if pp else -1), path
        self.node_of = node_of
        self.slot_cap = t.slot_cap[:nt['n']].cpu().numpy()
        # lists of the parents touched since the last audit
        self._audit_lists(sorted(self.touched))
        self.touched = set()
        # the free ring: pending entries distinct, free, and no live node
        c = nt['counters']
        head, pub = c[_lib.TC_FREE_HEAD], c[_lib.TC_FREE_PUB]
        assert c[_lib.TC_FREE_TAIL] == pub and head <= pub
        assert c[_lib.TC_DIRTY] == 0
        assert pub - head <= t.cap
        assert c[_lib.TC_NODES] <= t.cap
        ring = t.free_list.cpu().numpy()
        pend = [int(ring[k % t.cap]) for k in range(head, pub)]
        assert len(set(pend)) == len(pend), 'a node twice in the free ring'
        livenodes = set(node_of.values())
        for v in pend:
            assert 0 <= v < nt['n']
            assert nt['parent'][v] == NODE_FREE, ('ring node not free', v)
            assert v not in livenodes, ('live node in the free ring', v)
        assert nlive + len(pend) == c[_lib.TC_NODES], \
            (nlive, len(pend), c[_lib.TC_NODES])
        return nt

    def _audit_lists(self, parents):
        if not parents:
            return
        pk = [{'opcode': 'GET_CHILDREN2', 'path': p, 'watch': False}
              for p in parents]
        for p in pk:
            p['xid'] = self.xid
            self.xid += 1
        cap = self.srv.cap_frames
        for o in range(0, len(pk), cap):
            part = pk[o:o + cap]
            s = _stream(part)
            out, total, err, _ = self.srv.serve_list(dev_bytes(s, self.dev),
                                                     len(s))
            assert int(err.item()) == 0
            for p, r in zip(part, _decode(out, total, part)):
                node = self.db.nodes.get(p['path'])
                if node is None:
                    assert r['err'] == 'NO_NODE', (p['path'], r)
                    continue
                assert r['err'] == 'OK', (p['path'], r)
                assert sorted(r['children']) == sorted(node.children), \
                    p['path']
                assert r['stat'].numChildren == len(node.children)
