"""Model-checked watches of the GPU server (csrc/kernels/zk_tree.h wt_*, the
arm and fire block of tree.hip's serve, tree_watch.hip, GpuServer._notify /
_resume / expire): random and scripted histories whose every batch is
compared with the fake server — replies, the notifications of every watcher
by the rule of tests/watchmodel.py check_events, the loss counters of
GpuServer.watch_stats, and the tree audit of tests/treemodel.py.

The rule itself and the generators' contracts are tested without a GPU."""

import collections
import random

import pytest

from treemodel import (create, delete, hash_twin, home_slot, host_ranks,
                       set_data, window_names)
from watchmodel import (CC, WatchModel, check_events, ls, set_watches, wexists,
                        wget)

from zkmi.ops import _lib

FANOUT = 100
NLEAF = 2000
NDIR = NLEAF // FANOUT
SLOTS = (0, 31, 32, 63)     # the edges of a 32-bit shift and of the sign bit


def leaf(i):
    return '/bench/d%06d/n%09d' % (i // FANOUT, i)


def dirp(d):
    return '/bench/d%06d' % d


def _model(gpu, frames=1024, watch_cap=4096):
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(NLEAF, 16, fanout=FANOUT, device=gpu, seed=3,
                   watch_cap=watch_cap, scratch=1 << 20)
    srv = GpuServer(tree, frames, 1 << 21)
    return WatchModel(tree, srv, gpu)


def _data(rng, hi=100):
    return bytes(rng.getrandbits(8) for _ in range(rng.randint(0, hi)))


# ---- host-only: the comparison rule -----------------------------------------

def test_check_events_rule():
    """Each clause of the rule on hand-made sequences, accepted and
    rejected."""
    a, b, p = '/p/a', '/p/b', '/p'
    D, C, X = 'DATA_CHANGED', 'CREATED', 'DELETED'
    # -- the multiset, every batch, per watcher
    want = [(0, 0, D, a), (1, 0, D, b), (1, 63, D, b)]
    assert check_events({0: [(D, a), (D, b)], 63: [(D, b)]}, want,
                        False) is None
    assert 'missing' in check_events({0: [(D, a)], 63: [(D, b)]}, want, False)
    assert 'extra' in check_events({0: [(D, a), (D, b), (D, b)],
                                    63: [(D, b)]}, want, False)
    # the right events at the wrong watcher
    assert check_events({0: [(D, a), (D, b)], 31: [(D, b)]}, want,
                        False) is not None
    # the right path with the wrong type
    assert check_events({0: [(D, a), (C, b)], 63: [(D, b)]}, want,
                        False) is not None
    # nothing wanted, something sent (a failed write that fired)
    assert check_events({5: [(D, a)]}, [], False) is not None
    assert check_events({}, [], True) is None
    # -- unordered: any order
    assert check_events({0: [(D, b), (D, a)], 63: [(D, b)]}, want,
                        False) is None
    # -- ordered: the events other than NodeChildrenChanged in model order
    assert check_events({0: [(D, a), (D, b)], 63: [(D, b)]}, want,
                        True) is None
    assert 'order' in check_events({0: [(D, b), (D, a)], 63: [(D, b)]}, want,
                                   True)
    # -- ordered: a NodeChildrenChanged at a sibling's position.  Requests:
    # 0 set a, 1 create /p/x, 2 set b, 3 delete /p/y, 4 set a again
    writes = [(1, '/p/x'), (3, '/p/y')]
    want = [(0, 7, D, a), (1, 7, CC, p), (2, 7, D, b)]
    assert check_events({7: [(D, a), (CC, p), (D, b)]}, want, True,
                        writes) is None
    # the other sibling took the mask: after request 2's event
    assert check_events({7: [(D, a), (D, b), (CC, p)]}, want, True,
                        writes) is None
    # before any child write of the batch
    assert 'between' in check_events({7: [(CC, p), (D, a), (D, b)]}, want,
                                     True, writes)
    # after an event of a request later than the last child write
    want5 = want + [(4, 7, D, a)]
    assert check_events({7: [(D, a), (D, b), (CC, p), (D, a)]}, want5, True,
                        writes) is None
    assert 'between' in check_events({7: [(D, a), (D, b), (D, a), (CC, p)]},
                                     want5, True, writes)
    # a request's own NodeDeleted comes before its parent's event
    want = [(3, 7, X, '/p/y'), (3, 7, CC, p)]
    assert check_events({7: [(X, '/p/y'), (CC, p)]}, want, True,
                        writes) is None
    # a NodeChildrenChanged of a parent without a child write
    assert check_events({7: [(CC, '/q')]}, [(1, 7, CC, '/q')], True,
                        writes) is not None
    # -- an expiry (one txn): the multiset
    want = [(0, 1, X, a), (0, 1, CC, p), (0, 2, X, b)]
    assert check_events({1: [(CC, p), (X, a)], 2: [(X, b)]}, want,
                        False) is None
    assert check_events({1: [(X, a)], 2: [(X, b)]}, want, False) is not None


# ---- 1. / 2. churn ----------------------------------------------------------

class _Churn(object):
    """Unordered batches over ~200 paths — 25 leaves and 20 missing names
    (path lengths of every residue mod 8) in each of four directories, the
    directories themselves — that keep the batch contract: a path appears
    once in a batch; a directory that gets a CREATE / DELETE of a child does
    not appear in it (so no watched read meets a write of its path or of
    one of its children); the rest of a large batch are plain reads of
    leaves outside the pool."""

    DIRS = 4

    def __init__(self, m, rng):
        self.m, self.rng = m, rng
        self.kids = {}
        for d in range(self.DIRS):
            names = ['%s/m%s%02d' % (dirp(d), 'x' * (j % 16), j)
                     for j in range(20)]
            self.kids[dirp(d)] = [leaf(FANOUT * d + k) for k in range(25)] + \
                names
        self.filler = [leaf(k) for k in range(FANOUT * self.DIRS, NLEAF)]

    def pool(self):
        return [p for ks in self.kids.values() for p in ks] + list(self.kids)

    def _read(self, path, watcher):
        rng = self.rng
        w = watcher and rng.random() < 0.7
        r = rng.random()
        if r < 0.40:
            return wget(path, w)
        if r < 0.75:
            return wexists(path, w)
        return ls(path, w, stat=rng.random() < 0.5)

    def _write(self, path):
        rng, db = self.rng, self.m.db
        node = db.nodes.get(path)
        if node is None:
            r = rng.random()
            if r < 0.80:
                fl = ['EPHEMERAL'] if rng.random() < 0.4 else []
                return create(path, _data(rng), fl)
            return set_data(path, b'lost') if r < 0.9 else delete(path)
        ver = node.stat.version
        r = rng.random()
        if r < 0.35:
            return set_data(path, _data(rng), rng.choice([ver, -1]))
        if r < 0.45:
            return set_data(path, b'stale', ver + 1 + rng.randint(0, 2))
        if r < 0.80:
            return delete(path, rng.choice([ver, -1]))
        if r < 0.90:
            return delete(path, ver + 1)
        return create(path, b'twice')

    def batch(self, n, watcher, force_delete=()):
        """``n`` requests; ``watcher``: the session has a slot (its reads
        may set watch), else it mostly writes."""
        rng = self.rng
        pk = []
        pw = 0.25 if watcher else 0.8
        for d, ks in self.kids.items():
            forced = [p for p in force_delete if p in ks]
            if forced or rng.random() < 0.6:
                # the children's turn: any op on them, none on the directory
                for p in ks:
                    if p in forced:
                        pk.append(delete(p))
                    elif rng.random() < pw:
                        pk.append(self._write(p))
                    else:
                        pk.append(self._read(p, watcher))
            else:
                # the directory's turn: its children are read or set only
                if rng.random() < 0.3:
                    node = self.m.db.nodes[d]
                    pk.append(rng.choice([
                        set_data(d, _data(rng)), delete(d),
                        set_data(d, b'v', node.stat.version + 1)]))
                else:
                    pk.append(self._read(d, watcher))
                for p in ks:
                    node = self.m.db.nodes.get(p)
                    if node is not None and rng.random() < pw:
                        pk.append(set_data(p, _data(rng)))
                    else:
                        pk.append(self._read(p, False))
        rng.shuffle(pk)
        keep = [p for p in pk if p['path'] in force_delete]
        pk = keep + [p for p in pk if p['path'] not in force_delete]
        pk = pk[:n]
        for path in rng.sample(self.filler, max(0, n - len(pk))):
            pk.append(wget(path, False) if rng.random() < 0.5
                      else wexists(path, False))
        rng.shuffle(pk)
        return pk


def check_contract(pk):
    """The unordered batch contract of the generator (asserted on the CPU
    for every batch it makes)."""
    paths = [p['path'] for p in pk]
    assert len(set(paths)) == len(paths), 'a path twice'
    cpar = {p['path'][:p['path'].rfind('/')] for p in pk
            if p['opcode'] in ('CREATE', 'DELETE')}
    assert not (cpar & set(paths)), 'a parent beside its child\'s write'


def _how(pk):
    return 'mixed' if any(p['opcode'].startswith('GET_CHILDREN')
                          for p in pk) else 'serve'


def test_churn_generator_keeps_the_contract():
    """The generator on a model without a GPU (the fake database alone):
    every batch keeps the contract, the pool is about 200 paths and the
    created names' lengths cover every residue mod 8."""

    class _M(object):
        pass
    from treemodel import _Loop
    from zkmi.server.fakezk import ZKDatabase
    m = _M()
    m.db = ZKDatabase(_Loop())
    w = ZKDatabase._world()
    m.db.create('/bench', b'', [w], [], None)
    for d in range(NDIR):
        m.db.create(dirp(d), b'', [w], [], None)
    for i in range(NLEAF):
        m.db.create(leaf(i), b'x', [w], [], None)
    rng = random.Random(7)
    ch = _Churn(m, rng)
    assert 180 <= len(ch.pool()) <= 220
    made = [p for p in ch.pool() if p not in m.db.nodes]
    assert {len(p) % 8 for p in made} == set(range(8))
    for n in (1, 64, 65, 257, 600) * 3:
        pk = ch.batch(n, rng.random() < 0.8)
        assert len(pk) == n
        check_contract(pk)


SIZES = (1, 64, 65, 257, 600)


@pytest.mark.gpu
def test_unordered_watch_churn(gpu):
    """25 generations of contract-keeping batches of 1, 64, 65, 257 and 600
    requests from four watcher sessions (slots 0, 31, 32, 63) and a writer:
    watched and unwatched GET_DATA / EXISTS / lists (lists through
    serve_mixed), right and wrong SET_DATA / DELETE / CREATE, EPHEMERAL
    creates.  Every fifth generation all four watchers take a data and a
    child watch on one leaf and a child watch on its directory, and the
    writer's next batch deletes it: one request fires all three masks to
    several watchers, each told NodeDeleted once."""
    m = _model(gpu)
    rng = random.Random(23)
    ch = _Churn(m, rng)
    sess = [(m.session(s), s) for s in SLOTS] + [(m.session(), -1)]
    fired3 = 0
    for g in range(25):
        n = SIZES[g % len(SIZES)]
        if g % 5 == 3:
            # a leaf of the pool that exists, watched three ways by all
            x = rng.choice([p for ks in ch.kids.values() for p in ks
                            if p in m.db.nodes])
            for sid, slot in sess[:4]:
                m.serve([wget(x), ls(x), ls(x[:x.rfind('/')])], sid=sid,
                        wslot=slot, how='mixed', audit=False)
            force = (x,)
            sid, slot = sess[4]
        else:
            force = ()
            sid, slot = sess[rng.randrange(5)]
        pk = ch.batch(n, slot >= 0, force_delete=force)
        check_contract(pk)
        _, want = m.serve(pk, sid=sid, wslot=slot, how=_how(pk))
        if force:
            # 4 watchers x (NodeDeleted once + the parent's event, which the
            # model gives the parent's first child write of the batch)
            x = force[0]
            assert sorted(s for _, s, t, p in want
                          if (t, p) == ('DELETED', x)) == list(SLOTS), want
            assert sorted(s for _, s, t, p in want
                          if (t, p) == (CC, x[:x.rfind('/')])) == list(SLOTS)
            fired3 += 1
    assert fired3 == 5
    # the history fired every kind, to every slot
    assert set(m.kinds) == {'CREATED', 'DELETED', 'DATA_CHANGED', CC}, m.kinds
    assert m.events > 300, m.events
    st = m.stats()
    assert st['lost_arms'] == 0


def _ordered_pool():
    d0 = dirp(0)
    l1 = ['%s/a%d' % (d0, k) for k in range(8)]
    l2 = ['%s/b%s%d' % (p, 'y' * k, k) for p in l1 for k in range(4)]
    l3 = ['%s/c%d' % (p, k) for p in l2[::2] for k in range(4)]
    return l1, l2, l3


def _ordered_batch(rng, n, watcher):
    """Like the tree churn's ordered batch, with watch flags: same-path and
    parent / child conflicts as they fall — a read with watch followed by a
    write of its path among them."""
    l1, l2, l3 = _ordered_pool()
    pool = l1 + l2 + l3
    pk = []
    for _ in range(n):
        path = rng.choice(pool)
        w = watcher and rng.random() < 0.6
        r = rng.random()
        if r < 0.28:
            fl = ['EPHEMERAL'] if path in l3 and rng.random() < 0.5 else []
            pk.append(create(path, _data(rng), fl))
        elif r < 0.42:
            pk.append(set_data(path, _data(rng),
                               rng.choice([-1, -1, 0, 1, 2])))
        elif r < 0.62:
            pk.append(delete(path, rng.choice([-1, -1, -1, 0, 1])))
        elif r < 0.82:
            pk.append(wget(path, w))
        else:
            pk.append(wexists(path, w))
    return pk


ORD_PASSES = 24
ORD_ROUNDS = 8
ORD_N = 300


def _ordered_rounds():
    rng = random.Random(29)
    out = []
    for r in range(ORD_ROUNDS):
        k = r % 5                       # the session of the round
        out.append((k, _ordered_batch(rng, ORD_N, k < 4)))
    return out


def test_ordered_watch_rounds_fit_the_passes():
    """The fixed seed's batches rank under the passes the GPU test uses and
    hold a watched read followed by a write of its path."""
    l1, l2, l3 = _ordered_pool()
    assert len(l1 + l2 + l3) == 104
    mx = []
    rw = 0
    for _, pk in _ordered_rounds():
        mx.append(max(host_ranks(pk)))
        armed = set()
        for p in pk:
            if p.get('watch'):
                armed.add(p['path'])
            elif p['opcode'] in ('SET_DATA', 'DELETE', 'CREATE') and \
                    p['path'] in armed:
                rw += 1
    assert max(mx) < ORD_PASSES and min(mx) >= 6, mx
    assert rw > 50


@pytest.mark.gpu
def test_ordered_watch_churn(gpu):
    """8 rounds of 300 random requests over 104 paths in three levels,
    served in order by the five sessions in turn; before each round every
    watcher lists a dozen of the paths and parents with watch (serve_list),
    so the round's creates and deletes fire child watches too.  Replies as
    the fake server gives them one by one; per watcher the events in the
    model's order, a parent's NodeChildrenChanged where one of its
    children's writes of the batch puts it."""
    m = _model(gpu, frames=512)
    srv = m.srv
    rng = random.Random(31)
    sess = [(m.session(s), s) for s in SLOTS] + [(m.session(), -1)]
    l1, l2, l3 = _ordered_pool()
    parents = [dirp(0)] + l1 + l2
    for k, pk in _ordered_rounds():
        for sid, slot in sess[:4]:
            m.serve([ls(p, True, stat=rng.random() < 0.5)
                     for p in rng.sample(parents, 12)], sid=sid, wslot=slot,
                    how='list', audit=False)
        want_max = max(host_ranks(pk))
        assert want_max < ORD_PASSES
        sid, slot = sess[k]
        reps, _ = m.serve(pk, sid=sid, wslot=slot, ordered=True,
                          passes=ORD_PASSES)
        assert all(r['err'] != 'SYSTEM_ERROR' for r in reps)
        assert srv.order_stats()[0] == want_max
    assert set(m.kinds) == {'CREATED', 'DELETED', 'DATA_CHANGED', CC}, m.kinds
    assert m.kinds[CC] > 20 and m.events > 300, (m.kinds, m.events)


# ---- 3. table geometry ------------------------------------------------------

WCAP = 32               # GpuTree(watch_cap=32): a watch table of 64 entries
WHCAP = 64
WFMT = '/bench/d000000/w%07d'


def test_watch_window_names():
    names = window_names(48, WHCAP, fmt=WFMT)
    assert len(set(names)) == 48
    for p in names:
        s = home_slot(p, WHCAP)
        assert s >= WHCAP - 8 or s < 8


@pytest.mark.gpu
def test_watch_table_geometry(gpu):
    """36 watched names whose home entries are the last 8 and the first 8 of
    a 64-entry watch table: the chains crowd the table's end and wrap to
    its start.  Arm, fire, re-arm and resume over them from three slots,
    with writes to 12 never-watched names whose probes pass through the
    crowd; the table stays below full and nothing is lost."""
    m = _model(gpu, watch_cap=WCAP)
    assert m.tree.watch_hcap == WHCAP
    names = window_names(48, WHCAP, fmt=WFMT)
    W, U = list(names[:36]), list(names[36:])
    s0, s31, s63 = m.session(0), m.session(31), m.session(63)
    wr = m.session()
    m.serve([wexists(p) for p in W[:24]], sid=s0, wslot=0)
    m.serve([wexists(p) for p in W[12:]], sid=s31, wslot=31)
    assert m.tree.watch_census()[:2] == (36, 36)
    _, want = m.serve([create(p, b'1') for p in W[::2]] +
                      [create(p, b'u') for p in U[:6]], sid=wr)
    assert len(want) == 12 + 12                     # CREATED, both slots
    assert m.tree.watch_census()[:2] == (36, 18)
    # re-arm: data watches on the created half, exist watches on all, child
    # watches (lists) on a few
    m.serve([wget(p) for p in W[::2]], sid=s63, wslot=63)
    m.serve([wexists(p) for p in W], sid=s0, wslot=0)
    m.serve([ls(p) for p in W[:12:2]], sid=s31, wslot=31, how='list')
    rel = m.mark()
    _, want = m.serve([set_data(p, b'2') for p in W[:18:2]] +
                      [delete(p) for p in W[18::2]] +
                      [create(p, b'3') for p in W[1::2]] +
                      [set_data(p, b'u2') for p in U[:3]] +
                      [delete(p) for p in U[3:6]] +
                      [create(p, b'u3') for p in U[6:]], sid=wr)
    # (slot 31's first exist watches on the odd names were still armed)
    assert collections.Counter(t for _, _, t, _ in want) == {
        'DATA_CHANGED': 18, 'DELETED': 18, 'CREATED': 18 + 12}
    # resume slot 31 over the crowd with the zxid from before those writes
    m.serve([set_watches(rel, data=W[:18], exist=W[18:],
                         child=W[:12:2] + W[1::6])], sid=s31, wslot=31)
    _, want = m.serve([set_data(p, b'4') for p in W[1:18:2]] +
                      [create(p, b'5') for p in W[18::2]] +
                      [delete(p) for p in W[:12:2]] +
                      [set_data(p, b'u4') for p in U[6:]], sid=wr)
    assert want
    used, held, lost = m.tree.watch_census()
    assert used == 36 and lost == 0


# ---- 4. hash twins ----------------------------------------------------------

@pytest.mark.gpu
def test_hash_twins_keep_their_watches(gpu):
    """Paths of one 64-bit key (tests/treemodel.py hash_twin) are two paths
    to the watch table: a write to the twin of a watched path tells nobody,
    the write to the path itself its watcher; likewise an exist watch while
    the twin is created, and a SET_WATCHES re-arm."""
    m = _model(gpu)
    d0 = dirp(0)
    a = d0 + '/' + 'T' * 41                          # 56 bytes
    b = hash_twin(a, 5)
    a2 = d0 + '/' + 'S' * 25                         # 40 bytes
    b2 = hash_twin(a2, 3)
    s0, s1 = m.session(0), m.session(1)
    wr = m.session()
    m.serve([create(a, b'a')], sid=wr)
    m.serve([create(b, b'b')], sid=wr)
    # slot 0 watches A; the writer sets the twin, then A
    m.serve([wget(a)], sid=s0, wslot=0)
    _, want = m.serve([set_data(b, b'b1')], sid=wr)
    assert want == []
    _, want = m.serve([set_data(a, b'a1')], sid=wr)
    assert [e[1:] for e in want] == [(0, 'DATA_CHANGED', a)]
    # both watched, by one batch and by two sessions; both written
    m.serve([wget(a), wget(b)], sid=s0, wslot=0)
    m.serve([wget(b)], sid=s1, wslot=1)
    _, want = m.serve([set_data(a, b'a2')], sid=wr)
    assert [e[1:] for e in want] == [(0, 'DATA_CHANGED', a)]
    _, want = m.serve([set_data(b, b'b2')], sid=wr)
    assert sorted(e[1:] for e in want) == [(0, 'DATA_CHANGED', b),
                                           (1, 'DATA_CHANGED', b)]
    # an exist watch on a missing path while its twin is created
    m.serve([wexists(a2)], sid=s0, wslot=0)
    _, want = m.serve([create(b2, b'x')], sid=wr)
    assert [e for e in want if e[2] == 'CREATED'] == []
    _, want = m.serve([create(a2, b'x')], sid=wr)
    assert [e[1:] for e in want] == [(0, 'CREATED', a2)]
    # a SET_WATCHES re-arm of A, then a write to B, then to A
    rel = m.mark()
    m.serve([set_watches(rel, data=[a], exist=[])], sid=s0, wslot=0)
    _, want = m.serve([set_data(b, b'b3')], sid=wr)
    assert want == []
    _, want = m.serve([delete(a)], sid=wr)
    assert [e[1:] for e in want] == [(0, 'DELETED', a)]


# ---- 5. a full table --------------------------------------------------------

@pytest.mark.gpu
def test_full_watch_table(gpu):
    """Watches on more distinct paths than the 64-entry table has entries,
    in one batch and across batches: every reply as the model's, exactly the
    arms that found no entry counted in watch_stats()['lost_arms'], every
    other watch fires exactly once, a write to an unwatched path still
    answers, and watch_rehash() makes room again."""
    m = _model(gpu, watch_cap=WCAP)
    t, srv = m.tree, m.srv
    s0, s1 = m.session(0), m.session(63)
    wr = m.session()
    first = [leaf(k) for k in range(100)]
    # one batch: 100 arms for 64 entries
    m.serve([wget(p) for p in first], sid=s0, wslot=0, lost_ok=True)
    used, held, lost = t.watch_census()
    assert (used, held, lost) == (WHCAP, WHCAP, 100 - WHCAP)
    assert srv.watch_stats()['lost_arms'] == 100 - WHCAP
    # across batches: 20 new paths find nothing; arms on entered paths do
    key = {k & ((1 << 64) - 1)
           for k in t.watch[0][0:2 * WHCAP:2].cpu().tolist()}
    entered = [p for p in first if _lib.acl_hash(p.encode()) in key]
    assert len(entered) == WHCAP
    more = [leaf(k) for k in range(100, 120)]
    m.serve([wexists(p) for p in more] + [wget(p) for p in first[:50]],
            sid=s1, wslot=63, lost_ok=True)
    lost2 = t.watch_census()[2]
    armed1 = [p for p in first[:50] if p in entered]
    assert lost2 - lost == 20 + 50 - len(armed1)
    # an unwatched path on the full table
    reps, want = m.serve([set_data(leaf(500), b'q'),
                          wget(leaf(501), False)], sid=wr, lost_ok=True)
    assert [r['err'] for r in reps] == ['OK', 'OK'] and want == []
    # fire everything: the model sends 100 + 20 + 50 events, the GPU those
    # whose arm found an entry, once each
    _, want = m.serve([set_data(p, b'w') for p in first + more], sid=wr,
                      lost_ok=True, missing=lost2)
    assert len(want) == 100 + 20 + 50
    sent = m.last_sent
    assert sorted(sent) == [0, 63]
    assert sorted(sent[0]) == sorted(('DATA_CHANGED', p) for p in entered)
    assert sorted(sent[63]) == sorted(('DATA_CHANGED', p) for p in armed1)
    assert t.watch_census() == (WHCAP, 0, lost2)
    # the remedy: a rebuild keeps the entries with a watch — none here
    t.watch_rehash()
    assert t.watch_census() == (0, 0, lost2)
    m.serve([wget(p) for p in first[:40]], sid=s0, wslot=0, lost_ok=True)
    assert t.watch_census() == (40, 40, lost2)
    # a rebuild with watches held: they survive it and fire
    t.watch_rehash(watch_cap=64)
    assert t.watch_hcap == 128 and t.watch_census() == (40, 40, lost2)
    _, want = m.serve([set_data(p, b'z') for p in first[:40]], sid=wr,
                      lost_ok=True)
    assert len(want) == 40


# ---- 6. event overflow ------------------------------------------------------

@pytest.mark.gpu
def test_event_overflow_is_reported(gpu):
    """All 64 slots watch the same 64 leaves and one batch sets them all:
    4096 events for room for ``ecap``.  The written ones are the model's
    first ``ecap`` (whole requests: ecap is a multiple of 64), ev_total and
    watch_stats() say how many were fired and written, and the next batch's
    notifications are exact again."""
    m = _model(gpu)
    srv = m.srv
    assert srv.ecap == 3 * 1024 + 64 and srv.ecap % 64 == 0
    paths = [leaf(k) for k in range(64)]
    sids = [m.session(s) for s in range(64)]
    wr = m.session()
    for s in range(64):
        m.serve([wget(p) for p in paths], sid=sids[s], wslot=s, audit=False)
    # (serve compares ev_total and watch_stats() with [ecap, 4096])
    _, want = m.serve([set_data(p, b'all') for p in paths], sid=wr,
                      overflow=True)
    assert len(want) == srv.ecap
    # the watches are spent on both sides; the next batches are exact
    m.serve([wget(p) for p in paths[:10]], sid=sids[5], wslot=5)
    _, want = m.serve([set_data(p, b'next') for p in paths], sid=wr)
    assert len(want) == 10


# ---- 7. SET_WATCHES at size -------------------------------------------------

class _Resume(object):
    """The three lists of one SET_WATCHES of ``n`` paths with every branch
    of the catch-up in them, the writes that make them so, and the writes
    that fire what was re-armed.  Case ``c`` has names and leaves of its
    own, so the cases of one tree do not meet."""

    def __init__(self, c, n, gone0):
        # seven lists of q paths, the 18 directories, the rest unchanged
        q = (n - 18) // 7 if n >= 64 else 0
        nd = 18 if q else 0
        rest = n - nd - 7 * q
        tag = 'z%d' % c
        # leaves of directories 0..8 are deleted, of 9..19 set
        assert gone0 + q <= 9 * FANOUT
        self.deleted = [leaf(k) for k in range(gone0, gone0 + q)]
        keep = [leaf(k) for k in range(9 * FANOUT, NLEAF)]
        assert 2 * q + rest <= len(keep)
        self.changed = keep[:q]
        self.same = keep[q:2 * q + rest]
        self.born = ['%s/%sb%d' % (dirp(j % 8), tag, j) for j in range(q)]
        self.never = ['%s/%sn%d' % (dirp(j % 8), tag, j) for j in range(q)]
        self.exist = keep[:q]                   # an exist watch on a node
        touched = [dirp(d) for d in range(8)] if q else []
        calm = [dirp(d) for d in range(10, NDIR)] if q else []
        self.data = self.changed + self.deleted + self.same
        self.exists = self.born + self.never + self.exist
        self.child = touched + calm + self.deleted
        self.calm = calm
        assert len(self.data) + len(self.exists) + len(self.child) == n, \
            (n, len(self.data), len(self.exists), len(self.child))

    def before(self):
        return [set_data(p, b'chg') for p in self.changed] + \
            [delete(p) for p in self.deleted] + \
            [create(p, b'born') for p in self.born]

    def frame(self, rel):
        return set_watches(rel, self.data, self.exists, self.child)

    def after(self, c):
        return [set_data(p, b'fire') for p in self.same] + \
            [create(p, b'late') for p in self.never] + \
            [create('%s/z%dfire' % (d, c), b'') for d in self.calm]


def _chunks(pk, n):
    return [pk[o:o + n] for o in range(0, len(pk), n)]


def _resume_case(m, c, n, slot, sid, wr, gone0, split=False):
    r = _Resume(c, n, gone0)
    rel = m.mark()
    cap = m.srv.cap_frames
    for part in _chunks(r.before(), cap):
        m.serve(part, sid=wr, audit=False)
    if split:
        # two SET_WATCHES frames in one batch
        h = len(r.data) // 2
        pk = [set_watches(rel, r.data[:h], r.exists, ()),
              set_watches(rel, r.data[h:], (), r.child)]
    else:
        pk = [r.frame(rel)]
    m.serve(pk, sid=sid, wslot=slot)
    res = m.srv.resume_notif[2].cpu().tolist()
    # every re-armed watch fires on the writes that follow
    fired = 0
    parts = _chunks(r.after(c), cap)
    for k, part in enumerate(parts):
        _, want = m.serve(part, sid=wr, audit=k == len(parts) - 1)
        fired += len([e for e in want if e[1] == slot])
    assert fired == res[1], (fired, res)
    return r, res


@pytest.mark.gpu
@pytest.mark.parametrize('frames', [1024, 256])
def test_set_watches_at_size(gpu, frames):
    """One SET_WATCHES frame of 1, 1023, 1024, 1025 and 3000 paths (the
    256-frame server: 3000 only, past the 3 * 256 + 64 its event buffers
    hold) over the three lists with every branch of the catch-up: changed,
    deleted, unchanged; created, still missing, existing; children changed,
    unchanged, parent deleted.  Then two frames in one batch and one frame
    among ordinary requests.  Events in request order as
    fakezk.set_watches sends them, the re-arm count the model's, and every
    re-armed watch fires on the writes that follow."""
    m = _model(gpu, frames=frames, watch_cap=8192)
    wr = m.session()
    sizes = [1, 1023, 1024, 1025, 3000] if frames == 1024 else [3000]
    gone0 = 0
    seen = collections.Counter()
    for c, n in enumerate(sizes):
        slot = (0, 31, 32, 63, 17)[c]
        sid = m.session(slot)
        before = collections.Counter(m.kinds)
        r, res = _resume_case(m, c, n, slot, sid, wr, gone0)
        gone0 += len(r.deleted)
        assert res[0] == res[2] and res[3] == 0
        if n >= 1023:
            got = m.kinds - before
            assert set(got) == {'CREATED', 'DELETED', 'DATA_CHANGED', CC}
            assert res[1] > n // 4 and len(r.born) > 100
    # two frames in one batch
    sid = m.session(5)
    r, res = _resume_case(m, 7, 203, 5, sid, wr, gone0, split=True)
    gone0 += len(r.deleted)
    # a frame among ordinary requests (other paths): a watched read before
    # it, a write after it
    rel = m.mark()
    m.serve([set_data(leaf(1990), b'new')], sid=wr, audit=False)
    pk = [wget(leaf(1995)),
          set_watches(rel, [leaf(1990), leaf(1991)],
                      ['/bench/d000019/nope'], [dirp(19)]),
          set_data(leaf(1996), b'y')]
    m.serve(pk, sid=sid, wslot=5)
    res = m.srv.resume_notif[2].cpu().tolist()
    assert res[:3] == [1, 3, 1]
    _, want = m.serve([set_data(leaf(1995), b'1'), set_data(leaf(1991), b'2'),
                       create('/bench/d000019/nope', b'3')], sid=wr)
    assert sorted(e[2:] for e in want if e[1] == 5) == sorted([
        ('CREATED', '/bench/d000019/nope'), (CC, dirp(19)),
        ('DATA_CHANGED', leaf(1991)), ('DATA_CHANGED', leaf(1995))])
    assert m.stats()['lost_arms'] == 0


# ---- 8. expiry with watchers ------------------------------------------------

@pytest.mark.gpu
def test_expiry_with_watchers(gpu):
    """Sessions A and B own ephemerals under a shared and under separate
    parents; two watchers and A itself hold data, exist and child watches
    on them and child watches on the parents.  A expires: the watchers are
    told as if each ephemeral were deleted (one txn), A nothing; its own
    watches are gone — a re-created name, a write to a path only A watched,
    and a new session on A's slot all find nothing of A's left."""
    m = _model(gpu)
    p1, p2, p3 = dirp(0), dirp(1), dirp(2)
    a, b = m.session(0), m.session(31)
    w1, w2 = m.session(32), m.session(63)
    wr = m.session()
    ea = ['%s/ea%d' % (p1, k) for k in range(5)] + \
        ['%s/ea%d' % (p2, k) for k in range(5, 10)]
    eb = ['%s/eb%d' % (p1, k) for k in range(5)] + \
        ['%s/eb%d' % (p3, k) for k in range(5, 10)]
    tmp = p1 + '/eatmp'
    m.serve([create(p, b'a', ['EPHEMERAL']) for p in ea + [tmp]], sid=a,
            wslot=0)
    m.serve([create(p, b'b', ['EPHEMERAL']) for p in eb], sid=b, wslot=31)
    m.serve([delete(tmp)], sid=a, wslot=0)
    only_a = leaf(777)
    # watcher 1: data watches on both owners' nodes, a child watch on one of
    # A's too (told once), child watches on the parents
    m.serve([wget(p) for p in ea[:8] + eb[:3]] +
            [ls(ea[0]), ls(ea[9]), ls(p1), ls(p2), ls(p3)], sid=w1, wslot=32,
            how='mixed')
    # watcher 2: exist watches on live and on the deleted name, the shared
    # parent
    m.serve([wexists(p) for p in ea[5:] + [tmp] + eb[5:8]] + [ls(p1)],
            sid=w2, wslot=63, how='mixed')
    # B watches A's; A watches B's, its own, a leaf nobody else does, and
    # B's parent
    m.serve([wget(ea[1]), ls(p2)], sid=b, wslot=31, how='mixed')
    m.serve([wget(eb[0]), wget(ea[1]), wexists(tmp), wget(only_a), ls(p3),
             ls(p1)], sid=a, wslot=0, how='mixed')
    removed, want = m.expire(a)
    assert removed == 10
    by = collections.Counter((s, t) for _, s, t, _ in want)
    assert by == {(32, 'DELETED'): 9, (32, CC): 2, (63, 'DELETED'): 5,
                  (63, CC): 1, (31, 'DELETED'): 1, (31, CC): 1}, by
    # one of its names again, and the name it deleted itself: only watcher
    # 2's exist watch on the latter is left
    _, want = m.serve([create(ea[0], b'again'), create(tmp, b'again')],
                      sid=wr)
    assert [e[1:] for e in want] == [(63, 'CREATED', tmp)]
    # a path only A watched
    _, want = m.serve([set_data(only_a, b'w')], sid=wr)
    assert want == []
    # a new session on A's slot hears nothing of what A watched
    c = m.session(0)
    _, want = m.serve([set_data(eb[0], b'w2'), delete(eb[9])], sid=wr)
    assert sorted(e[1:] for e in want) == [(32, CC, p3),
                                           (32, 'DATA_CHANGED', eb[0])]
    # ... and its own watches work; B expires with C watching
    m.serve([wget(eb[1]), wexists(eb[5]), ls(p3), ls(p1)], sid=c, wslot=0,
            how='mixed')
    removed, want = m.expire(b)
    assert removed == 9
    assert sorted(e[1:] for e in want if e[1] == 0) == [
        (0, CC, p1), (0, CC, p3), (0, 'DELETED', eb[1]),
        (0, 'DELETED', eb[5])]
    assert m.stats()['lost_arms'] == 0
