"""Model-checked churn of the HBM tree's index and node recycling
(csrc/kernels/zk_tree.h, tree.hip, tree_order.hip): long mixed histories
over names chosen to crowd one 16-entry window at the end of the hash table,
each batch compared reply by reply with the fake server's database and
followed by an audit (tests/treemodel.py) that reads every live znode back
with its bytes and Stat, every dead path as NO_NODE, and checks the digest's
counts, the lists of the parents written under and the free ring.  All
comparisons are exact."""

import random

import pytest

from treemodel import (TreeModel, create, delete, exists, get, hash_twin,
                       home_slot, host_ranks, set_data, window_names)

from zkmi.ops import _lib

D0 = '/bench/d000000'
HCAP = 4096
WIN = 400               # windowed names, one scan shared by the tests


def _tree(gpu, cap_frames=1024, **kw):
    """The smallest tree: 12 static nodes, 1024 spare, 4096 index entries."""
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(10, 16, fanout=10, device=gpu, spare=0.0, **kw)
    # (the names below are chosen for this table size)
    assert (tree.cap, tree.hcap) == (1036, HCAP)
    srv = GpuServer(tree, cap_frames, 1 << 20)
    return TreeModel(tree, srv, gpu)


def _data(rng, hi=100):
    return bytes(rng.getrandbits(8) for _ in range(rng.randint(0, hi)))


# ---- host-only: the rank rule -----------------------------------------------

def test_host_ranks_rule():
    """The host mirror of tree_order.hip's ranks on the batches whose
    largest rank the GPU tests assert: create -> set -> get -> delete of one
    path is 3 (test_chain_pipeline_steps), ten sets of one path 9, reads of
    one path and SEQUENTIAL creates under one parent 0."""
    p = D0 + '/x'
    chain = [create(p), set_data(p, b'1'), get(p), delete(p)]
    assert host_ranks(chain) == [0, 1, 2, 3]
    # many chains under one parent: children of one parent commute
    many = [op for k in range(5) for op in
            [create('%s/y%d' % (D0, k))]] + \
        [set_data('%s/y%d' % (D0, k), b'') for k in range(5)] + \
        [delete('%s/y%d' % (D0, k)) for k in range(5)]
    assert max(host_ranks(many)) == 2
    assert host_ranks([set_data(p, b'', k) for k in range(10)]) == \
        list(range(10))
    ro = [get(p)] * 50 + [create(D0 + '/s-', b'', ['SEQUENTIAL'])] * 50
    assert max(host_ranks(ro)) == 0
    # a parent's read between its children's writes, a child before its
    # parent: C-A and A-C edges, none between the two children
    x, y, z = D0 + '/x', D0 + '/x/y', D0 + '/x/z'
    assert host_ranks([create(y), exists(x), create(z), create(x),
                       delete(y), get(x)]) == [0, 1, 2, 3, 4, 5]
    assert host_ranks([create(y), create(z), exists(x), delete(y),
                       delete(z)]) == [0, 0, 1, 2, 2]
    # a SEQUENTIAL create is no member of its own name's group
    s = create(x + '/s-', b'', ['SEQUENTIAL'])
    assert host_ranks([s, s, exists(x), s, get(x + '/s-')]) == \
        [0, 0, 1, 2, 0]


def test_window_names_and_twins():
    """The chosen names' home slots lie in the window; a hash twin has the
    same key and differs in the two words asked for only."""
    names = window_names(40, HCAP)
    assert len(set(names)) == 40
    for p in names:
        s = home_slot(p, HCAP)
        assert s >= HCAP - 8 or s < 8
    a = D0 + '/' + 'T' * 41                       # 56 bytes
    b = hash_twin(a, 5)
    assert a != b and len(a) == len(b) and a[:40] == b[:40]
    assert _lib.acl_hash(a.encode()) == _lib.acl_hash(b.encode())
    c = hash_twin(a, 3)
    assert c[:24] == a[:24] and c[24:40] != a[24:40] and c[40:] == a[40:]


# ---- 1. unordered churn -----------------------------------------------------

class _Churn(object):
    """Random batches that keep the unordered serve's batch contract: a
    path is written by at most one request and then not read; no request
    names the parent of a node the batch creates or deletes; a parent given
    SEQUENTIAL creates gets no other child write."""

    def __init__(self, m, rng):
        self.m, self.rng = m, rng
        self.win = list(window_names(WIN, HCAP)[:300])
        self.par = ['/bench/p/p%d' % k for k in range(8)]
        self.kids = {p: ['%s/k%d' % (p, j) for j in range(3)]
                     for p in self.par}
        self.eph = ['/bench/e/e%d' % k for k in range(6)]
        self.long = ['/bench/l/' + 'L' * (n - 9) for n in
                     (39, 40, 41, 47, 48, 49, 120)]
        self.static = ['%s/n%09d' % (D0, k) for k in range(10)]
        self.seq = []           # SEQUENTIAL names made so far

    def setup(self):
        """Two batches: the directories, then some of the parents."""
        return [[create('/bench/' + d) for d in 'pels'] +
                [create('/bench/nil')], [create(p) for p in self.par[:5]]]

    def _write(self, path, sid, eph_only=False):
        """One write of ``path``, right for its state or wrong on purpose."""
        rng, db = self.rng, self.m.db
        node = db.nodes.get(path)
        if node is None:
            fl = ['EPHEMERAL'] if eph_only or rng.random() < 0.4 else []
            r = rng.random()
            if r < 0.85:
                return create(path, _data(rng), fl)
            if r < 0.93:
                return set_data(path, b'lost')           # NO_NODE
            return delete(path)                          # NO_NODE
        ver = node.stat.version
        r = rng.random()
        if r < 0.30:
            return set_data(path, _data(rng, 128), rng.choice([ver, -1]))
        if r < 0.40:
            return set_data(path, b'stale', ver + 1 + rng.randint(0, 2))
        if r < 0.75:
            return delete(path, rng.choice([ver, -1]))
        if r < 0.85:
            return delete(path, ver + 1)                 # BAD_VERSION
        return create(path, b'twice')                    # NODE_EXISTS

    def batch(self, n, sid, tail_creates=False):
        rng, db = self.rng, self.m.db
        wr = []
        # windowed names, the long ones and the static leaves: one role each
        pool = self.win + self.long + self.static
        rng.shuffle(pool)
        nw = min(len(pool) * 3 // 5, max(1, n * 2 // 5))
        for path in pool[:nw]:
            wr.append(self._write(path, sid))
        readable = pool[nw:]
        # parents with kids: the parent's turn or its kids' (a kid's write
        # and a request on its parent conflict)
        for p in self.par:
            if rng.random() < 0.5:
                node = db.nodes.get(p)
                if node is not None and node.children:
                    # NOT_EMPTY; with a stale version BAD_VERSION (the
                    # version is checked first, as ZooKeeper does)
                    ver = node.stat.version
                    wr.append(delete(p, rng.choice([-1, ver, ver + 1])))
                else:
                    wr.append(self._write(p, sid))
            else:
                for k in self.kids[p]:                   # NO_NODE if p is
                    if rng.random() < 0.6:               # missing
                        wr.append(self._write(k, sid))
                    else:
                        readable.append(k)
        for e in self.eph:
            if rng.random() < 0.5:
                wr.append(self._write(e, sid, eph_only=True))
            else:                       # NO_CHILDREN_FOR_EPHEMERALS / NO_NODE
                wr.append(create(e + '/x'))
        wr.append(create('/bench/nil/gone/x'))           # NO_NODE
        # /bench/s: SEQUENTIAL creates, or the turn of the names made so far
        if rng.random() < 0.5 and len(self.seq) < 40:
            for _ in range(rng.randint(1, 6)):
                fl = ['SEQUENTIAL'] + (['EPHEMERAL'] if rng.random() < 0.5
                                       else [])
                wr.append(create('/bench/s/q-', _data(rng, 20), fl))
        else:
            for s in self.seq:
                if rng.random() < 0.5:
                    wr.append(self._write(s, sid))
                else:
                    readable.append(s)
        rng.shuffle(wr)
        wr = wr[:max(1, n * 2 // 5)] if n > 1 else wr[:1]
        # a truncated write list may leave a written path readable: drop them
        written = {p['path'] for p in wr}
        cpar = {p['path'][:p['path'].rfind('/')] for p in wr
                if p['opcode'] in ('CREATE', 'DELETE')}
        readable = [p for p in readable
                    if p not in written and p not in cpar]
        pk = list(wr)
        while len(pk) < n:
            path = rng.choice(readable)
            pk.append(get(path) if rng.random() < 0.5 else exists(path))
        if n == 1:
            pk = pk[:1]
        rng.shuffle(pk)
        if tail_creates:
            # the only creates of the batch in its last, partial wave
            room = n - 64 * ((n - 1) // 64)
            cr = [p for p in pk if p['opcode'] == 'CREATE'][:room]
            rest = [p for p in pk if p['opcode'] != 'CREATE']
            fill = [get(rng.choice(readable))
                    for _ in range(n - len(cr) - len(rest))]
            pk = rest + fill + cr
            assert all(p['opcode'] != 'CREATE' for p in pk[:n - room])
            assert cr and len(pk) == n
        return pk

    def after(self, pk, reps):
        for p, r in zip(pk, reps):
            if r['err'] == 'OK' and p['opcode'] == 'CREATE' and \
                    'SEQUENTIAL' in p['flags']:
                self.seq.append(r['path'])


@pytest.mark.gpu
def test_unordered_churn(gpu):
    """30 generations of contract-keeping batches of 1, 63, 64, 65, 255,
    256, 257 and 1000 requests over 300 windowed names and ~70 of other
    shapes (parents with children, EPHEMERAL parents, SEQUENTIAL names,
    paths of 39..120 bytes, the static leaves), under two sessions: every
    reply and, after every batch, every znode as the model has it."""
    m = _tree(gpu)
    rng = random.Random(11)
    ch = _Churn(m, rng)
    sids = [m.session(), m.session()]
    for pk in ch.setup():
        m.serve(pk)
    sizes = [1, 63, 64, 65, 255, 256, 257, 1000]
    errs = {}
    for g in range(30):
        n = sizes[g % len(sizes)]
        pk = ch.batch(n, sids[g % 2], tail_creates=8 <= g < 16 and n > 1)
        assert len(pk) == n
        reps, _ = m.serve(pk, sid=sids[g % 2])
        ch.after(pk, reps)
        for p, r in zip(pk, reps):
            k = (p['opcode'], r['err'])
            errs[k] = errs.get(k, 0) + 1
    # the history met every case it is meant to
    for k in [('CREATE', 'OK'), ('CREATE', 'NODE_EXISTS'),
              ('CREATE', 'NO_NODE'),
              ('CREATE', 'NO_CHILDREN_FOR_EPHEMERALS'),
              ('SET_DATA', 'OK'), ('SET_DATA', 'BAD_VERSION'),
              ('SET_DATA', 'NO_NODE'), ('DELETE', 'OK'),
              ('DELETE', 'BAD_VERSION'), ('DELETE', 'NOT_EMPTY'),
              ('DELETE', 'NO_NODE'), ('GET_DATA', 'OK'),
              ('GET_DATA', 'NO_NODE'), ('EXISTS', 'OK'),
              ('EXISTS', 'NO_NODE')]:
        assert errs.get(k, 0) > 0, (k, errs)
    assert len(m.dead) > 50 and ch.seq


# ---- 2. storage edges -------------------------------------------------------

def _names(n):
    """Two paths of ``n`` bytes that differ in their last byte only."""
    stem = D0 + '/' + ('%03d' % n) + 'x' * (n - len(D0) - 5)
    return stem + 'a', stem + 'b'


@pytest.mark.gpu
def test_storage_edges(gpu):
    """Paths of 39 .. 120 bytes around the 40 bytes a hash entry holds, in
    pairs that differ in the last byte, in the first byte past the entry's
    40, and pairs of EQUAL hash key that differ only inside / only past the
    40 bytes (told apart by ent_is alone); recycled nodes re-created with
    longer and with shorter paths and data (phase A's new_path / new_slot:
    the arena tops move by exactly the storage that no longer fits); data
    of 0 .. 300 bytes; SET_DATA to 0 bytes, to the slot's capacity, and one
    byte past it — BAD_ARGUMENTS, the tree's documented divergence from
    ZooKeeper."""
    m = _tree(gpu)
    t = m.tree
    pairs = [_names(n) for n in (39, 40, 41, 47, 48, 49, 120)]
    for n in (48, 49, 120):                 # differ at byte 40 only
        a = _names(n)[0]
        pairs.append((a[:40] + 'Y' + a[41:], a[:40] + 'Z' + a[41:]))
    base = D0 + '/' + 'T' * 41              # 56 bytes
    pairs.append((base, hash_twin(base, 5)))         # same key, tails differ
    pairs.append((base[:-1] + 'U', hash_twin(base[:-1] + 'U', 3)))  # heads
    short = D0 + '/' + 'S' * 25             # 40 bytes: whole in the entry
    pairs.append((short, hash_twin(short, 3)))
    long = D0 + '/' + 'W' * 105             # 120 bytes
    pairs.append((long, hash_twin(long, 12)))
    for a, b in pairs:
        assert len(a) == len(b) and a != b
    sizes = [0, 1, 127, 128, 129, 300]
    rng = random.Random(3)
    # a pair's two names in two batches: names of one hash key in one
    # batch are one path to the batch contract (the later insert waits for
    # the earlier one's entry and gives up: SYSTEM_ERROR)
    for side in (0, 1):
        pk = [create(pr[side], bytes(rng.getrandbits(8) for _ in
                                     range(sizes[(k + 3 * side) % 6])))
              for k, pr in enumerate(pairs)]
        reps, _ = m.serve(pk)
        assert all(r['err'] == 'OK' for r in reps)
    # one of each pair goes; its twin stays reachable, it does not
    reps, _ = m.serve([delete(a) for a, _ in pairs])
    assert all(r['err'] == 'OK' for r in reps)
    # (the audit read the dead name of each pair and its live twin.)  A
    # create of the live twin is NODE_EXISTS — also where the dead name left
    # a tombstone of the SAME key earlier in the chain: the insert may take
    # it only once the chain ended without the path — beside sets of others
    reps, _ = m.serve([create(b) for _, b in pairs[::2]] +
                      [set_data(b, b'kept') for _, b in pairs[1::2]])
    assert [r['err'] for r in reps] == \
        ['NODE_EXISTS'] * len(pairs[::2]) + ['OK'] * len(pairs[1::2])

    # recycled nodes: creates pop the ring in request order (one workgroup)
    def recreate(paths, datas):
        nt = m.audit()
        c = nt['counters']
        head, pub = c[_lib.TC_FREE_HEAD], c[_lib.TC_FREE_PUB]
        assert pub - head >= len(paths)
        ring = t.free_list.cpu().tolist()
        pcap = t.node_path_cap.cpu().tolist()
        scap = t.slot_cap.cpu().tolist()
        dp = ds = 0
        taken = []
        for k, (p, d) in enumerate(zip(paths, datas)):
            v = ring[(head + k) % t.cap]
            new_path = len(p) > pcap[v]
            new_slot = max(len(d), 128) > scap[v]
            taken.append((new_path, new_slot))
            dp += ((len(p) + 15) & ~15) if new_path else 0
            ds += (76 + ((max(len(d), 128) + 15) & ~15) + 4) if new_slot \
                else 0
        reps, _ = m.serve([create(p, d) for p, d in zip(paths, datas)])
        assert all(r['err'] == 'OK' for r in reps)
        c2 = t.counters.cpu().tolist()
        assert c2[_lib.TC_PATH_TOP] - c[_lib.TC_PATH_TOP] == dp
        assert c2[_lib.TC_SLAB_TOP] - c[_lib.TC_SLAB_TOP] == ds
        assert c2[_lib.TC_NODES] == c[_lib.TC_NODES]        # all recycled
        for p, d in zip(paths, datas):
            v = m.node_of[p]
            assert m.slot_cap[v] >= max(len(d), 128)
        return taken

    # the deleted names again, longest first: the ring holds their nodes in
    # deletion order (shortest first), so long paths land on short storage
    gone = sorted((a for a, _ in pairs), key=len, reverse=True)
    datas = [bytes([65 + k]) * s for k, s in
             enumerate([300, 0, 129, 1, 128, 127, 300, 0, 200, 5, 64, 140,
                        33, 77])]
    assert len(datas) == len(gone)
    taken = recreate(gone, datas)
    assert any(p for p, _ in taken) and any(not p for p, _ in taken)
    assert any(s for _, s in taken) and any(not s for _, s in taken)
    # delete all of them and re-create in ring order again, shortest first
    reps, _ = m.serve([delete(p) for p in gone])
    assert all(r['err'] == 'OK' for r in reps)
    taken = recreate(gone[::-1], [b'z'] * len(gone))
    assert any(p for p, _ in taken) and any(not p for p, _ in taken)
    assert not any(s for _, s in taken)       # a slot never shrinks

    # SET_DATA at the slot's capacity
    small, big = gone[0], gone[1]
    for p in (small, big, pairs[0][1]):
        cap = int(m.slot_cap[m.node_of[p]])
        assert cap >= 128
        ver = m.db.nodes[p].stat.version
        old = bytes(m.db.nodes[p].data)
        reps, _ = m.serve([set_data(p, b'\x5a' * (cap + 1), ver)])
        assert reps[0]['err'] == 'BAD_ARGUMENTS'
        assert m.db.nodes[p].stat.version == ver        # (audited: the same
        assert bytes(m.db.nodes[p].data) == old         # on the tree)
        reps, _ = m.serve([set_data(p, b'\xa5' * cap, ver)])
        assert reps[0]['err'] == 'OK' and reps[0]['stat'].dataLength == cap
        reps, _ = m.serve([set_data(p, b'', ver + 1)])
        assert reps[0]['err'] == 'OK' and reps[0]['stat'].dataLength == 0
        reps, _ = m.serve([set_data(p, b'\x5a' * (cap + 1), 99)])
        assert reps[0]['err'] == 'BAD_ARGUMENTS'        # before the version
    assert any(int(m.slot_cap[m.node_of[p]]) >= 300 for p in gone)


# ---- 3. expiry among strangers ----------------------------------------------

@pytest.mark.gpu
def test_expiry_among_strangers(gpu):
    """Three owners' names interleaved in one window of the index — session
    A's and B's ephemerals and persistent nodes, ~100 each — with plain
    DELETE tombstones from an earlier batch between them.  Expiring A, then
    B, then a session C created into the same window, moves other owners'
    entries back (ht_shift), meets the blocked cases and reclaims across
    the table's end; after each, every survivor is found and every removed
    name is gone.  A session that owns nothing removes nothing."""
    m = _tree(gpu)
    names = window_names(WIN, HCAP)
    a, b, c = m.session(), m.session(), m.session()
    own = names[:300]
    hole = names[300:350]
    later = names[350:400]
    # every batch creates its owner's names and a third of the
    # tombstones-to-be (plain nodes), interleaved
    order = []
    for k in range(50):
        order += list(own[6 * k:6 * k + 6]) + [hole[k]]
    turn = {p: k % 3 for k, p in enumerate(own)}
    turn.update({p: k % 3 for k, p in enumerate(hole)})
    for n, sid in enumerate((a, b, 0)):
        pk = [create(p, p[-3:].encode(),
                     ['EPHEMERAL'] if sid and p not in hole else [])
              for p in order if turn[p] == n]
        reps, _ = m.serve(pk, sid=sid)
        assert all(r['err'] == 'OK' for r in reps)
    reps, _ = m.serve([delete(p) for p in hole])
    assert all(r['err'] == 'OK' for r in reps)
    _, live, used, tomb = m.tree.digest()
    assert tomb == 50
    # a session without nodes
    d0 = m.tree.digest()
    assert m.expire(m.session()) == 0
    assert m.tree.digest() == d0
    assert m.expire(a) == 100
    reps, _ = m.serve([create(p, b'c', ['EPHEMERAL']) for p in later] +
                      [create(p, b'c2', ['EPHEMERAL']) for p in hole[:25]],
                      sid=c)
    assert all(r['err'] == 'OK' for r in reps)
    assert m.expire(b) == 100
    assert m.expire(c) == 75
    _, live, used, tomb = m.tree.digest()
    assert live == 12 + 100
    assert m.expire(c) == 0


# ---- 4. tombstone growth, a full index, rehash ------------------------------

@pytest.mark.gpu
def test_full_index_and_rehash(gpu):
    """Never-reused plain names leave a tombstone each; when the empty
    entries run out, exactly the creates that found none answer
    SYSTEM_ERROR (a new name is never NODE_EXISTS) and change nothing;
    rehash() drops the tombstones and the same names are created."""
    m = _tree(gpu)
    t = m.tree
    gen = 0
    while True:
        names = ['%s/g%dn%04d' % (D0, gen, k) for k in range(1000)]
        _, live, used, tomb = t.digest()
        empty = t.hcap - used
        assert tomb == 1000 * gen and live == 12
        pk = [create(p, b'%d' % gen) for p in names]
        if empty >= len(pk):
            reps, _ = m.serve(pk)
            assert all(r['err'] == 'OK' for r in reps)
            reps, _ = m.serve([delete(p) for p in names])
            assert all(r['err'] == 'OK' for r in reps)
            gen += 1
            continue
        # the generation the index fills up in: the model is told which
        # creates failed (the concurrent batch decides which), then audited
        assert gen == 4 and 0 < empty < len(pk)
        got = m.serve_full_index(pk)
        assert got.count('OK') == empty
        assert got.count('SYSTEM_ERROR') == len(pk) - empty
        break
    _, live, used, tomb = t.digest()
    assert used == t.hcap and live == 12 + empty
    made = [p for p, e in zip(names, got) if e == 'OK']
    reps, _ = m.serve([delete(p) for p in made])
    assert all(r['err'] == 'OK' for r in reps)
    # a full index of tombstones: a read of a missing name ends, NO_NODE
    reps, _ = m.serve([exists(names[0]), get(D0)])
    assert [r['err'] for r in reps] == ['NO_NODE', 'OK']
    t.rehash()
    _, live, used, tomb = t.digest()
    assert (live, used, tomb) == (12, 12, 0)
    m.audit()
    reps, _ = m.serve([create(p, b'again') for p in names])
    assert all(r['err'] == 'OK' for r in reps)


# ---- 5. ordered churn -------------------------------------------------------

def _ordered_pool():
    l1 = ['%s/a%d' % (D0, k) for k in range(10)]
    l2 = ['%s/b%d' % (p, k) for p in l1 for k in range(4)]
    l3 = ['%s/c%d' % (p, k) for p in l2[::2] for k in range(5)]
    return l1 + l2 + l3


def _ordered_batch(rng, pool, n):
    """Random requests with same-path and parent / child conflicts as they
    fall.  SEQUENTIAL creates go under /bench/q0 and /bench/q1, which get
    no other request: the numbering pass counts a parent's SEQUENTIAL
    creates of the whole batch at once (tree_seq.hip), so a read of the
    parent between them, or another child write, would not see ZooKeeper's
    one-by-one numbers."""
    pk = []
    for _ in range(n):
        path = rng.choice(pool)
        r = rng.random()
        if r < 0.06:
            pk.append(create('/bench/q%d/s-' % rng.randint(0, 1),
                             _data(rng, 30), ['SEQUENTIAL']))
        elif r < 0.30:
            pk.append(create(path, _data(rng)))
        elif r < 0.45:
            pk.append(set_data(path, _data(rng, 120),
                               rng.choice([-1, -1, 0, 1, 2])))
        elif r < 0.65:
            pk.append(delete(path, rng.choice([-1, -1, -1, 0, 1])))
        elif r < 0.85:
            pk.append(get(path))
        else:
            pk.append(exists(path))
    return pk


ORD_PASSES = 24
ORD_ROUNDS = 10
ORD_N = 500


def _ordered_rounds():
    rng = random.Random(5)
    pool = _ordered_pool()
    return [_ordered_batch(rng, pool, ORD_N) for _ in range(ORD_ROUNDS)]


def test_ordered_rounds_fit_the_passes():
    """The fixed seed's batches rank under the passes the GPU test uses, so
    none of its replies may be a refusal."""
    assert len(_ordered_pool()) == 150
    mx = [max(host_ranks(pk)) for pk in _ordered_rounds()]
    assert max(mx) < ORD_PASSES and min(mx) >= 8, mx


@pytest.mark.gpu
def test_ordered_churn(gpu):
    """10 rounds of 500 random requests over 150 paths in three levels,
    served in order (serve(ordered=True)): every reply as the fake server
    gives it applying the batch one by one — errors, created names, data,
    version, dataLength, numChildren and cversion; zxids are not compared
    here — then the audit with plain reads.  SEQUENTIAL creates have
    parents of their own (see _ordered_batch), so their names are compared
    in full.  The largest rank the ordering pass reports equals the host's
    (treemodel.host_ranks)."""
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(10, 16, fanout=10, device=gpu, spare=0.0,
                   scratch=1 << 20)
    srv = GpuServer(tree, 512, 1 << 20)
    m = TreeModel(tree, srv, gpu)
    m.serve([create('/bench/q0'), create('/bench/q1')])
    for pk in _ordered_rounds():
        want_max = max(host_ranks(pk))
        assert want_max < ORD_PASSES
        reps, _ = m.serve(pk, zxids=False, ordered=True, passes=ORD_PASSES)
        assert all(r['err'] != 'SYSTEM_ERROR' for r in reps)
        assert srv.order_stats()[0] == want_max
