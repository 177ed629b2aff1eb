"""zkmi.Client against zkmi.server.gpu.GpuZKServer: the real client state
machines over a socket to the HBM tree.  Where ZooKeeper's behaviour is the
yardstick the same script runs against FakeZKServer and the results must be
equal.  Every wait is bounded by 10 s; the server is shut down in the
fixture's teardown."""

import socket
import struct
import threading

import pytest

from zkmi import jute
from zkmi.errors import ZKError
from zkmi.server.fakezk import FakeZKServer

from zkhelpers import client, wait_for

pytestmark = pytest.mark.gpu

D0 = '/bench/d000000'
LEAF = D0 + '/n%09d'
STAT_FIELDS = ('version', 'cversion', 'aversion', 'dataLength', 'numChildren')


def _make(gpu, table=None, **kw):
    from zkmi.server.tree import GpuTree
    from zkmi.server.gpu import GpuZKServer
    tree = GpuTree(n_nodes=2000, fanout=100, watch_cap=4096, acl_cap=64,
                   device=gpu)
    tab = table(tree) if table is not None else None
    kw.setdefault('cap_frames', 1024)
    kw.setdefault('out_cap', 1 << 20)
    kw.setdefault('max_conns', 128)
    return GpuZKServer(tree, table=tab, **kw)


@pytest.fixture
def srv(gpu):
    s = _make(gpu)
    yield s
    s.shutdown()
    assert s.error is None, s.error


def _stat(st):
    return tuple(getattr(st, f) for f in STAT_FIELDS) + \
        (st.ephemeralOwner != 0,)


def _norm(v):
    if hasattr(v, 'ephemeralOwner'):
        return _stat(v)
    if isinstance(v, tuple):
        return tuple(_norm(x) for x in v)
    if isinstance(v, list):
        return sorted(v, key=repr)
    return v


def _call(c, method, *args):
    try:
        return _norm(c.call_sync(method, *args, timeout=10))
    except ZKError as e:
        return ('ERR', e.code)


# ---- 1. the client's surface ---------------------------------------------------

def _surface(c, data=None):
    """The script; returns [(label, result)] and the data of the 300 bulk
    paths (to preload the other server with)."""
    out = []

    def run(label, method, *args):
        out.append((label, _call(c, method, *args)))

    base = D0 + '/t'
    run('create', 'create', base, b'hello', {})
    run('create again', 'create', base, b'x', {})
    run('create eph', 'create', base + '/e', b'e', {'flags': ['EPHEMERAL']})
    run('create under eph', 'create', base + '/e/x', b'', {})
    run('create seq', 'create', base + '/s', b's', {'flags': ['SEQUENTIAL']})
    run('create seq 2', 'create', base + '/s', b's',
        {'flags': ['SEQUENTIAL', 'EPHEMERAL']})
    run('create orphan', 'create', D0 + '/no/such', b'', {})
    run('get', 'get', base)
    run('get missing', 'get', base + '/none')
    run('get eph', 'get', base + '/e')
    run('set', 'set', base, b'world!', 0)
    run('set bad version', 'set', base, b'nope', 7)
    run('set any', 'set', base, b'', -1)
    run('set missing', 'set', base + '/none', b'', -1)
    run('get after sets', 'get', base)
    run('stat', 'stat', base)
    run('stat missing', 'stat', base + '/none')
    run('stat dir', 'stat', D0)
    run('list', 'list', base)
    run('list dir', 'list', D0)
    run('list missing', 'list', base + '/none')
    run('getACL', 'getACL', base)
    run('getACL missing', 'getACL', base + '/none')
    run('delete not empty', 'delete', base, -1)
    run('delete bad version', 'delete', base + '/e', 3)
    run('delete', 'delete', base + '/e', 0)
    run('delete again', 'delete', base + '/e', -1)
    run('sync', 'sync', base)
    run('ping', 'ping')
    run('deep', 'createWithEmptyParents', D0 + '/p/q/r', b'deep', {})
    run('deep get', 'get', D0 + '/p/q/r')
    run('deep parent', 'get', D0 + '/p/q')
    paths = ['/bench/d%06d/n%09d' % (i // 100, i) for i in range(300)]
    res = c.call_sync('bulk_get', paths, timeout=10)
    pk = res.packets()
    assert res.ok_count() == 300
    got = [(p['data'], _stat(p['stat'])) for p in pk]
    out.append(('bulk_get', got))
    return out, dict(zip(paths, (g[0] for g in got)))


def test_client_surface(srv):
    c = client(srv.servers())
    c.wait_connected(10)
    got, data = _surface(c)
    c.close_sync(10)
    fake = FakeZKServer()
    try:
        fake.cli_create('/bench', b'')
        for d in range(3):
            fake.cli_create('/bench/d%06d' % d, b'')
        for p, v in data.items():
            fake.cli_create(p, v)
        f = client(fake.servers())
        f.wait_connected(10)
        want, _ = _surface(f)
        f.close_sync(10)
    finally:
        fake.shutdown()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
    by = dict(got[:-1])
    assert by['create'] == D0 + '/t' and by['set bad version'] == \
        ('ERR', 'BAD_VERSION')
    assert by['get after sets'][0] in (b'', None)
    assert by['delete not empty'] == ('ERR', 'NOT_EMPTY')
    st = srv.stats()
    assert st['batches_lost'] == 0 and st['bad_batches'] == 0
    assert st['max_reads_per_tick'] <= 2
    assert st['sessions'] == 0 and st['sessions_closed'] == 1


# ---- 2. pipelining ---------------------------------------------------------------

def test_pipelined_requests_take_effect_in_order(srv):
    c = client(srv.servers())
    c.wait_connected(10)
    for rep in range(50):
        p = D0 + '/pipe%03d' % rep
        got = [None] * 7
        done = threading.Event()
        left = [7]

        def cb(k):
            def f(err=None, *res):
                got[k] = ('ERR', err.code) if err is not None else _norm(res)
                left[0] -= 1
                if left[0] == 0:
                    done.set()
            return f

        def issue():
            c.create(p, b'0', {}, cb(0))
            c.set(p, b'1', -1, cb(1))
            c.get(p, cb(2))
            c.set(p, b'2', -1, cb(3))
            c.get(p, cb(4))
            c.delete(p, -1, cb(5))
            c.stat(p, cb(6))
        c.loop.run(issue)
        assert done.wait(10), (rep, got)
        assert got[0] == (p,) and got[1] == () and got[3] == () and \
            got[5] == (), (rep, got)
        assert got[2][0] == b'1' and got[2][1][0] == 1, (rep, got)
        assert got[4][0] == b'2' and got[4][1][0] == 2, (rep, got)
        assert got[6] == ('ERR', 'NO_NODE'), (rep, got)
    c.close_sync(10)
    st = srv.stats()
    assert st['bad_batches'] == 0 and st['batches_lost'] == 0


# ---- 3. watches across connections ---------------------------------------------

def _watch_scenario(servers):
    a = client(servers)
    b = client(servers)
    a.wait_connected(10)
    b.wait_connected(10)
    got = []
    lock = threading.Lock()

    def rec(*ev):
        with lock:
            got.append(ev)

    def saw(*ev):
        assert wait_for(lambda: ev in got, 10), (ev, got)

    p, d, q = D0 + '/wp', D0 + '/wd', D0 + '/wq'
    b.call_sync('create', p, b'1', {})
    b.call_sync('create', d, b'', {})
    a.watcher(p).on('dataChanged', lambda x, s: rec('p.data', x, s.version))
    a.watcher(d).on('childrenChanged', lambda k, s: rec('d.kids', tuple(
        sorted(k))))
    a.watcher(q).on('created', lambda s: rec('q.created', s.version))
    a.watcher(q).on('deleted', lambda: rec('q.deleted'))
    saw('p.data', b'1', 0)
    saw('d.kids', ())
    b.call_sync('set', p, b'2', -1)
    saw('p.data', b'2', 1)
    b.call_sync('set', p, b'3', -1)             # after the re-arm
    saw('p.data', b'3', 2)
    b.call_sync('create', d + '/x', b'', {})
    saw('d.kids', ('x',))
    b.call_sync('create', d + '/y', b'', {})
    saw('d.kids', ('x', 'y'))
    b.call_sync('create', q, b'q', {})
    saw('q.created', 0)
    b.call_sync('delete', q, -1)
    saw('q.deleted')
    b.call_sync('create', q, b'q', {})
    assert wait_for(lambda: got.count(('q.created', 0)) == 2, 10), got
    a.close_sync(10)
    b.close_sync(10)
    return sorted(set(got), key=repr)


def test_watches_across_connections(srv):
    got = _watch_scenario(srv.servers())
    fake = FakeZKServer()
    try:
        fake.cli_create('/bench', b'')
        fake.cli_create(D0, b'')
        want = _watch_scenario(fake.servers())
    finally:
        fake.shutdown()
    assert got == want


# ---- 4. reconnect with catch-up ------------------------------------------------

def test_reconnect_catches_up(srv):
    a = client(srv.servers())
    b = client(srv.servers())
    a.wait_connected(10)
    b.wait_connected(10)
    p = LEAF % 7
    seen = []
    a.watcher(p).on('dataChanged', lambda x, s: seen.append((x, s.version)))
    assert wait_for(lambda: len(seen) == 1, 10)
    sid = a.getSession().session_id
    again = threading.Event()
    a.once('connect', lambda *_: again.set())
    wrote = threading.Event()

    def cut():
        ok = srv.disconnect(sid)
        b.set(p, b'while away', -1, lambda *e: wrote.set())
        return ok
    assert srv.call(cut)
    assert wrote.wait(10) and again.wait(10)
    assert a.getSession().session_id == sid
    assert wait_for(lambda: (b'while away', 1) in seen, 10), seen
    b.call_sync('set', p, b'back', -1)
    assert wait_for(lambda: (b'back', 2) in seen, 10), seen
    assert seen.count((b'while away', 1)) == 1 and len(seen) == 3, seen
    st = srv.stats()
    assert st['catchup_events'] == 1, st
    a.close_sync(10)
    b.close_sync(10)


# ---- raw-socket peers ------------------------------------------------------------

class Raw(object):
    """A peer that does the handshake by hand with the host codec."""

    def __init__(self, srv, timeout=30000):
        self.s = socket.create_connection(('127.0.0.1', srv.port), timeout=10)
        self.s.sendall(jute.frame(jute.encode_connect_request(
            {'timeOut': timeout, 'sessionId': 0, 'passwd': b'\0' * 16})))
        pkt = jute.decode_connect_response(self.frame())
        self.sid, self.timeout = pkt['sessionId'], pkt['timeOut']
        self.xid = 0

    def frame(self):
        n = struct.unpack('>i', self._read(4))[0]
        return self._read(n)

    def _read(self, n):
        b = b''
        while len(b) < n:
            part = self.s.recv(n - len(b))
            if not part:
                raise EOFError('closed by the server')
            b += part
        return b

    def request(self, pkt):
        self.xid += 1
        pkt = dict(pkt, xid=self.xid)
        self.s.sendall(jute.frame(jute.encode_request(pkt)))
        return jute.decode_response(self.frame(), {self.xid: pkt['opcode']})

    def closed_by_server(self):
        try:
            return self.s.recv(1) == b''
        except (ConnectionResetError, BrokenPipeError):
            return True

    def close(self):
        self.s.close()


# ---- 5. session expiry -----------------------------------------------------------

def test_expiry_and_close_session(gpu):
    from zkmi.server.sessions import GpuSessionTable

    def table(tree):
        t = GpuSessionTable(tree)
        t.MIN_TO = 500
        return t
    srv = _make(gpu, table=table)
    try:
        a = client(srv.servers())
        a.wait_connected(10)
        peer = Raw(srv, timeout=500)
        assert peer.timeout == 500 and peer.sid != 0
        node = D0 + '/silent'
        rep = peer.request({'opcode': 'CREATE', 'path': node, 'data': b'e',
                            'acl': jute.DEFAULT_ACL, 'flags': ['EPHEMERAL']})
        assert rep['err'] == 'OK'
        gone = threading.Event()
        a.watcher(node).on('deleted', gone.set)
        assert gone.wait(5)
        assert a.isConnected()
        assert srv.call(lambda: srv.tree.find_host(node)) == -1
        assert peer.closed_by_server()
        peer.close()
        st = srv.stats()
        assert st['sessions_expired'] == 1 and st['expiry_passes'] == 1
        assert st['watcher_slots'] == 1 and st['max_reads_per_tick'] <= 2
        # CLOSE_SESSION from a real client: its ephemerals go at once and its
        # watcher slot is free again
        c = client(srv.servers())
        c.wait_connected(10)
        mine = D0 + '/mine'
        c.call_sync('create', mine, b'', {'flags': ['EPHEMERAL']})
        assert srv.stats()['watcher_slots'] == 2
        away, armed = threading.Event(), threading.Event()
        a.watcher(mine).on('deleted', away.set)
        a.watcher(mine).on('dataChanged', lambda x, s: armed.set())
        assert armed.wait(10)
        c.close_sync(10)
        assert srv.call(lambda: srv.tree.find_host(mine)) == -1
        assert away.wait(10)
        st = srv.stats()
        assert st['watcher_slots'] == 1 and st['sessions_closed'] == 1
        a.close_sync(10)
    finally:
        srv.shutdown()
    assert srv.error is None, srv.error


# ---- 6. bad peers do not hurt good ones ------------------------------------------

def test_bad_peers(srv):
    a = client(srv.servers())
    a.wait_connected(10)
    bad = Raw(srv)
    half = Raw(srv)
    want = {}
    for k in range(5):
        want[LEAF % k] = a.call_sync('get', LEAF % k)[0]
    f = jute.frame(jute.encode_request(
        {'opcode': 'GET_DATA', 'path': LEAF % 1, 'watch': False, 'xid': 9}))
    results = []
    done = threading.Event()

    def cb(p):
        def g(err, data=None, stat=None):
            results.append((p, err, data))
            if len(results) == 200:
                done.set()
        return g

    def issue(lo, hi):
        for k in range(lo, hi):
            a.get(LEAF % (k % 5), cb(LEAF % (k % 5)))
    a.loop.run(lambda: issue(0, 100))
    bad.s.sendall(f + struct.pack('>i', -1) + f)
    half.s.sendall(f[:len(f) // 2])
    a.loop.run(lambda: issue(100, 200))
    assert done.wait(10)
    assert all(e is None and d == want[p] for p, e, d in results)
    # the frame before the bad length was served, then the socket closed
    rep = jute.decode_response(bad.frame(), {9: 'GET_DATA'})
    assert rep['err'] == 'OK' and rep['data'] == want[LEAF % 1]
    assert bad.closed_by_server()
    assert wait_for(lambda: srv.stats()['bad_length'] == 1, 10)
    st = srv.stats()
    assert st['bad_batches'] == 0 and st['batches_lost'] == 0
    assert st['connections'] == 2                 # a and the stalled peer
    # the stalled peer's frame is served once it is whole
    half.s.sendall(f[len(f) // 2:])
    rep = jute.decode_response(half.frame(), {9: 'GET_DATA'})
    assert rep['err'] == 'OK' and rep['data'] == want[LEAF % 1]
    bad.close()
    half.close()
    a.close_sync(10)


# ---- 7. more sessions than watcher slots ---------------------------------------

def test_more_sessions_than_watcher_slots(srv):
    peers = [Raw(srv) for _ in range(70)]
    st = srv.stats()
    assert st['no_watcher_slot'] == 6 and st['watcher_slots'] == 64
    slots = srv.call(lambda: [srv.sessions[p.sid].wslot for p in peers])
    assert slots == list(range(64)) + [-1] * 6
    want = peers[0].request({'opcode': 'GET_DATA', 'path': LEAF % 3,
                             'watch': False})
    for p in peers[64:]:
        rep = p.request({'opcode': 'GET_DATA', 'path': LEAF % 3,
                         'watch': True})
        assert rep['err'] == 'OK' and rep['data'] == want['data']
    rep = peers[0].request({'opcode': 'CLOSE_SESSION'})
    assert rep['err'] == 'OK' and peers[0].closed_by_server()
    late = Raw(srv)
    assert srv.call(lambda: srv.sessions[late.sid].wslot) == 0
    st = srv.stats()
    assert st['no_watcher_slot'] == 6 and st['watcher_slots'] == 64
    assert st['sessions'] == 70
    for p in peers + [late]:
        p.close()
