"""zkmi.Client against GpuZKServer(order_passes=4): a connection's pipelined
writes are served in one tick, and what the passes cannot reach is deferred,
not refused.  The same scripts run against FakeZKServer and every callback's
result must be equal.  Every wait is bounded by 10 s; the servers are shut
down in teardown."""

import threading

import pytest

from zkmi.errors import ZKError
from zkmi.server.fakezk import FakeZKServer

from zkhelpers import client, wait_for

pytestmark = pytest.mark.gpu

D0 = '/bench/d000000'
HOT = D0 + '/n%09d' % 5
STAT_FIELDS = ('version', 'cversion', 'aversion', 'dataLength', 'numChildren')


def _make(gpu, **kw):
    from zkmi.server.tree import GpuTree
    from zkmi.server.gpu import GpuZKServer
    tree = GpuTree(n_nodes=2000, fanout=100, watch_cap=4096, acl_cap=64,
                   scratch=kw.pop('scratch', 1 << 20), device=gpu)
    kw.setdefault('cap_frames', 1024)
    kw.setdefault('out_cap', 1 << 20)
    kw.setdefault('max_conns', 128)
    kw.setdefault('order_passes', 4)
    return GpuZKServer(tree, **kw)


@pytest.fixture
def srv(gpu):
    s = _make(gpu)
    yield s
    s.shutdown()
    assert s.error is None, s.error


@pytest.fixture
def fake():
    f = FakeZKServer()
    f.cli_create('/bench', b'')
    f.cli_create(D0, b'')
    for i in range(100):
        f.cli_create(D0 + '/n%09d' % i, b'x' * 100)
    yield f
    f.shutdown()


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


def _pipeline(c, calls):
    """Issue ``calls`` ([(method, args)]) from one turn of the client's loop,
    so they leave in one write; returns every callback's result in order."""
    n = len(calls)
    got = [None] * n
    done = threading.Event()
    left = [n]

    def cb(k):
        def f(err=None, *res):
            got[k] = ('ERR', err.code) if err is not None else _norm(res)
            left[0] -= 1
            if left[0] == 0:
                done.set()
        return f

    def issue():
        for k, (method, args) in enumerate(calls):
            getattr(c, method)(*(tuple(args) + (cb(k),)))
    c.loop.run(issue)
    assert done.wait(10), got
    return got


def _script(c):
    """32 sets of one path in one write, then a chain on 16 paths in one
    write: create, set, get, list of the parent, delete."""
    out = []
    out += _pipeline(c, [('set', (HOT, b'v%02d' % k, -1)) for k in range(32)])
    out += _pipeline(c, [('get', (HOT,))])
    calls = []
    for k in range(16):
        p = D0 + '/ch%02d' % k
        calls += [('create', (p, b'c%d' % k, {})), ('set', (p, b'dd%d' % k, -1)),
                  ('get', (p,)), ('list', (D0,)), ('delete', (p, -1))]
    out += _pipeline(c, calls)
    out += _pipeline(c, [('list', (D0,)), ('stat', (D0,))])
    return out


def test_ordered_mode_needs_a_scratch_tail(gpu):
    from zkmi.server.tree import GpuTree
    from zkmi.server.gpu import GpuZKServer
    tree = GpuTree(n_nodes=200, fanout=100, watch_cap=1024, device=gpu)
    with pytest.raises(ValueError):
        GpuZKServer(tree, 64, 1 << 16, max_conns=4, order_passes=4)


def test_pipelined_writes_in_one_tick(srv, fake):
    c = client(srv.servers())
    c.wait_connected(10)
    got = _script(c)
    c.close_sync(10)
    f = client(fake.servers())
    f.wait_connected(10)
    want = _script(f)
    f.close_sync(10)
    assert len(got) == len(want) == 32 + 1 + 80 + 2
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)
    assert got[32][0] == b'v31' and got[32][1][0] == 32
    st = srv.stats()
    assert st['bad_batches'] == 0 and st['batches_lost'] == 0
    assert st['max_reads_per_tick'] <= 2
    # the feature: several writes of one connection in one tick, and the ones
    # the four passes could not reach were deferred, not refused
    assert st['max_writes_per_tick'] > 1
    assert st['deferred_frames'] > 0
    assert st['order_max_rank'] >= 4
    assert st['order_scratch_full'] == 0


def test_seventy_sessions_set_one_znode(srv):
    n = 70
    cs = [client(srv.servers()) for _ in range(n)]
    for c in cs:
        c.wait_connected(10)
    res = [None] * n
    left = [n]
    done = threading.Event()
    lock = threading.Lock()

    def cb(k):
        def f(err=None, *r):
            with lock:
                res[k] = ('ERR', err.code) if err is not None else 'OK'
                left[0] -= 1
                if left[0] == 0:
                    done.set()
        return f

    for k, c in enumerate(cs):
        c.loop.run(lambda c=c, k=k: c.set(HOT, b's%02d' % k, -1, cb(k)))
    assert done.wait(10), res
    assert res == ['OK'] * n
    data, stat = cs[0].call_sync('get', HOT, timeout=10)
    assert stat.version == n
    for c in cs:
        c.close_sync(10)
    st = srv.stats()
    assert st['bad_batches'] == 0 and st['batches_lost'] == 0


def test_sequential_creates_beside_a_deferred_one(srv):
    """One connection's SEQUENTIAL create stands behind more sets of one path
    than a tick's passes reach, so it is deferred with a number taken, while
    other connections create SEQUENTIAL nodes under the same parent: every
    create succeeds and no name is given twice."""
    a = client(srv.servers())
    others = [client(srv.servers()) for _ in range(3)]
    for c in [a] + others:
        c.wait_connected(10)
    seq = ('create', (D0 + '/q-', b's', {'flags': ['SEQUENTIAL']}))
    res = {}
    ts = [threading.Thread(target=lambda: res.__setitem__('a', _pipeline(
        a, [('set', (HOT, b'x', -1))] * 9 + [seq] * 2)))]
    for k, c in enumerate(others):
        ts.append(threading.Thread(target=lambda k=k, c=c: res.__setitem__(
            k, _pipeline(c, [seq] * 6))))
    for t in ts:
        t.start()
    for t in ts:
        t.join(20)
    names = [r[0] for r in res['a'][9:]] + \
        [r[0] for k in range(3) for r in res[k]]
    assert all(isinstance(n, str) and n.startswith(D0 + '/q-')
               for n in names), names
    assert len(set(names)) == len(names) == 20
    kids, _ = a.call_sync('list', D0, timeout=10)
    assert sorted(k for k in kids if k.startswith('q-')) == \
        sorted(n.rsplit('/', 1)[1] for n in names)
    for c in [a] + others:
        c.close_sync(10)
    assert srv.stats()['deferred_frames'] > 0


def _watch_script(servers):
    """get(watch) then set of the same path, in one write of one connection:
    the watcher's fetches, in order."""
    c = client(servers)
    c.wait_connected(10)
    p = D0 + '/n%09d' % 9
    got = []
    lock = threading.Lock()

    def rec(data, st):
        # (the two servers' trees start with other bytes in the leaf)
        with lock:
            got.append((data if st.version else None, st.version))

    def issue():
        c.watcher(p).on('dataChanged', rec)
        c.set(p, b'new', -1, lambda err=None, *r: None)
    c.loop.run(issue)
    assert wait_for(lambda: (b'new', 1) in got, 10), got
    # a round trip behind it: nothing more is on its way
    c.call_sync('sync', p, timeout=10)
    c.call_sync('get', p, timeout=10)
    c.close_sync(10)
    return got


def test_watch_then_set_on_one_connection(srv, fake):
    got = _watch_script(srv.servers())
    want = _watch_script(fake.servers())
    assert got == want
    assert got.count((b'new', 1)) == 1          # exactly one dataChanged


def test_default_is_one_write_a_tick(gpu):
    """order_passes=0: the tick of before (its scenarios: test_gpu_front_end);
    the ordered counters stay 0."""
    s = _make(gpu, order_passes=0, scratch=0)
    try:
        c = client(s.servers())
        c.wait_connected(10)
        got = _pipeline(c, [('set', (HOT, b'v%02d' % k, -1))
                            for k in range(8)])
        assert got == [()] * 8
        c.close_sync(10)
        st = s.stats()
        assert st['max_writes_per_tick'] == 0 and st['deferred_frames'] == 0
        assert st['ticks'] >= 8
    finally:
        s.shutdown()
    assert s.error is None, s.error
