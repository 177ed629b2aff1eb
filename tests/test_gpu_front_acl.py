"""zkmi.Client against GpuZKServer(enforce_acl=True) over 127.0.0.1: the ACL a
client stored is honoured (csrc/kernels/tree_aclperm.hip; the rule:
zk_aclperm.h).  The client's identity is its peer address, 127.0.0.1: no AUTH.
Every wait is bounded by 10 s; the server is shut down in the fixture's
teardown."""

import threading

import pytest

from zkmi.errors import ZKError

from zkhelpers import client

pytestmark = pytest.mark.gpu

D0 = '/bench/d000000'
READ, WRITE, CREATE, DELETE, ADMIN, ALL = 1, 2, 4, 8, 16, 31


def acl(perms, scheme='world', ident='anyone'):
    return {'acl': [{'perms': perms, 'id': {'scheme': scheme, 'id': ident}}]}


def _make(gpu, **kw):
    from zkmi.server.tree import GpuTree
    from zkmi.server.gpu import GpuZKServer
    tree = GpuTree(n_nodes=2000, fanout=100, watch_cap=4096, acl_cap=64,
                   scratch=1 << 20, device=gpu)
    kw.setdefault('cap_frames', 1024)
    kw.setdefault('out_cap', 1 << 20)
    kw.setdefault('max_conns', 16)
    return GpuZKServer(tree, **kw)


def _serving(gpu, **kw):
    s = _make(gpu, **kw)
    c = client(s.servers())
    c.wait_connected(10)
    return s, c


def _done(s, c):
    c.close_sync(10)
    s.shutdown()
    assert s.error is None, s.error


def _call(c, method, *args):
    try:
        return c.call_sync(method, *args, timeout=10)
    except ZKError as e:
        return ('ERR', e.code)


def _pipeline(c, calls):
    """Issue ``calls`` ([(method, args)]) from one turn of the client's loop,
    so they leave in one write; returns every callback's outcome in order
    ('OK' or the error's code)."""
    n = len(calls)
    got = [None] * n
    done = threading.Event()
    left = [n]

    def cb(k):
        def f(err=None, *res):
            got[k] = err.code if err is not None else 'OK'
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


NO_AUTH = ('ERR', 'NO_AUTH')


def _nodes(c):
    """The protected nodes, made by the client itself under the open D0."""
    assert _call(c, 'create', D0 + '/ro', b'r', acl(READ)) == D0 + '/ro'
    assert _call(c, 'create', D0 + '/noread', b'', acl(ALL & ~READ)) == \
        D0 + '/noread'
    assert _call(c, 'create', D0 + '/mine', b'', acl(ALL, 'ip', '127.0.0.1'))\
        == D0 + '/mine'
    assert _call(c, 'create', D0 + '/theirs', b'',
                 acl(ALL, 'ip', '10.9.9.9')) == D0 + '/theirs'
    assert _call(c, 'create', D0 + '/keep', b'', acl(ALL & ~DELETE)) == \
        D0 + '/keep'
    assert _call(c, 'create', D0 + '/keep/child', b'', {}) == \
        D0 + '/keep/child'


@pytest.mark.parametrize('order_passes', [0, 4])
def test_stored_acls_are_honoured(gpu, order_passes):
    s, c = _serving(gpu, enforce_acl=True, order_passes=order_passes)
    try:
        _nodes(c)
        data, st = _call(c, 'get', D0 + '/ro')
        assert data == b'r'
        assert _call(c, 'set', D0 + '/ro', b'x', -1) == NO_AUTH
        assert _call(c, 'create', D0 + '/ro/x', b'', {}) == NO_AUTH
        assert _call(c, 'list', D0 + '/noread') == NO_AUTH
        assert _call(c, 'get', D0 + '/noread') == NO_AUTH
        assert _call(c, 'stat', D0 + '/ro').version == 0
        assert _call(c, 'stat', D0 + '/noread').version == 0
        got = _call(c, 'getACL', D0 + '/ro')
        assert [(a['id']['scheme'], a['id']['id']) for a in got] == \
            [('world', 'anyone')]
        assert len(_call(c, 'getACL', D0 + '/noread')) == 1
        # the peer is 127.0.0.1
        assert _call(c, 'set', D0 + '/mine', b'm', -1) is None
        assert _call(c, 'create', D0 + '/mine/c', b'', {}) == D0 + '/mine/c'
        assert _call(c, 'get', D0 + '/mine')[0] == b'm'
        assert _call(c, 'set', D0 + '/theirs', b'm', -1) == NO_AUTH
        assert _call(c, 'get', D0 + '/theirs') == NO_AUTH
        # a parent without DELETE keeps its child; NO_NODE still comes first
        assert _call(c, 'delete', D0 + '/keep/child', -1) == NO_AUTH
        assert _call(c, 'delete', D0 + '/keep/none', -1) == ('ERR', 'NO_NODE')
        assert _call(c, 'stat', D0 + '/keep/child').version == 0
        assert _call(c, 'delete', D0 + '/mine/c', -1) is None
        # more pipelined sets than one tick serves, of a permitted and a
        # denied node in turn: request order, the right codes
        calls = []
        for k in range(12):
            calls += [('set', (D0 + '/mine', b'v%02d' % k, -1)),
                      ('set', (D0 + '/ro', b'v%02d' % k, -1))]
        assert _pipeline(c, calls) == ['OK', 'NO_AUTH'] * 12
        assert _call(c, 'get', D0 + '/mine')[0] == b'v11'
        assert _call(c, 'get', D0 + '/ro')[0] == b'r'
        st = s.stats()
        assert st['acl_denied'] == 7 + 12
        assert st['max_reads_per_tick'] <= 2
        assert st['batches_lost'] == 0 and st['bad_batches'] == 0
        # (the check's own count: a denied frame the ordered tick deferred
        # was checked again in the tick that served it)
        den = s.call(lambda: s.gs.acl_enforce_stats())['denied']
        assert den == 19 if order_passes == 0 else den >= 19
    finally:
        _done(s, c)


def test_off_is_the_behaviour_of_before(gpu):
    s, c = _serving(gpu)
    try:
        _nodes(c)
        assert _call(c, 'set', D0 + '/ro', b'x', -1) is None
        assert _call(c, 'create', D0 + '/ro/x', b'', {}) == D0 + '/ro/x'
        assert _call(c, 'list', D0 + '/noread')[0] == []
        assert _call(c, 'set', D0 + '/theirs', b'm', -1) is None
        assert _call(c, 'delete', D0 + '/keep/child', -1) is None
        calls = []
        for k in range(4):
            calls += [('set', (D0 + '/mine', b'v', -1)),
                      ('set', (D0 + '/ro', b'v', -1))]
        assert _pipeline(c, calls) == ['OK'] * 8
        st = s.stats()
        assert st['acl_denied'] == 0
        assert s.call(lambda: s.gs.acl_enforce_stats())['denied'] == 0
    finally:
        _done(s, c)


def test_needs_an_acl_table(gpu):
    from zkmi.server.tree import GpuTree
    from zkmi.server.gpu import GpuZKServer
    tree = GpuTree(n_nodes=2000, fanout=100, watch_cap=64, device=gpu)
    with pytest.raises(ValueError):
        GpuZKServer(tree, 64, 1 << 16, max_conns=4, enforce_acl=True)


def test_peer_ipv4():
    from zkmi.server.gpu import peer_ipv4
    assert peer_ipv4(('127.0.0.1', 5)) == 0x7F000001
    assert peer_ipv4(('10.1.2.9', 5)) == 0x0A010209
    assert peer_ipv4(('200.1.2.9', 5)) == 0xC8010209 - (1 << 32)
    assert peer_ipv4(('::ffff:10.1.2.9', 5, 0, 0)) == 0x0A010209
    assert peer_ipv4(('::1', 5, 0, 0)) == 0
    assert peer_ipv4(('fe80::1%eth0', 5, 0, 3)) == 0
    assert peer_ipv4(('nonsense', 5)) == 0
    assert peer_ipv4(None) == 0 and peer_ipv4(()) == 0
