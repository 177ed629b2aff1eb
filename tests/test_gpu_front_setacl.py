"""zkmi.Client against GpuZKServer over 127.0.0.1: ``set_acl`` re-protects a
node (csrc/kernels/tree_setacl.hip; the rule: zk_setacl.h), in the plain and
in the ordered tick.  Every wait is bounded by 10 s; the server is shut down
in each test's ``finally``."""

import base64
import hashlib
import threading

import pytest

from zkmi.errors import ZKError

from zkhelpers import client

pytestmark = pytest.mark.gpu

D0 = '/bench/d000000'
READ, WRITE, CREATE, DELETE, ADMIN, ALL = 1, 2, 4, 8, 16, 31
NO_AUTH = ('ERR', 'NO_AUTH')
ALL_NAMES = ['READ', 'WRITE', 'CREATE', 'DELETE', 'ADMIN']


def ident(cred):
    return (cred.split(b':', 1)[0] + b':' +
            base64.b64encode(hashlib.sha1(cred).digest())).decode()


def ent(perms, scheme='world', who='anyone'):
    return {'perms': perms, 'id': {'scheme': scheme, 'id': who}}


def _make(gpu, **kw):
    from zkmi.server.tree import GpuTree
    from zkmi.server.gpu import GpuZKServer
    tree = GpuTree(n_nodes=2000, fanout=100, watch_cap=4096, acl_cap=64,
                   scratch=1 << 20, device=gpu)
    kw.setdefault('cap_frames', 1024)
    kw.setdefault('out_cap', 1 << 20)
    kw.setdefault('max_conns', 4)
    return GpuZKServer(tree, **kw)


def _call(c, method, *args):
    try:
        return c.call_sync(method, *args, timeout=10)
    except ZKError as e:
        return ('ERR', e.code)


def _pipeline(c, calls):
    """Issue ``calls`` ([(method, args)]) from one turn of the client's loop,
    so they leave in one write; returns every callback's outcome in order
    (the error's code, or the callback's values)."""
    n = len(calls)
    got = [None] * n
    done = threading.Event()
    left = [n]

    def cb(k):
        def f(err=None, *res):
            got[k] = err.code if err is not None else res
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


@pytest.mark.parametrize('order_passes', [0, 4])
def test_owner_re_protects_a_node(gpu, order_passes):
    s = _make(gpu, order_passes=order_passes, enforce_acl=True)
    owner = client(s.servers())
    other = client(s.servers())
    try:
        owner.wait_connected(10)
        other.wait_connected(10)
        node = D0 + '/shared'
        me = ident(b'own:secret')
        assert _call(owner, 'create', node, b'v', {}) == node
        assert _call(other, 'get', node)[0] == b'v'
        assert _call(owner, 'add_auth', 'digest', b'own:secret') is None
        mine = [ent(ALL, 'digest', me)]
        st = _call(owner, 'set_acl', node, mine, -1)
        assert st.aversion == 1 and st.version == 0
        assert _call(owner, 'get_acl', node) == \
            [ent(ALL_NAMES, 'digest', me)]
        # the second client: shut out of set_acl and of what the ACL shuts
        assert _call(other, 'set_acl', node, [ent(ALL)], -1) == NO_AUTH
        assert _call(other, 'get', node) == NO_AUTH
        assert _call(other, 'set', node, b'x', -1) == NO_AUTH
        assert _call(other, 'create', node + '/kid', b'', {}) == NO_AUTH
        assert _call(owner, 'get', node)[0] == b'v'
        # ... until it holds the identity
        assert _call(other, 'add_auth', 'digest', b'own:secret') is None
        assert _call(other, 'get', node)[0] == b'v'
        st = _call(other, 'set_acl', node, mine + [ent(READ)], 1)
        assert st.aversion == 2
        # aversion and BAD_VERSION over the wire
        assert _call(owner, 'set_acl', node, mine, 1) == \
            ('ERR', 'BAD_VERSION')
        assert _call(owner, 'set_acl', node, [], -1) == ('ERR', 'INVALID_ACL')
        assert _call(owner, 'set_acl', node + '/none', mine, -1) == \
            ('ERR', 'NO_NODE')
        assert _call(owner, 'stat', node).aversion == 2
        stt = s.stats()
        assert stt['setacl_unreached'] == 0 and stt['batches_lost'] == 0
        assert stt['bad_batches'] == 0 and stt['max_reads_per_tick'] <= 2
        assert s.call(lambda: s.gs.setacl_stats())['applied'] == 2
    finally:
        for c in (owner, other):
            if not c.isInState('closed'):
                c.close_sync(10)
        s.shutdown()
    assert s.error is None, s.error


@pytest.mark.parametrize('order_passes', [0, 4])
def test_pipelined_get_set_get_keeps_the_connections_order(gpu, order_passes):
    s = _make(gpu, order_passes=order_passes)
    c = client(s.servers())
    try:
        c.wait_connected(10)
        node = D0 + '/n000000007'
        new = [ent(READ), ent(ALL, 'ip', '127.0.0.1')]
        got = _pipeline(c, [('get_acl', (node,)),
                            ('set_acl', (node, new, 0)),
                            ('get_acl', (node,)),
                            ('set', (node, b'after', -1)),
                            ('set_acl', (node, [ent(ALL)], 1)),
                            ('get_acl', (node,))])
        assert got[0] == ([ent(ALL_NAMES)],)
        assert got[1][0].aversion == 1
        assert got[2] == ([ent(['READ']),
                           ent(ALL_NAMES, 'ip', '127.0.0.1')],)
        assert got[3] == ()
        assert got[4][0].aversion == 2 and got[4][0].version == 1
        assert got[5] == ([ent(ALL_NAMES)],)
        # without enforcement nothing is checked
        assert _call(c, 'set_acl', node, [ent(READ)], 2).aversion == 3
        assert _call(c, 'set_acl', node, [ent(ALL)], -1).aversion == 4
        assert s.stats()['max_reads_per_tick'] <= 2
    finally:
        if not c.isInState('closed'):
            c.close_sync(10)
        s.shutdown()
    assert s.error is None, s.error
