"""zkmi.Client against GpuZKServer(enforce_acl=True) over 127.0.0.1: a node
with a ``digest`` ACL opens to a connection after ``add_auth`` and to no
other (csrc/kernels/tree_auth.hip; the rule: zk_auth.h).  Every wait is
bounded by 10 s; the server is shut down in each test's ``finally``."""

import base64
import hashlib

import pytest

from zkmi.errors import ZKError

from zkhelpers import client, wait_for

pytestmark = pytest.mark.gpu

D0 = '/bench/d000000'
READ, WRITE, CREATE, DELETE, ADMIN, ALL = 1, 2, 4, 8, 16, 31
NO_AUTH = ('ERR', 'NO_AUTH')


def ident(cred):
    return (cred.split(b':', 1)[0] + b':' +
            base64.b64encode(hashlib.sha1(cred).digest())).decode()


def acl(perms, scheme, who):
    return {'acl': [{'perms': perms, 'id': {'scheme': scheme, 'id': who}}]}


def _make(gpu, **kw):
    from zkmi.server.tree import GpuTree
    from zkmi.server.gpu import GpuZKServer
    tree = GpuTree(n_nodes=2000, fanout=100, watch_cap=4096, acl_cap=64,
                   scratch=1 << 20, device=gpu)
    kw.setdefault('cap_frames', 1024)
    kw.setdefault('out_cap', 1 << 20)
    kw.setdefault('max_conns', 1)
    return GpuZKServer(tree, enforce_acl=True, **kw)


def _call(c, method, *args):
    try:
        return c.call_sync(method, *args, timeout=10)
    except ZKError as e:
        return ('ERR', e.code)


@pytest.mark.parametrize('order_passes', [0, 4])
def test_digest_acl_opens_after_add_auth(gpu, order_passes):
    # one row: the second client's connection takes the first one's
    s = _make(gpu, order_passes=order_passes)
    c = client(s.servers())
    c2 = None
    try:
        c.wait_connected(10)
        node = D0 + '/secret'
        assert _call(c, 'create', node, b'top',
                     acl(READ | WRITE, 'digest', ident(b'u:pw'))) == node
        assert ident(b'u:pw') == 'u:BvFaefuhWURhnvpD7ipe45CKTpk='
        assert _call(c, 'get', node) == NO_AUTH
        assert _call(c, 'set', node, b'x', -1) == NO_AUTH
        # a wrong password: AUTH itself succeeds, as in ZooKeeper; the node
        # stays shut
        assert _call(c, 'add_auth', 'digest', b'u:wrong') is None
        assert _call(c, 'get', node) == NO_AUTH
        # a scheme this server does not know: AUTH_FAILED, the connection
        # stays
        assert _call(c, 'add_auth', 'sasl', b'u:pw') == ('ERR', 'AUTH_FAILED')
        assert _call(c, 'get', node) == NO_AUTH
        assert _call(c, 'add_auth', 'digest', b'u:pw') is None
        assert _call(c, 'get', node)[0] == b'top'
        assert _call(c, 'set', node, b'new', -1) is None
        assert _call(c, 'get', node)[0] == b'new'
        # READ and WRITE only
        assert _call(c, 'create', node + '/kid', b'', {}) == NO_AUTH
        # the same credentials again take no slot
        assert _call(c, 'addAuth', 'digest', b'u:pw') is None
        st = s.stats()
        a = st['auth_stats']
        assert a['answered_ok'] == 3 and a['answered_failed'] == 1
        assert a['known'] >= 1 and a['full'] == 0 and a['failed'] >= 1
        assert st['batches_lost'] == 0 and st['bad_batches'] == 0
        assert st['max_reads_per_tick'] <= 2
        row = s.call(lambda: s.auth.identities()[0])
        assert sorted(row) == sorted([ident(b'u:pw').encode(),
                                      ident(b'u:wrong').encode()])
        # the connection goes; the next one takes its row and is anonymous
        c.close_sync(10)
        assert wait_for(lambda: s.stats()['connections'] == 0, 10)
        c2 = client(s.servers())
        c2.wait_connected(10)
        assert _call(c2, 'get', node) == NO_AUTH
        assert s.call(lambda: s.auth.identities()[0]) == []
        assert _call(c2, 'add_auth', 'digest', b'u:pw') is None
        assert _call(c2, 'get', node)[0] == b'new'
        assert s.stats()['auth_stats']['answered_ok'] == 4
    finally:
        if c2 is not None:
            c2.close_sync(10)
        elif not c.isInState('closed'):
            c.close_sync(10)
        s.shutdown()
    assert s.error is None, s.error


def test_without_enforcement_auth_is_no_request(gpu):
    """enforce_acl off: the server keeps no identities, and an AUTH frame is
    the unknown request it was."""
    from zkmi.server.tree import GpuTree
    from zkmi.server.gpu import GpuZKServer
    tree = GpuTree(n_nodes=2000, fanout=100, watch_cap=4096, acl_cap=64,
                   scratch=1 << 20, device=gpu)
    s = GpuZKServer(tree, 1024, 1 << 20, max_conns=4)
    c = client(s.servers())
    try:
        c.wait_connected(10)
        assert s.auth is None
        assert _call(c, 'add_auth', 'digest', b'u:pw') == \
            ('ERR', 'BAD_ARGUMENTS')
        assert 'auth_stats' not in s.stats()
        assert c._auths == []
    finally:
        c.close_sync(10)
        s.shutdown()
    assert s.error is None, s.error
