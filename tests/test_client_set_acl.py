"""``Client.set_acl`` against :class:`FakeZKServer`: set then ``get_acl``,
``aversion`` in the returned Stat, the error codes, the argument checks, with
the native reply router on (where the loop has one) and off."""

import pytest

from zkmi import jute
from zkmi.errors import ZKError
from zkmi.server import FakeZKServer

from zkhelpers import Box, client, fast_config

OWNER = {'perms': ['READ', 'WRITE', 'CREATE', 'DELETE', 'ADMIN'],
         'id': {'scheme': 'digest', 'id': 'u:BvFaefuhWURhnvpD7ipe45CKTpk='}}
READERS = {'perms': ['READ'], 'id': {'scheme': 'world', 'id': 'anyone'}}


@pytest.fixture
def zk():
    s = FakeZKServer(tick_ms=250)
    yield s
    s.shutdown()


@pytest.fixture(params=[True, False], ids=['routed', 'native_route_off'])
def c(request, zk):
    cl = client(zk.servers(), config=fast_config(native_route=request.param))
    cl.wait_connected(10)
    if not request.param:
        assert not cl.session.conn.routing
    yield cl
    cl.close_sync(10)


def test_set_then_get(c, zk):
    zk.cli_create('/n', b'x')
    assert c.call_sync('get_acl', '/n', timeout=10) == \
        [{'perms': ['READ', 'WRITE', 'CREATE', 'DELETE', 'ADMIN'],
          'id': {'scheme': 'world', 'id': 'anyone'}}]
    before = c.call_sync('stat', '/n', timeout=10)
    st = c.call_sync('set_acl', '/n', [OWNER, READERS], -1, timeout=10)
    assert isinstance(st, jute.Stat)
    assert st.aversion == 1 and before.aversion == 0
    # nothing else of the node moves
    assert (st.version, st.cversion, st.mzxid, st.czxid, st.dataLength) == \
        (before.version, before.cversion, before.mzxid, before.czxid,
         before.dataLength)
    assert c.call_sync('get_acl', '/n', timeout=10) == [OWNER, READERS]
    assert c.call_sync('stat', '/n', timeout=10) == st
    assert c.call_sync('get', '/n', timeout=10)[0] == b'x'


def test_aversion_counts_up(c, zk):
    zk.cli_create('/n', b'')
    z0 = zk.run(lambda: zk.db.zxid)
    # the camel-case name, an explicit version, None for "any"
    s1 = c.call_sync('setACL', '/n', [OWNER], 0, timeout=10)
    s2 = c.call_sync('set_acl', '/n', [READERS], 1, timeout=10)
    s3 = c.call_sync('set_acl', '/n', [OWNER, READERS], None, timeout=10)
    assert [s.aversion for s in (s1, s2, s3)] == [1, 2, 3]
    # each took a zxid
    assert zk.run(lambda: zk.db.zxid) == z0 + 3
    assert c.call_sync('get_acl', '/n', timeout=10) == [OWNER, READERS]


def _code(c, *args):
    with pytest.raises(ZKError) as e:
        c.call_sync('set_acl', *args, timeout=10)
    return e.value.code


def test_errors(c, zk):
    zk.cli_create('/n', b'')
    z0 = zk.run(lambda: zk.db.zxid)
    assert _code(c, '/n', [OWNER], 1) == 'BAD_VERSION'
    assert _code(c, '/n', [OWNER], 7) == 'BAD_VERSION'
    assert _code(c, '/missing', [OWNER], -1) == 'NO_NODE'
    assert _code(c, '/n', [], -1) == 'INVALID_ACL'
    # INVALID_ACL comes before NO_NODE, NO_NODE before BAD_VERSION
    assert _code(c, '/missing', [], 5) == 'INVALID_ACL'
    assert _code(c, '/missing', [OWNER], 5) == 'NO_NODE'
    # nothing happened
    assert zk.run(lambda: zk.db.zxid) == z0
    assert c.call_sync('stat', '/n', timeout=10).aversion == 0
    assert c.call_sync('get_acl', '/n', timeout=10)[0]['id'] == \
        {'scheme': 'world', 'id': 'anyone'}
    # ... and the connection goes on serving
    assert c.call_sync('set_acl', '/n', [OWNER], 0, timeout=10).aversion == 1


def test_callback_form(c, zk):
    zk.cli_create('/n', b'')
    b = Box()
    c.set_acl('/n', [READERS], -1, b)
    err, st = b.wait(10)
    assert err is None and st.aversion == 1
    b = Box()
    c.set_acl('/gone', [READERS], -1, b)
    (err,) = b.wait(10)
    assert isinstance(err, ZKError) and err.code == 'NO_NODE'


def test_argument_checks(c):
    def cb(*a):
        pass
    with pytest.raises(TypeError):
        c.set_acl(5, [OWNER], -1, cb)
    with pytest.raises(TypeError):
        c.set_acl('/n', OWNER, -1, cb)
    with pytest.raises(TypeError):
        c.set_acl('/n', ['world'], -1, cb)
    with pytest.raises(TypeError):
        c.set_acl('/n', [OWNER], '1', cb)
    with pytest.raises(TypeError):
        c.set_acl('/n', [OWNER], True, cb)
    with pytest.raises(TypeError):
        c.set_acl('/n', [OWNER], -1, None)
    assert 'SET_ACL' not in c.BULK_OPS
    with pytest.raises(ValueError):
        c.bulk([{'opcode': 'SET_ACL', 'path': '/n', 'acl': [OWNER]}], cb)
