"""``Client.add_auth``: the AUTH request on the wire (the Jute oracle and the
native host codec produce the golden bytes), and the call against
:class:`FakeZKServer` — success, an unknown scheme, and the credentials
reaching the new connection after a forced reconnect."""

import os
import sys

import pytest

from zkmi import jute
from zkmi.errors import ZKDecodeError, ZKError
from zkmi.server import FakeZKServer

from zkhelpers import Recorder, client, wait_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# xid -4, opcode 100, type 0, scheme 'digest', auth 'u:pw': 34 bytes, the
# length prefix 30
GOLDEN = bytes.fromhex('0000001e' 'fffffffc' '00000064' '00000000'
                       '00000006') + b'digest' + \
    bytes.fromhex('00000004') + b'u:pw'
U_ID = b'u:BvFaefuhWURhnvpD7ipe45CKTpk='
PKT = {'xid': -4, 'opcode': 'AUTH', 'type': 0, 'scheme': 'digest',
       'auth': b'u:pw'}


@pytest.fixture(scope='module')
def native():
    if os.environ.get('ZKMI_HOST_CODEC_PATH'):
        from zkmi import codec
        assert codec.IMPL == 'native'
        return codec._zkhost
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import build_native
    build_native.build_host()
    from zkmi import _zkhost
    _zkhost.init(jute.Stat, ZKDecodeError)
    return _zkhost


@pytest.fixture
def zk():
    s = FakeZKServer(tick_ms=250)
    yield s
    s.shutdown()


def test_golden_frame_jute():
    assert len(GOLDEN) == 34
    assert jute.frame(jute.encode_request(dict(PKT))) == GOLDEN
    assert jute.decode_request(GOLDEN[4:], auth=True) == PKT
    # (without the flag AUTH stays the unsupported opcode it is for the GPU
    # server's request parse, whose oracle decode_request is)
    with pytest.raises(ZKDecodeError):
        jute.decode_request(GOLDEN[4:])
    # the type defaults to 0; an ordinary xid is carried as it is
    p = {'xid': 7, 'opcode': 'AUTH', 'scheme': 'digest', 'auth': b'u:pw'}
    assert jute.encode_request(p) == \
        bytes.fromhex('00000007') + GOLDEN[8:]


def test_golden_frame_host_codec(native):
    assert native.encode_request(dict(PKT)) == GOLDEN[4:]
    for p in (PKT,
              {'xid': 7, 'opcode': 'AUTH', 'scheme': 'digest',
               'auth': b'u:pw'},
              {'xid': 0x7fffffff, 'opcode': 'AUTH', 'type': 3,
               'scheme': 'ip', 'auth': b''},
              {'xid': 1, 'opcode': 'AUTH', 'scheme': 'digest',
               'auth': bytes(range(256))}):
        assert native.encode_request(dict(p)) == jute.encode_request(p), p
    with pytest.raises((KeyError, ValueError, TypeError)):
        native.encode_request({'xid': 1, 'opcode': 'AUTH', 'auth': b'x'})


def test_auth_reply_decodes(native):
    for xid, xmap in ((-4, {}), (9, {9: 'AUTH'})):
        for err in ('OK', 'AUTH_FAILED'):
            body = jute.encode_response({'xid': xid, 'zxid': 5, 'err': err,
                                         'opcode': 'AUTH'})
            assert len(body) == 16
            want = {'xid': xid, 'zxid': 5, 'err': err, 'opcode': 'AUTH'}
            assert jute.decode_response(body, xmap) == want
            assert native.decode_response(body, xmap) == want


def _server_ids(zk):
    """The identities of the server's live connections."""
    return zk.run(lambda: [list(c.auth_ids) for c in zk.conns
                           if getattr(c, 'handshook', False) and
                           not c.closed])


def test_add_auth(zk):
    c = client(zk.servers())
    c.wait_connected(10)
    assert c.call_sync('add_auth', 'digest', b'u:pw', timeout=10) is None
    assert _server_ids(zk) == [[U_ID]]
    # the alias, and a str for the credentials
    assert c.call_sync('addAuth', 'digest', 'super:test', timeout=10) is None
    assert _server_ids(zk) == [[U_ID, b'super:D/InIHSb7yEEbrWz8b9l71RjZJU=']]
    # the connection goes on serving
    assert c.call_sync('ping', timeout=10) is None
    c.close_sync(10)


def test_unknown_scheme_fails(zk):
    c = client(zk.servers())
    c.wait_connected(10)
    with pytest.raises(ZKError) as e:
        c.call_sync('add_auth', 'kerberos', b'u:pw', timeout=10)
    assert e.value.code == 'AUTH_FAILED'
    assert _server_ids(zk) == [[]]
    # refused credentials are not remembered, and the connection stays
    assert c._auths == []
    assert c.call_sync('ping', timeout=10) is None
    c.close_sync(10)


def test_credentials_follow_a_reconnect(zk):
    c = client(zk.servers(), session_timeout=4000)
    rec = Recorder(c)
    c.wait_connected(10)
    assert c.call_sync('add_auth', 'digest', b'u:pw', timeout=10) is None
    assert c.call_sync('add_auth', 'digest', b'u:pw', timeout=10) is None
    assert c._auths == [('digest', b'u:pw')]
    accepted = zk.accepted
    zk.drop_connections()
    rec.wait('connect', n=2, timeout=10)
    assert zk.accepted > accepted
    # the new connection starts without an identity; the client adds it
    assert wait_for(lambda: _server_ids(zk) == [[U_ID]], 10), _server_ids(zk)
    assert c.call_sync('ping', timeout=10) is None
    c.close_sync(10)
