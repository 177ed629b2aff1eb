"""SET_ACL on the wire: ``SetACLRequest {ustring path; vector<ACL> acl; int
version}`` and ``SetACLResponse {Stat stat}`` in the Jute oracle
(zkmi/jute.py) and in the native host codec (csrc/host/zk_host_codec.cpp),
byte for byte the same in both directions, and every truncation of a request
rejected by the oracle's server-mode decode and by the GPU rule's mirror
(tests/setacl_model.py)."""

import os
import struct
import sys

import pytest

from zkmi import consts, jute
from zkmi.errors import ZKDecodeError

import setacl_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ACL2 = [{'perms': ['READ'], 'id': {'scheme': 'world', 'id': 'anyone'}},
        {'perms': ['READ', 'WRITE', 'CREATE', 'DELETE', 'ADMIN'],
         'id': {'scheme': 'digest', 'id': 'u:BvFaefuhWURhnvpD7ipe45CKTpk='}}]
PKT = {'xid': 5, 'opcode': 'SET_ACL', 'path': '/a', 'acl': ACL2, 'version': 3}
# xid 5, opcode 7, path '/a', two entries, version 3
GOLDEN = bytes.fromhex('00000005' '00000007' '00000002') + b'/a' + \
    bytes.fromhex('00000002'
                  '00000001' '00000005') + b'world' + \
    bytes.fromhex('00000006') + b'anyone' + \
    bytes.fromhex('0000001f' '00000006') + b'digest' + \
    bytes.fromhex('0000001e') + b'u:BvFaefuhWURhnvpD7ipe45CKTpk=' + \
    bytes.fromhex('00000003')
STAT = jute.Stat(3, 9, 1700000000000, 1700000000001, 4, 5, 6, 0, 7, 8, 10)

PACKETS = [
    PKT,
    {'xid': 1, 'opcode': 'SET_ACL', 'path': '/', 'acl': [], 'version': -1},
    {'xid': 0x7fffffff, 'opcode': 'SET_ACL', 'path': '/x/' + 'y' * 300,
     'acl': [dict(a) for a in jute.DEFAULT_ACL], 'version': 0},
    {'xid': 2, 'opcode': 'SET_ACL', 'path': '/é', 'version': 2 ** 31 - 1,
     'acl': [{'perms': ['ADMIN'], 'id': {'scheme': 'ip',
                                         'id': '10.1.2.0/24'}}] * 3},
    # perms as a mask, lower-case names, empty strings (written as -1)
    {'xid': 3, 'opcode': 'SET_ACL', 'path': '/a', 'version': -1,
     'acl': [{'perms': 31, 'id': {'scheme': '', 'id': ''}},
             {'perms': ['read', 'admin'],
              'id': {'scheme': 'auth', 'id': ''}}]},
]


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


def _canon(pkt):
    """``pkt`` as decode_request returns it: upper-case perm names."""
    p = dict(pkt)
    p['acl'] = [{'perms': [k for k, m in consts.PERM_MASKS.items()
                           if jute.perms_to_mask(a['perms']) & m],
                 'id': dict(a['id'])} for a in pkt.get('acl', [])]
    return p


def test_request_round_trip_jute():
    assert jute.encode_request(dict(PKT)) == GOLDEN
    assert jute.decode_request(GOLDEN, set_acl=True) == PKT
    # (without the flag SET_ACL stays the unsupported opcode it is for the
    # GPU server's request parse, whose oracle decode_request is)
    with pytest.raises(ZKDecodeError):
        jute.decode_request(GOLDEN)
    for p in PACKETS:
        body = jute.encode_request(dict(p))
        assert jute.decode_request(body, set_acl=True) == _canon(p), p
    # the version defaults to -1, as SET_DATA's
    p = {'xid': 5, 'opcode': 'SET_ACL', 'path': '/a', 'acl': ACL2}
    assert jute.encode_request(p) == GOLDEN[:-4] + b'\xff\xff\xff\xff'


def test_reply_round_trip_jute():
    ok = {'xid': 5, 'zxid': 77, 'err': 'OK', 'opcode': 'SET_ACL',
          'stat': STAT}
    body = jute.encode_response(ok)
    assert len(body) == 16 + consts.STAT_SIZE
    assert body == struct.pack('>iqi', 5, 77, 0) + STAT.to_bytes()
    assert jute.decode_response(body, {5: 'SET_ACL'}, set_acl=True) == ok
    # (without the flag it stays the unsupported opcode it is for the GPU
    # reply decoders, whose oracle decode_response is; the client's codec
    # decodes it)
    with pytest.raises(ZKDecodeError):
        jute.decode_response(body, {5: 'SET_ACL'})
    from zkmi import codec
    assert codec.decode_response(body, {5: 'SET_ACL'}) == ok
    for err in ('NO_NODE', 'NO_AUTH', 'BAD_VERSION', 'INVALID_ACL'):
        rep = {'xid': 5, 'zxid': 77, 'err': err, 'opcode': 'SET_ACL'}
        body = jute.encode_response(dict(rep, stat=STAT))
        assert len(body) == 16
        assert jute.decode_response(body, {5: 'SET_ACL'}, set_acl=True) == rep
    # an OK reply without its Stat does not decode
    with pytest.raises(ZKDecodeError):
        jute.decode_response(jute.encode_response(ok)[:-1], {5: 'SET_ACL'},
                             set_acl=True)


def test_request_parity_host_codec(native):
    assert native.encode_request(dict(PKT)) == GOLDEN
    for p in PACKETS:
        assert native.encode_request(dict(p)) == jute.encode_request(p), p
    p = {'xid': 5, 'opcode': 'SET_ACL', 'path': '/a', 'acl': ACL2}
    assert native.encode_request(dict(p)) == jute.encode_request(p)
    with pytest.raises((KeyError, ValueError, TypeError)):
        native.encode_request({'xid': 1, 'opcode': 'SET_ACL', 'path': '/a',
                               'acl': [{'perms': ['NOPE'], 'id': {
                                   'scheme': 'world', 'id': 'anyone'}}]})


def test_reply_parity_host_codec(native):
    xmap = {5: 'SET_ACL'}
    ok = {'xid': 5, 'zxid': 77, 'err': 'OK', 'opcode': 'SET_ACL',
          'stat': STAT}
    body = jute.encode_response(ok)
    assert native.decode_response(body, xmap) == ok == \
        jute.decode_response(body, xmap, set_acl=True)
    for err in ('NO_NODE', 'NO_AUTH', 'BAD_VERSION', 'INVALID_ACL',
                'SYSTEM_ERROR'):
        body = jute.encode_response({'xid': 5, 'zxid': 1, 'err': err,
                                     'opcode': 'SET_ACL'})
        assert native.decode_response(body, xmap) == \
            jute.decode_response(body, xmap, set_acl=True)
    # every truncation of the reply: both refuse it
    body = jute.encode_response(ok)
    for k in range(len(body)):
        with pytest.raises(ZKDecodeError):
            jute.decode_response(body[:k], xmap, set_acl=True)
        with pytest.raises(ZKDecodeError):
            native.decode_response(body[:k], xmap)


def test_every_truncation_of_a_request_is_rejected():
    for p in PACKETS:
        body = jute.encode_request(dict(p))
        for k in range(len(body)):
            with pytest.raises(ZKDecodeError):
                jute.decode_request(body[:k], set_acl=True)
            assert S.parse(body[:k])[0] == S.SF_BAD_ARGUMENTS, (p, k)
    # the whole frames: the oracle and the rule's mirror see the same fields
    for p in PACKETS:
        body = jute.encode_request(dict(p))
        st, xid, pl, version, poff, voff, vlen = S.parse(body)
        if not p['acl']:
            assert st == S.SF_INVALID_ACL
            continue
        assert st == S.SF_OK and xid == p['xid'] and version == p['version']
        assert body[poff:poff + pl].decode('utf-8') == p['path']
        r = jute.JuteReader(body, voff, voff + vlen)
        assert r.read_acl() == _canon(p)['acl'] and r.at_end()
