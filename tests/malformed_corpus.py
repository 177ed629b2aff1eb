"""Malformed-wire corpora for the differential decode tests: reply and
request bodies generated from a fixed seed with the Jute oracle
(zkmi/jute.py), one mutation a body or none, and the oracle's verdict on
each — what the GPU decoders (tests/test_gpu_decode_malformed.py) and the
device request parser built for the host (tests/test_parse_host.py) must
agree with."""

import random
import struct

from zkmi import consts, jute
from zkmi.errors import ZKDecodeError
from zkmi.utils import synth

N_FRAMES = 256 * 16 + 37     # several workgroups, a ragged last block
XID_BITS = 13                # the reply corpus' xid table: 8192 > N_FRAMES

ST_OK, ST_BAD_DECODE, ST_NO_XID, ST_BAD_OPCODE = 0, 1, 2, 3
SKIP = -1                    # text-only rejection: left out of the comparison

WORDS = (-1, -2**31, 0, 1, 3, 5, 17, 67, 68, 69, 0x7f, 0x100, 0x7f7f,
         0x10000, 0x7f000000, 0x7fffffff)
BAD_REQ_OPS = (7, 13, 14, 100, 9999)
BAD_TABLE_OPS = ('SET_ACL', 'CHECK', 'MULTI')

_REPLY_OPS = ('GET_DATA', 'EXISTS', 'SET_DATA', 'CREATE', 'GET_CHILDREN',
              'GET_CHILDREN2', 'GET_ACL', 'DELETE', 'SYNC')
_NAME = 'abcdefghij0123456789_-'


def _low_bytes(r, n):
    return bytes(r.randrange(0x80) for _ in range(n))


def _stat(r):
    """A Stat whose 68 wire bytes are all below 0x80."""
    return jute.JuteReader(_low_bytes(r, consts.STAT_SIZE)).read_stat()


def _name(r):
    return ''.join(r.choice(_NAME) for _ in range(r.randint(1, 12)))


def _acl(r):
    return [{'perms': [p for p in consts.PERM_MASKS if r.random() < 0.6]
             or ['READ'],
             'id': {'scheme': r.choice(['world', 'digest', 'ip']),
                    'id': r.choice(['anyone', 'u:x', '10.0.0.1', ''])}}
            for _ in range(r.randint(0, 3))]


def _overwrite(r, body, lo):
    """One 4-byte word at a random byte offset >= lo (None: too short)."""
    if len(body) < lo + 4:
        return None
    at = r.randint(lo, len(body) - 4)
    return body[:at] + struct.pack('>i', r.choice(WORDS)) + body[at + 4:]


def _truncate(r, body, small):
    """Cut to a random length below the body's; three in ten below
    ``small`` bytes (inside the header)."""
    if not body:
        return None
    hi = len(body) - 1
    return body[:r.randint(0, min(small - 1, hi) if r.random() < 0.3 else hi)]


def _trail(r, body):
    return body + _low_bytes(r, r.randint(1, 80))


# ---------------------------------------------------------------- replies

class ReplyCorpus(object):
    """``bodies[i]``: reply i's bytes; ``kind[i]``: its mutation ('' none);
    ``xid_map``: xid -> opcode name, as the encoder recorded them (the
    oracle's map, and with ``table()`` the kernel's); ``chk_idx`` /
    ``chk_xid``: the request the fused GET check holds reply i against
    (node, xid); ``chk_rows``: the unmutated GET_DATA replies built to
    pass it."""

    def __init__(self, seed=1, n=N_FRAMES, nodes=None):
        """``nodes = (first, last, data_len)``: GET_DATA replies of tree
        nodes first..last (czxid node + 1, ``data_len`` bytes) are mixed
        in for the fused check; last + 1 < 128, so their Stats keep to
        bytes below 0x80."""
        r = random.Random(seed)
        self.bodies, self.kind, self.xid_map = [], [], {}
        self.chk_idx, self.chk_xid, self.chk_rows = [], [], []
        for i in range(n):
            xid = i
            rep, node = self._reply(r, xid, nodes)
            op = rep['opcode']
            if rep['xid'] >= 0:
                self.xid_map[xid] = op
            body = jute.encode_response(rep)
            kind, body = self._mutate(r, body, xid, rep)
            self.bodies.append(body)
            self.kind.append(kind)
            clean = kind == '' and node is not None
            self.chk_idx.append(node if clean else 0)
            self.chk_xid.append(xid)
            if clean:
                self.chk_rows.append(i)

    @staticmethod
    def _reply(r, xid, nodes):
        u = r.random()
        err = 'OK' if r.random() < 0.85 else r.choice(
            ['NO_NODE', 'NODE_EXISTS', 'BAD_VERSION', -77])
        zxid = r.randint(0, 2**48)
        if u < 0.08:
            return {'xid': -1, 'zxid': -1, 'err': 'OK',
                    'opcode': 'NOTIFICATION',
                    'type': r.choice(list(consts.NOTIFICATION_TYPE) + [9]),
                    'state': r.choice(list(consts.STATE) + [7]),
                    'path': '/' + _name(r)}, None
        if u < 0.12:
            sx = r.choice([-2, -4, -8])
            return {'xid': sx, 'zxid': zxid, 'err': err,
                    'opcode': consts.SPECIAL_XIDS[sx]}, None
        if nodes is not None and u < 0.27:
            v = r.randint(nodes[0], nodes[1])
            st = _stat(r)
            st.czxid = v + 1
            return {'xid': xid, 'zxid': zxid, 'err': 'OK',
                    'opcode': 'GET_DATA', 'data': _low_bytes(r, nodes[2]),
                    'stat': st}, v
        op = r.choice(_REPLY_OPS)
        rep = {'xid': xid, 'zxid': zxid, 'err': err, 'opcode': op}
        if op == 'GET_DATA':
            rep['data'] = _low_bytes(r, r.choice([0, 1, r.randint(0, 64)]))
            rep['stat'] = _stat(r)
        elif op in ('EXISTS', 'SET_DATA'):
            rep['stat'] = _stat(r)
        elif op == 'CREATE':
            rep['path'] = '/' + _name(r)
        elif op in ('GET_CHILDREN', 'GET_CHILDREN2'):
            rep['children'] = [_name(r) for _ in range(r.randint(0, 5))]
            rep['stat'] = _stat(r)
        elif op == 'GET_ACL':
            rep['acl'] = _acl(r)
            rep['stat'] = _stat(r)
        return rep, None

    def _mutate(self, r, body, xid, rep):
        u = r.random()
        if u < 0.40:
            return '', body
        special = rep['xid'] < 0
        if u < 0.58:
            m = _overwrite(r, body, 16)
            return ('', body) if m is None else ('word', m)
        if u < 0.74:
            return 'cut', _truncate(r, body, 16)
        if u < 0.84:
            return 'trail', _trail(r, body)
        if special:
            return '', body
        if u < 0.88:                      # no such request
            return 'absent', struct.pack('>i', 20000 + xid) + body[4:]
        if u < 0.92:                      # its slot holds another xid
            return 'alias', struct.pack('>i', xid + (1 << XID_BITS)) + \
                body[4:]
        if u < 0.96:                      # negative, not a special xid
            return 'negative', struct.pack(
                '>i', r.choice([-3, -5, -2**31])) + body[4:]
        self.xid_map[xid] = r.choice(BAD_TABLE_OPS)
        return 'badop', body

    def table(self):
        """The xid table's (slot, entry) pairs for ``xid_map``."""
        mask = (1 << XID_BITS) - 1
        return [(x & mask, (x << 32) | (consts.OP_CODES[op] & 0xffffffff))
                for x, op in self.xid_map.items()]

    def stream(self):
        return b''.join(jute.frame(b) for b in self.bodies)

    def expect(self, i):
        return expect_reply(self.bodies[i], self.xid_map)


def expect_reply(body, xid_map):
    """(status, packet) the oracle gives a reply body: (0, packet), (ST_*,
    None), or (SKIP, None) when only its text check refuses the body."""
    try:
        return ST_OK, jute.decode_response(body, xid_map)
    except UnicodeDecodeError:
        return SKIP, None
    except ZKDecodeError as e:
        msg = str(e)
        if 'must match a request' in msg:
            return ST_NO_XID, None
        if 'Unsupported opcode' in msg:
            return ST_BAD_OPCODE, None
        assert 'shorter than' in msg or 'overruns' in msg, msg
        return ST_BAD_DECODE, None


def short_stat_after_names(body, xid_map):
    """Is ``body`` a GET_CHILDREN2 success whose names parse and whose Stat
    is cut short (the row decode_replies_k used to leave half filled)?"""
    if len(body) < 16:
        return False
    xid, _, err = struct.unpack_from('>iqi', body, 0)
    if xid_map.get(xid) != 'GET_CHILDREN2' or err != 0:
        return False
    rd = jute.JuteReader(body, 16)
    try:
        n = rd.read_int()
        for _ in range(max(n, 0)):
            rd.read_buffer()
    except ZKDecodeError:
        return False
    return rd.end - rd.off < consts.STAT_SIZE


# --------------------------------------------------------------- requests

def _set_watches(r, xid):
    return {'xid': xid, 'opcode': 'SET_WATCHES',
            'relZxid': r.randint(0, 2**48),
            'events': {k: ['/' + _name(r) for _ in range(r.randint(0, 3))]
                       for k in ('dataChanged', 'createdOrDestroyed',
                                 'childrenChanged')}}


def _put(body, at, fmt, v):
    return body[:at] + struct.pack(fmt, v) + body[at + struct.calcsize(fmt):]


def _mutate_request(r, p, body):
    op = p['opcode']
    u = r.random()
    if u < 0.36:
        return '', body
    if u < 0.50:
        m = _overwrite(r, body, 8)
        return ('', body) if m is None else ('word', m)
    if u < 0.62:
        return 'cut', _truncate(r, body, 8)
    if u < 0.70:
        return 'trail', _trail(r, body)
    if u < 0.78:
        return 'op', _put(body, 4, '>i', r.choice(BAD_REQ_OPS))
    if u < 0.82:
        return 'tiny', body[:r.randint(0, 7)]
    pl = len(p['path'].encode()) if 'path' in p else 0
    if op in ('GET_DATA', 'EXISTS', 'GET_CHILDREN', 'GET_CHILDREN2'):
        return 'watch', body[:-1] + bytes([r.choice([2, 0xff])])
    if op == 'CREATE':
        d = len(p['data'])
        if r.random() < 0.5:
            return 'acl', _put(body, 12 + pl + 4 + d, '>i',
                               r.choice([-1, -7, -2**31]))
        return 'neglen', _put(body, r.choice([8, 12 + pl]), '>i',
                              r.choice([-1, -5, -2**31]))
    if op == 'SET_DATA':
        return 'neglen', _put(body, r.choice([8, 12 + pl]), '>i',
                              r.choice([-1, -5, -2**31]))
    if op in ('DELETE', 'GET_ACL', 'SYNC'):
        return 'neglen', _put(body, 8, '>i', r.choice([-1, -5, -2**31]))
    if op == 'SET_WATCHES':
        # cut inside the second or the third list
        ev = p['events']
        w = jute.JuteWriter()
        w.write_string_vector(ev['dataChanged'])
        a = 16 + len(w.getvalue())
        w = jute.JuteWriter()
        w.write_string_vector(ev['createdOrDestroyed'])
        b = a + len(w.getvalue())
        lo, hi = r.choice([(a, b - 1), (b, len(body) - 1)])
        return 'lists', body[:r.randint(lo, hi)]
    return '', body


class RequestCorpus(object):
    """``bodies[i]`` / ``kind[i]`` as in :class:`ReplyCorpus`; ``ops[i]``
    the opcode name the body was generated as."""

    def __init__(self, seed=2, n=N_FRAMES):
        r = random.Random(seed)
        self.bodies, self.kind, self.ops = [], [], []
        for i in range(n):
            xid = r.choice([i, i, r.randint(-2**31, 2**31 - 1)])
            p = _set_watches(r, xid) if r.random() < 0.12 else \
                synth.rand_request(r, xid)
            kind, body = _mutate_request(r, p, jute.encode_request(p))
            self.bodies.append(body)
            self.kind.append(kind)
            self.ops.append(p['opcode'])

    def stream(self):
        return b''.join(jute.frame(b) for b in self.bodies)


def expect_request(body):
    """(status, fields) the oracle gives a request body.  ``fields``: xid,
    op, path / data bytes (None: the op has none), arg (watch, version or
    the create flags as names), vec_count (ACL entries; SET_WATCHES paths)
    and rel_zxid."""
    try:
        w = jute.decode_request(body)
    except UnicodeDecodeError:
        return SKIP, None
    except ZKDecodeError as e:
        if 'Unsupported opcode' in str(e):
            return ST_BAD_OPCODE, None
        return ST_BAD_DECODE, None
    f = {'xid': w['xid'], 'op': consts.OP_CODES[w['opcode']],
         'path': w['path'].encode() if 'path' in w else None,
         'data': w.get('data'), 'arg': None, 'flags': None, 'vec_count': 0,
         'rel_zxid': w.get('relZxid', 0)}
    if 'watch' in w:
        f['arg'] = int(w['watch'])
    elif 'version' in w:
        f['arg'] = w['version']
    if w['opcode'] == 'CREATE':
        f['flags'] = w['flags']
        f['vec_count'] = len(w['acl'])
    elif w['opcode'] == 'SET_WATCHES':
        f['vec_count'] = sum(len(v) for v in w['events'].values())
    return ST_OK, f


def check_request_row(body, base, row, want):
    """Assert one decoded request row (dict of the K12 columns, offsets
    absolute in a stream where the body starts at ``base``) against
    ``want`` = :func:`expect_request`'s fields."""
    assert row['status'] == ST_OK
    assert row['xid'] == want['xid'] and row['opcode'] == want['op']

    def cut(off, ln):
        assert base <= off and off + ln <= base + len(body) and ln >= 0
        return body[off - base:off - base + ln]
    if want['path'] is not None:
        assert cut(row['path_off'], row['path_len']) == want['path']
    if want['data'] is not None:
        assert cut(row['data_off'], row['data_len']) == want['data']
    if want['arg'] is not None:
        assert row['arg'] == want['arg']
    if want['flags'] is not None:
        assert jute.mask_to_flags(row['arg']) == want['flags']
    assert row['vec_count'] == want['vec_count']
    assert row['rel_zxid'] == want['rel_zxid']


def stats(statuses):
    """Share of each verdict in a list of oracle statuses."""
    n = float(len(statuses))
    return {k: sum(1 for s in statuses if s == k) / n
            for k in (SKIP, ST_OK, ST_BAD_DECODE, ST_NO_XID, ST_BAD_OPCODE)}
