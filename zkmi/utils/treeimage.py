"""The GPU tree's image (version 1) on the host: build, read and check one
without a GPU.  The layout is csrc/kernels/zk_snap.h's, which this module
mirrors; :meth:`zkmi.server.tree.GpuTree.snapshot` writes such an image
on the device and :meth:`~zkmi.server.tree.GpuTree.load` reads one.

A record is a dict ``{'path': str, 'stat': jute.Stat, 'data': bytes,
'acl': [ACL entries] or None}`` (``None``: the node's ACL binding was lost,
ACL count -1 in the image).  Records keep the order they are given in: a
loaded tree places record ``i`` at node ``i``.  The image holds no watches
and no sessions, and it is not canonical across replicas (two trees with
the same znodes may order them differently): compare replicas by the
header's ``digest``.
"""

import struct

from .. import jute

MAGIC = b'ZKMITREE'
VERSION = 1
HEAD = 64
_HEAD = struct.Struct('<8sIIqqqQqq')
assert _HEAD.size == HEAD
STAT = 68
PATH_MAX = (1 << 24) - 1
ACL_MAX = (1 << 24) - 1

# outcome of a check / load, in check order (zk_snap.h SNAP_*)
(OK, BAD_HEADER, BAD_TABLE, BAD_RECORD, NO_ROOM, DUP_PATH, ORPHAN,
 DIGEST) = range(8)
CODE_NAMES = ('OK', 'BAD_HEADER', 'BAD_TABLE', 'BAD_RECORD', 'NO_ROOM',
              'DUP_PATH', 'ORPHAN', 'DIGEST')

_M64 = (1 << 64) - 1


class TreeImageError(Exception):
    """A refused image: ``code`` (one of the module's outcome codes) and the
    record ``index`` it was found at (-1: none)."""

    def __init__(self, code, index=-1):
        Exception.__init__(self, 'tree image refused: %s at record %d' %
                           (CODE_NAMES[code], index))
        self.code = code
        self.index = index


def _pad8(x):
    return (x + 7) & ~7


def _pad16(x):
    return (x + 15) & ~15


def path_hash(raw):
    """Host mirror of csrc/kernels/zk_tree.h path_hash."""
    n = len(raw)
    h = 0x9E3779B97F4A7C15 ^ n
    for i in range(0, n, 8):
        w = int.from_bytes(raw[i:i + 8], 'little')
        h = ((h ^ w) * 0xFF51AFD7ED558CCD) & _M64
        h ^= h >> 32
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & _M64
    h ^= h >> 33
    return h


def node_digest(path, stat, data):
    """One znode's term of the tree digest (tree.hip tree_digest_k): path,
    czxid, mzxid, version, cversion | numChildren, pzxid, ephemeralOwner and
    data; the times and aversion stay out."""
    h = path_hash(path)

    def mix(x):
        nonlocal h
        h = ((h ^ (x & _M64)) * 0x9E3779B97F4A7C15) & _M64
        h ^= h >> 29

    mix(stat.czxid)
    mix(stat.mzxid)
    mix(stat.version & 0xffffffff)
    mix((stat.cversion & 0xffffffff) << 32 | (stat.numChildren & 0xffffffff))
    mix(stat.pzxid)
    mix(stat.ephemeralOwner)
    mix(len(data))
    mix(path_hash(data))
    return h


def _path_bytes(p):
    return p.encode('utf-8', 'surrogateescape') if isinstance(p, str) \
        else bytes(p)


def digest(records):
    """The ``tree_digest`` sum of exactly ``records`` (mod 2^64)."""
    d = 0
    for r in records:
        d += node_digest(_path_bytes(r['path']), r['stat'], r['data'] or b'')
    return d & _M64


def _record(r):
    w = jute.JuteWriter()
    p = _path_bytes(r['path'])
    data = r['data'] or b''
    w.write_int(len(p))
    w.buf += p
    w.write_stat(r['stat'])
    w.write_int(len(data))
    w.buf += data
    if r['acl'] is None:
        w.write_int(-1)
    else:
        w.write_acl(r['acl'])
    w.buf += b'\0' * (_pad8(len(w.buf)) - len(w.buf))
    return bytes(w.buf)


def pack(records, zxid):
    """The image of ``records`` (in their order) at ``zxid``, as bytes."""
    recs = [_record(r) for r in records]
    offs, o = [0], 0
    for b in recs:
        o += len(b)
        offs.append(o)
    head = _HEAD.pack(
        MAGIC, VERSION, 0, len(recs), o, zxid, digest(records),
        sum(_pad16(len(_path_bytes(r['path']))) for r in records),
        max([len(r['data'] or b'') for r in records] or [0]))
    return head + struct.pack('<%dq' % len(offs), *offs) + b''.join(recs)


def header(image):
    """The header fields of ``image`` as a dict (no check but its length
    and magic)."""
    image = bytes(image[:HEAD])
    if len(image) < HEAD:
        raise TreeImageError(BAD_HEADER)
    magic, ver, _, n, body, zxid, dig, path16, max_data = _HEAD.unpack(image)
    if magic != MAGIC:
        raise TreeImageError(BAD_HEADER)
    return {'version': ver, 'n': n, 'body_bytes': body, 'zxid': zxid,
            'digest': dig, 'path16': path16, 'max_data': max_data}


def _skip_strings(b, k, end, count):
    for _ in range(count):
        if k + 4 > end:
            return -1
        ln = struct.unpack_from('>i', b, k)[0]
        k += 4 + max(ln, 0)
        if k > end:
            return -1
    return k


def _skip_acl(b, k, end, count):
    for _ in range(count):
        if k + 4 > end:
            return -1
        k = _skip_strings(b, k + 4, end, 2)
        if k < 0:
            return -1
    return k


def _parse_record(b, a, e):
    """Field offsets of the record b[a:e] as zk_snap.h snap_check_record
    finds them — (path, stat, data, acl offset, acl bytes, acl count) — or
    None when it refuses the record."""
    k = a
    if k + 4 > e:
        return None
    pl = struct.unpack_from('>i', b, k)[0]
    k += 4
    if pl < 2 or pl > PATH_MAX or k + pl > e:
        return None
    if b[k] != 0x2f or b[k + pl - 1] == 0x2f:
        return None
    path = (k, pl)
    k += pl
    if k + STAT > e:
        return None
    stat = k
    k += STAT
    if k + 4 > e:
        return None
    dl = struct.unpack_from('>i', b, k)[0]
    k += 4
    if dl < 0 or k + dl > e:
        return None
    if struct.unpack_from('>i', b, stat + 52)[0] != dl:
        return None
    data = (k, dl)
    k += dl
    if k + 4 > e:
        return None
    cnt = struct.unpack_from('>i', b, k)[0]
    acl = k
    k += 4
    if cnt < -1 or cnt == 0:
        return None
    if cnt > 0:
        k = _skip_acl(b, k, e, cnt)
        if k < 0 or k - acl > ACL_MAX:
            return None
    if _pad8(k - a) != e - a or any(b[k:e]):
        return None
    return path, stat, data, acl, k - acl, cnt


def _structure(image):
    """(code, index, header, spans): the header, table and record checks."""
    b = bytes(image)
    if len(b) < HEAD:
        return BAD_HEADER, -1, None, None
    magic, ver, _, n, body, zxid, dig, path16, max_data = \
        _HEAD.unpack_from(b)
    if magic != MAGIC or ver != VERSION:
        return BAD_HEADER, -1, None, None
    room = len(b) - HEAD
    if n < 0 or n > room // 8 - 1:
        return BAD_HEADER, -1, None, None
    left = room - 8 * (n + 1)
    if body < 0 or body & 7 or body > left:
        return BAD_HEADER, -1, None, None
    offs = struct.unpack_from('<%dq' % (n + 1), b, HEAD)
    if n == 0:
        if body != 0:
            return BAD_HEADER, -1, None, None
        if offs[0] != 0:
            return BAD_TABLE, 0, None, None
    for i in range(n):
        lo, hi = offs[i], offs[i + 1]
        if (i == 0 and lo != 0) or (i == n - 1 and hi != body) or \
                (lo | hi) & 7 or not 0 <= lo < hi <= body:
            return BAD_TABLE, i, None, None
    base = HEAD + 8 * (n + 1)
    spans = []
    for i in range(n):
        f = _parse_record(b, base + offs[i], base + offs[i + 1])
        if f is None:
            return BAD_RECORD, i, None, None
        spans.append(f)
    hd = {'version': ver, 'n': n, 'body_bytes': body, 'zxid': zxid,
          'digest': dig, 'path16': path16, 'max_data': max_data}
    return OK, -1, hd, spans


def _records(b, spans, acls=True):
    out = []
    for (po, pl), st, (do, dl), ao, al, cnt in spans:
        r = jute.JuteReader(b, st, st + STAT)
        acl = None if cnt < 0 or not acls else \
            jute.JuteReader(b, ao, ao + al).read_acl()
        out.append({'path': b[po:po + pl].decode('utf-8', 'surrogateescape'),
                    'stat': r.read_stat(), 'data': b[do:do + dl],
                    'acl': acl})
    return out


def unpack(image):
    """(header dict, records) of a structurally sound image; raises
    :class:`TreeImageError` otherwise.  Duplicates, orphans and the digest
    are :func:`check`'s."""
    b = bytes(image)
    code, index, hd, spans = _structure(b)
    if code != OK:
        raise TreeImageError(code, index)
    return hd, _records(b, spans)


def check(image):
    """The ``(code, index)`` the loader reports for ``image``, NO_ROOM
    aside (that depends on the tree): the earliest failing phase and the
    smallest record index failing in it.  For DUP_PATH the index is the
    second record of the first duplicated path (the loader may report
    either record of a pair)."""
    b = bytes(image)
    code, index, hd, spans = _structure(b)
    if code != OK:
        return code, index
    paths = [b[po:po + pl] for (po, pl), *_ in spans]
    seen = {}
    for i, p in enumerate(paths):
        if p in seen:
            return DUP_PATH, i
        seen[p] = i
    for i, p in enumerate(paths):
        cut = p.rfind(b'/')
        if cut > 0 and p[:cut] not in seen:
            return ORPHAN, i
    if digest(_records(b, spans, acls=False)) != hd['digest']:
        return DIGEST, -1
    return OK, -1
