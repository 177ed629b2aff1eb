"""Tree images for the reject side of the image tests: one sound image and
its mutations (and a few sound images that are hard on the loader), each
with the outcome ``zkmi.utils.treeimage.check`` must give it (and the device
loader, and — for the structural codes — the stand-alone checker
tools/fuzz_snap.cpp).  Host code only."""

import struct

from treemodel import hash_twin
from zkmi import jute
from zkmi.utils import treeimage as TI

OPEN = [{'perms': ['READ', 'WRITE', 'CREATE', 'DELETE', 'ADMIN'],
         'id': {'scheme': 'world', 'id': 'anyone'}}]
DIGEST_ACL = [{'perms': ['READ'], 'id': {'scheme': 'digest', 'id': 'u:hash'}},
              {'perms': ['READ', 'WRITE'],
               'id': {'scheme': 'ip', 'id': '10.0.0.1'}}]


def rec(path, data=b'', z=1, acl=OPEN, kids=0, owner=0, version=0):
    return {'path': path, 'data': data, 'acl': acl,
            'stat': jute.Stat(z, z + version, 1000 + z, 2000 + z, version,
                              kids, 0, owner, len(data), kids, z + kids)}


def base_records():
    """Two roots, depth three, data of 0 / 5 / 300 bytes, an ephemeral, two
    ACL vectors and a lost binding."""
    return [rec('/a', b'root', 1, kids=2),
            rec('/a/b', b'', 2, kids=1),
            rec('/a/b/c', b'x' * 300, 3, acl=DIGEST_ACL, version=4),
            rec('/a/e', b'hello', 4, owner=0x1234),
            rec('/zz', b'\xff' * 17, 5, acl=None)]


def base_image():
    return TI.pack(base_records(), 77)


def _tab(img, i):
    return struct.unpack_from('<q', img, TI.HEAD + 8 * i)[0]


def _rec_at(img, i):
    """Absolute offset of record i."""
    n = struct.unpack_from('<q', img, 16)[0]
    return TI.HEAD + 8 * (n + 1) + _tab(img, i)


def _put(img, off, fmt, *v):
    b = bytearray(img)
    struct.pack_into(fmt, b, off, *v)
    return bytes(b)


def _acl_off(img, i):
    """Absolute offset of record i's ACL count."""
    o = _rec_at(img, i)
    pl = struct.unpack_from('>i', img, o)[0]
    d = o + 4 + pl + TI.STAT
    dl = struct.unpack_from('>i', img, d)[0]
    return d + 4 + dl


def twin_paths():
    """Three distinct paths under /a with one 64-bit path hash."""
    a = '/a/' + 'T' * 53
    out = (a, hash_twin(a, 5), hash_twin(a, 3, seed=1))
    assert len(set(out)) == 3 and len(a) == 56
    return out


def corpus():
    """[(name, image bytes, (code, index))]; index None: any record of a
    duplicated pair is a right answer."""
    img = base_image()
    recs = base_records()
    n = len(recs)
    out = [('sound', img, (TI.OK, -1)),
           ('empty', TI.pack([], 5), (TI.OK, -1)),
           ('one', TI.pack([rec('/only', b'1')], 9), (TI.OK, -1))]
    # sound, but hard on the loader: two and three distinct paths of ONE
    # 64-bit hash key at adjacent record indices (one wave inserts them: the
    # index build's second launch), and a header whose sizing hints lie
    # (the loader sizes the tree by them, the device never trusts them)
    twins = [rec(p, p[-9:].encode(), 6 + j)
             for j, p in enumerate(twin_paths())]
    out.append(('twins2', TI.pack(recs + twins[:2], 77), (TI.OK, -1)))
    out.append(('twins3', TI.pack(recs + twins, 77), (TI.OK, -1)))
    out.append(('hint-huge', _put(_put(img, 48, '<q', 1 << 62), 56, '<q',
                                  1 << 62), (TI.OK, -1)))
    out.append(('hint-neg', _put(_put(img, 48, '<q', -5), 56, '<q', -1),
                (TI.OK, -1)))
    H, T, R = TI.BAD_HEADER, TI.BAD_TABLE, TI.BAD_RECORD
    # truncation at every header field, inside the table, inside the body
    for cut in (0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 63, 64, 71,
                TI.HEAD + 8 * n, TI.HEAD + 8 * (n + 1) - 1,
                TI.HEAD + 8 * (n + 1), len(img) - 8, len(img) - 1):
        out.append(('cut%d' % cut, img[:cut], (H, -1)))
    out.append(('magic', b'ZKMITREX' + img[8:], (H, -1)))
    out.append(('version', _put(img, 8, '<I', 2), (H, -1)))
    out.append(('n-neg', _put(img, 16, '<q', -1), (H, -1)))
    out.append(('n-min', _put(img, 16, '<q', -(1 << 63)), (H, -1)))
    out.append(('n-past', _put(img, 16, '<q', len(img)), (H, -1)))
    out.append(('n-huge', _put(img, 16, '<q', (1 << 62)), (H, -1)))
    out.append(('body-neg', _put(img, 24, '<q', -8), (H, -1)))
    out.append(('body-odd', _put(img, 24, '<q', _tab(img, n) - 4), (H, -1)))
    out.append(('body-past', _put(img, 24, '<q', _tab(img, n) + 8), (H, -1)))
    # a shorter body than the table ends at
    out.append(('body-short', _put(img, 24, '<q', _tab(img, n) - 8),
                (T, n - 1)))
    out.append(('empty-tab', _put(TI.pack([], 5), TI.HEAD, '<q', 8), (T, 0)))
    # the table
    t2 = TI.HEAD + 8 * 2
    out.append(('tab-first', _put(img, TI.HEAD, '<q', 8), (T, 0)))
    out.append(('tab-decr', _put(img, t2, '<q', _tab(img, 1) - 8), (T, 1)))
    out.append(('tab-equal', _put(img, t2, '<q', _tab(img, 1)), (T, 1)))
    out.append(('tab-unaligned', _put(img, t2, '<q', _tab(img, 2) + 4),
                (T, 1)))
    out.append(('tab-past', _put(img, t2, '<q', _tab(img, n) + 64), (T, 1)))
    out.append(('tab-neg', _put(img, t2, '<q', -(1 << 62)), (T, 1)))
    out.append(('tab-end', _put(img, TI.HEAD + 8 * n, '<q',
                                _tab(img, n) - 8), (T, n - 1)))
    # an aligned but shifted boundary: both neighbours are broken records
    out.append(('tab-shift', _put(img, t2, '<q', _tab(img, 2) + 8), (R, 1)))
    # records
    r2 = _rec_at(img, 2)
    for name, pl in (('pl-0', 0), ('pl-1', 1), ('pl-neg', -5),
                     ('pl-past', 4096), ('pl-max', 0x7fffffff),
                     ('pl-word', 1 << 24)):
        out.append((name, _put(img, r2, '>i', pl), (R, 2)))
    out.append(('no-slash', _put(img, r2 + 4, 'B', 0x61), (R, 2)))
    out.append(('trail-slash', _put(img, r2 + 4 + 5, 'B', 0x2f), (R, 2)))
    d2 = r2 + 4 + 6 + TI.STAT
    for name, dl in (('dl-neg', -1), ('dl-past', 4000),
                     ('dl-max', 0x7fffffff), ('dl-other', 299)):
        out.append((name, _put(img, d2, '>i', dl), (R, 2)))
    out.append(('stat-dl', _put(img, r2 + 4 + 6 + 52, '>i', 301), (R, 2)))
    a2 = _acl_off(img, 2)
    for name, cnt in (('acl-0', 0), ('acl-neg', -2), ('acl-more', 3),
                      ('acl-max', 0x7fffffff)):
        out.append((name, _put(img, a2, '>i', cnt), (R, 2)))
    out.append(('acl-str', _put(img, a2 + 8, '>i', 1 << 20), (R, 2)))
    out.append(('acl-short', _put(img, a2, '>i', 1), (R, 2)))
    out.append(('pad', _put(img, _rec_at(img, 1) - 1, 'B', 7), (R, 0)))
    # a record cut short by its span: the last one's tail dropped
    short = TI.pack(recs, 77)
    short = _put(short[:-8], 24, '<q', _tab(img, n) - 8)
    short = _put(short, TI.HEAD + 8 * n, '<q', _tab(img, n) - 8)
    out.append(('span-short', short, (R, n - 1)))
    # sound records, a bad set
    out.append(('dup', TI.pack(recs + [rec('/a/b', b'again', 9)], 77),
                (TI.DUP_PATH, None)))
    out.append(('orphan', TI.pack(recs + [rec('/a/nobody/kid', b'', 9)], 77),
                (TI.ORPHAN, n)))
    out.append(('orphan-root', TI.pack([rec('/q/r', b'')], 3),
                (TI.ORPHAN, 0)))
    out.append(('digest-bit', _put(img, 40, '<Q',
                                   TI.header(img)['digest'] ^ (1 << 17)),
                (TI.DIGEST, -1)))
    # a changed data byte under an unchanged header digest
    out.append(('data-bit', _put(img, _rec_at(img, 3) + 4 + 4 + TI.STAT + 4,
                                 'B', 0x48), (TI.DIGEST, -1)))
    return out


def stream(images):
    """The corpus file of tools/fuzz_snap.cpp --corpus: per image a
    little-endian u64 length, then its bytes."""
    return b''.join(struct.pack('<Q', len(b)) + b for b in images)
