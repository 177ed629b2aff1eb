"""The tree image's host codec (zkmi/utils/treeimage.py): pack / unpack,
the digest's host mirror, and check() on the mutation corpus of
tests/image_corpus.py.  No GPU."""

import struct

import pytest

import image_corpus as C
from treemodel import _Loop
from zkmi import jute
from zkmi.server.fakezk import ZKDatabase
from zkmi.utils import treeimage as TI


def db_records(db):
    """A ZKDatabase's znodes ('/' aside, which a tree has no node for) as
    image records, parents before children."""
    return [{'path': p, 'stat': n.stat, 'data': bytes(n.data or b''),
             'acl': n.acl}
            for p, n in sorted(db.nodes.items()) if p != '/']


def _same(a, b):
    assert [r['path'] for r in a] == [r['path'] for r in b]
    for x, y in zip(a, b):
        assert x['stat'].as_tuple() == y['stat'].as_tuple(), x['path']
        assert bytes(x['data'] or b'') == y['data'], x['path']
        if x['acl'] is None:
            assert y['acl'] is None
        else:
            w, v = jute.JuteWriter(), jute.JuteWriter()
            w.write_acl(x['acl'])
            v.write_acl(y['acl'])
            assert w.getvalue() == v.getvalue(), x['path']


def test_pack_unpack_round_trip():
    recs = C.base_records()
    img = TI.pack(recs, 77)
    hd, got = TI.unpack(img)
    _same(recs, got)
    assert hd['n'] == len(recs) and hd['zxid'] == 77 and hd['version'] == 1
    assert hd['digest'] == TI.digest(recs) == TI.digest(got)
    assert hd['path16'] == sum((len(r['path']) + 15) & ~15 for r in recs)
    assert hd['max_data'] == 300
    assert TI.pack(got, 77) == img
    assert TI.check(img) == (TI.OK, -1)


def test_layout():
    img = C.base_image()
    n = len(C.base_records())
    assert img[:8] == b'ZKMITREE'
    assert struct.unpack_from('<I', img, 8)[0] == 1
    offs = struct.unpack_from('<%dq' % (n + 1), img, 64)
    assert offs[0] == 0 and offs[-1] == TI.header(img)['body_bytes']
    assert all(o % 8 == 0 for o in offs)
    assert all(a < b for a, b in zip(offs, offs[1:]))
    assert len(img) == 64 + 8 * (n + 1) + offs[-1]
    body = img[64 + 8 * (n + 1):]
    # record 0: be32 path_len, path, Stat, be32 data_len, data, open ACL
    assert body[:6] == b'\0\0\0\x02/a'
    assert body[6:74] == C.base_records()[0]['stat'].to_bytes()
    assert body[74:82] == b'\0\0\0\x04root'
    assert body[82:86] == b'\0\0\0\x01'
    # a lost binding is count -1 (the last record: 100 bytes, padded to 104)
    assert img[-8:] == b'\xff\xff\xff\xff\0\0\0\0'


def test_digest_is_order_independent_and_sensitive():
    recs = C.base_records()
    d = TI.digest(recs)
    assert TI.digest(recs[::-1]) == d
    recs[2]['data'] = b'y' + recs[2]['data'][1:]
    assert TI.digest(recs) != d


@pytest.mark.parametrize('name,img,want',
                         C.corpus(), ids=[c[0] for c in C.corpus()])
def test_check_corpus(name, img, want):
    code, index = TI.check(img)
    assert code == want[0], (name, TI.CODE_NAMES[code], index)
    if want[1] is not None:
        assert index == want[1], (name, index)
    else:
        assert index in (1, 5)
    if code <= TI.BAD_RECORD and code != TI.OK:
        with pytest.raises(TI.TreeImageError) as e:
            TI.unpack(img)
        assert (e.value.code, e.value.index) == (code, index)


def test_corpus_covers_every_structural_code():
    seen = {c[2][0] for c in C.corpus()}
    assert seen == {TI.OK, TI.BAD_HEADER, TI.BAD_TABLE, TI.BAD_RECORD,
                    TI.DUP_PATH, TI.ORPHAN, TI.DIGEST}


def test_database_round_trip():
    db = ZKDatabase(_Loop())
    world = [db._world()]
    sid = db.new_session(30000).sid
    for top in ('/app', '/cfg'):
        db.create(top, b'top', world, [], None)
    for k in range(12):
        db.create('/app/n%02d' % k, b'd' * (k * 7), world, [], None)
    db.create('/app/n03/deep', b'', C.DIGEST_ACL, [], None)
    db.create('/app/n03/deep/er', b'x' * 300, world, [], None)
    db.create('/cfg/eph', b'e', world, ['EPHEMERAL'], sid)
    db.create('/cfg/seq-', b's', world, ['SEQUENTIAL'], None)
    db.set_data('/app/n05', b'changed', 0)
    db.set_data('/app/n05', b'', 1)
    for k in (1, 4, 7):
        db.delete('/app/n%02d' % k, -1, None)
    db.create('/app/n04', b'again', world, [], None)
    recs = db_records(db)
    img = TI.pack(recs, db.zxid)
    assert TI.check(img) == (TI.OK, -1)
    hd, got = TI.unpack(img)
    assert hd['zxid'] == db.zxid and hd['n'] == len(db.nodes) - 1
    _same(recs, got)
    by = {r['path']: r for r in got}
    assert by['/cfg/eph']['stat'].ephemeralOwner == sid
    assert by['/app/n05']['stat'].version == 2
    assert by['/app/n05']['data'] == b''
    assert '/app/n01' not in by and by['/app/n04']['data'] == b'again'
    assert by['/app']['stat'].numChildren == 10
