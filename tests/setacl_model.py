"""The Python mirror of csrc/kernels/zk_setacl.h: the parse of a SET_ACL
request body, the ADMIN check on the node's current ACL and the precedence of
the answers.  tests/test_setacl_host.py holds the header's host build against
it."""

import struct

import aclperm_model as A
import auth_model as M

SET_ACL = 7
VEC_MAX = 1 << 24
SF_OK, SF_BAD_ARGUMENTS, SF_INVALID_ACL = 0, 1, 2
SA_OPEN, SA_LOST, SA_VECTOR = 0, 1, 2
OK, BAD_ARGUMENTS, NO_NODE, NO_AUTH, BAD_VERSION, INVALID_ACL = \
    0, -8, -101, -102, -103, -114


def body(xid, path, vec, version):
    """A SET_ACL request body (no length prefix); ``vec`` is the wire vector
    (:func:`aclperm_model.vector`)."""
    if isinstance(path, str):
        path = path.encode()
    return struct.pack('>ii', xid, SET_ACL) + A.ustr(path) + vec + \
        struct.pack('>i', version)


def _skip_acl(b, k, count):
    """The end of ``count`` entries from ``k`` in ``b``, or -1."""
    L = len(b)
    for _ in range(count):
        if k + 4 > L:
            return -1
        k += 4
        for _ in range(2):
            if k + 4 > L:
                return -1
            n = max(struct.unpack_from('>i', b, k)[0], 0)
            k += 4 + n
            if k > L:
                return -1
    return k


def parse(b):
    """SET_ACL body ``b`` -> (status, xid, pl, version, poff, voff, vlen):
    zk_setacl.h setacl_frame (offsets relative to the body; -1 none)."""
    L = len(b)
    none = (0, 0, -1, -1, 0)
    if L < 8:
        return (SF_BAD_ARGUMENTS, 0) + none
    xid, op = struct.unpack_from('>ii', b, 0)
    bad = (SF_BAD_ARGUMENTS, xid) + none
    if op != SET_ACL or L < 12:
        return bad
    pl = struct.unpack_from('>i', b, 8)[0]
    k = 12
    if pl < 1 or pl > L - k:
        return bad
    k += pl
    if k + 4 > L:
        return bad
    count = struct.unpack_from('>i', b, k)[0]
    v0 = k
    k += 4
    if count > 0:
        k = _skip_acl(b, k, count)
        if k < 0:
            return bad
    if k + 4 != L:
        return bad
    if count <= 0 or k - v0 >= VEC_MAX:
        return (SF_INVALID_ACL, xid) + none
    return (SF_OK, xid, pl, struct.unpack_from('>i', b, k)[0], 12, v0,
            k - v0)


def admin(kind, vec, addr, ids=None):
    """zk_setacl.h setacl_admin; ``ids`` None: no identity table."""
    if kind == SA_OPEN:
        return True
    if kind != SA_VECTOR:
        return False
    if ids is None:
        return A.permits(vec, A.ADMIN, addr)
    return M.permits_auth(vec, A.ADMIN, addr, ids)


def verdict(status, exists, admin_ok, version, aversion):
    """zk_setacl.h setacl_verdict."""
    if status == SF_BAD_ARGUMENTS:
        return BAD_ARGUMENTS
    if status == SF_INVALID_ACL:
        return INVALID_ACL
    if not exists:
        return NO_NODE
    if not admin_ok:
        return NO_AUTH
    if version != -1 and version != aversion:
        return BAD_VERSION
    return OK


# ---- routing and the front end's cuts (zk_mix.h, zk_front.h) ----------------

WRITES = (1, 2, 5, -11)           # CREATE, DELETE, SET_DATA, CLOSE_SESSION
MIX_A, MIX_C, MIX_L = 0, 1, 2


def mix_class(b, has_acl, setacl):
    """zk_mix.h mix_class (``setacl``: mix_class_setacl) of frame body
    ``b``."""
    if len(b) < 8:
        return MIX_A
    op = struct.unpack_from('>i', b, 4)[0]
    if setacl and has_acl and op == SET_ACL:
        return MIX_C
    if op in (8, 12):
        return MIX_L
    if op == 6 and has_acl:
        return MIX_C
    return MIX_A


def _frames(seg, quota, max_packet):
    """(start, L, opcode word or 0) of the whole frames of ``seg``, then the
    flag of a bad length."""
    p, out = 0, []
    while len(out) < min(quota, 0x7fffffff) and len(seg) - p >= 4:
        L = struct.unpack_from('>i', seg, p)[0]
        if L < 0 or L > max_packet:
            return out, 1
        if L > len(seg) - p - 4:
            break
        out.append((p, L, struct.unpack_from('>i', seg, p + 8)[0]
                    if L >= 8 else 0))
        p += 4 + L
    return out, 0


def walk(seg, quota, max_packet):
    """zk_front.h front_walk_setacl -> (take, nfr, flag)."""
    frames, flag = _frames(seg, quota, max_packet)
    take = nfr = 0
    for p, L, op in frames:
        wr = op in WRITES or op == SET_ACL
        if wr and nfr > 0:
            return take, nfr, 0
        take, nfr = p + 4 + L, nfr + 1
        if wr:
            return take, nfr, 0
    return take, nfr, flag


def walk_ordered(seg, quota, max_packet, has_acl):
    """zk_front.h front_walk_ordered_setacl -> (take, nfr, flag, nwr)."""
    frames, flag = _frames(seg, quota, max_packet)
    take = nfr = nwr = phase = 0
    for p, L, op in frames:
        if op == SET_ACL and nfr > 0:
            return take, nfr, 0, nwr
        if phase == 1 and op in (1, 2, 5):
            return take, nfr, 0, nwr
        if op in (8, 12, 101) or (op == 6 and has_acl):
            phase = 1
        take, nfr = p + 4 + L, nfr + 1
        if op in WRITES:
            nwr += 1
        if op in (-11, SET_ACL):
            return take, nfr, 0, nwr
    return take, nfr, flag, nwr
