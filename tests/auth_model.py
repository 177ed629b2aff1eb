"""The Python mirror of csrc/kernels/zk_auth.h: the parse of an AUTH request
body, ZooKeeper's digest identity (``hashlib`` and ``base64`` are the
reference), the ACL walk with ``digest`` entries, and the identity table of a
batch's connections.  tests/test_auth_host.py holds the header's host build
against it, tests/test_gpu_auth.py the kernels."""

import base64
import hashlib
import struct

import aclperm_model as A

AUTH = 100
AUTH_MAX = 119
AUTH_K = 4
AUTH_FAILED = -115
AF_OK, AF_MALFORMED, AF_SCHEME, AF_LONG = 0, 1, 2, 3


def identity(cred):
    """``user:base64(SHA1(cred))``, user the bytes before the first ``:``."""
    user = cred.split(b':', 1)[0]
    return user + b':' + base64.b64encode(hashlib.sha1(cred).digest())


def body(xid, scheme, auth, auth_type=0):
    """An AUTH request body (no length prefix)."""
    return struct.pack('>iii', xid, AUTH, auth_type) + A.ustr(scheme) + \
        A.ustr(auth)


def parse(b):
    """AUTH body ``b`` -> (status, xid, type, n, off): zk_auth.h
    auth_frame (off relative to the body; -1 none)."""
    L = len(b)
    if L < 8:
        return AF_MALFORMED, 0, 0, 0, -1
    xid, op = struct.unpack_from('>ii', b, 0)
    if op != AUTH or L < 20:
        return AF_MALFORMED, xid, 0, 0, -1
    typ, sl = struct.unpack_from('>ii', b, 8)
    sl = max(sl, 0)
    k = 16
    if sl > L - k:
        return AF_MALFORMED, xid, typ, 0, -1
    scheme = bytes(b[k:k + sl])
    k += sl
    if k + 4 > L:
        return AF_MALFORMED, xid, typ, 0, -1
    al = max(struct.unpack_from('>i', b, k)[0], 0)
    k += 4
    if al != L - k:
        return AF_MALFORMED, xid, typ, 0, -1
    st = AF_SCHEME if scheme != b'digest' else \
        AF_LONG if al > AUTH_MAX else AF_OK
    return st, xid, typ, min(al, AUTH_MAX + 1), k


def permits_auth(vec, perm, addr, ids):
    """:func:`aclperm_model.permits` where a ``digest`` entry that carries
    the bit grants when its id is one of ``ids`` (bytes)."""
    ids = list(ids)[:AUTH_K]
    L = len(vec)
    if L < 4:
        return False
    n = struct.unpack_from('>i', vec, 0)[0]
    k = 4
    for _ in range(max(n, 0)):
        if k + 8 > L:
            return False
        perms, sl = struct.unpack_from('>ii', vec, k)
        k += 8
        sl = max(sl, 0)
        if sl > L - k:
            return False
        scheme = bytes(vec[k:k + sl])
        k += sl
        if k + 4 > L:
            return False
        il = max(struct.unpack_from('>i', vec, k)[0], 0)
        k += 4
        if il > L - k:
            return False
        ident = bytes(vec[k:k + il])
        k += il
        if perms & perm == 0:
            continue
        if scheme == b'world':
            if ident == b'anyone':
                return True
        elif scheme == b'ip':
            if A.ip_match(ident, addr):
                return True
        elif scheme == b'digest':
            # (an identity is never shorter than ':' and 28 digest bytes)
            if any(ident == i for i in ids if len(i) >= 29):
                return True
    return False


class Table(object):
    """The identities of S connections as serve_sessions_mixed keeps them,
    batch by batch: :meth:`batch` takes the AUTH bodies of one batch in frame
    order and returns their codes (1 OK, 2 AUTH_FAILED).  An identity known
    from an earlier batch takes no slot; within a batch every new identity
    takes one, equal ones too (so a test that wants one answer sends each
    identity once a row and batch)."""

    def __init__(self, S):
        self.rows = [[] for _ in range(S)]
        self.claimed = [0] * S

    def clear(self, rows):
        for r in rows:
            self.rows[r] = []
            self.claimed[r] = 0

    def batch(self, frames):
        """frames: [(row, body)] -> [code]"""
        before = [list(r) for r in self.rows]
        have = [min(c, AUTH_K) for c in self.claimed]
        out = []
        for row, b in frames:
            st, _, _, n, off = parse(b)
            if st != AF_OK:
                out.append(2)
                continue
            ident = identity(bytes(b[off:off + n]))
            if ident in before[row]:
                out.append(1)
            elif have[row] >= AUTH_K or self.claimed[row] >= AUTH_K:
                if have[row] < AUTH_K:
                    self.claimed[row] += 1
                out.append(2)
            else:
                self.claimed[row] += 1
                self.rows[row].append(ident)
                out.append(1)
        return out
