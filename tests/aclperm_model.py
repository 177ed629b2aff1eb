"""The Python mirror of csrc/kernels/zk_aclperm.h: which permission an op
needs and where, ZooKeeper's ``ip`` provider match and the walk over an ACL
vector in wire format.  tests/test_aclperm_host.py holds the header's host
build against it, tests/test_gpu_aclperm.py the kernels."""

import struct

READ, WRITE, CREATE, DELETE, ADMIN = 1, 2, 4, 8, 16
ALL = 31
T_NONE, T_NODE, T_PARENT, T_PARENT_OF_NODE = 0, 1, 2, 3
OPS = {'CREATE': 1, 'DELETE': 2, 'EXISTS': 3, 'GET_DATA': 4, 'SET_DATA': 5,
       'GET_ACL': 6, 'SET_ACL': 7, 'GET_CHILDREN': 8, 'SYNC': 9, 'PING': 11,
       'GET_CHILDREN2': 12, 'CHECK': 13, 'MULTI': 14, 'AUTH': 100,
       'SET_WATCHES': 101, 'SASL': 102, 'CREATE_SESSION': -10,
       'CLOSE_SESSION': -11}
NO_AUTH = -102


def need(op):
    """(perm bit, target) of opcode ``op``."""
    if op in (OPS['GET_DATA'], OPS['GET_CHILDREN'], OPS['GET_CHILDREN2']):
        return READ, T_NODE
    if op == OPS['SET_DATA']:
        return WRITE, T_NODE
    if op == OPS['CREATE']:
        return CREATE, T_PARENT
    if op == OPS['DELETE']:
        return DELETE, T_PARENT_OF_NODE
    return 0, T_NONE


def _digits(b, k, most):
    n, v = 0, 0
    while k < len(b) and n <= most and 0x30 <= b[k] <= 0x39:
        v = v * 10 + b[k] - 0x30
        n += 1
        k += 1
    return n, v, k


def ip_match(ident, addr):
    """Does the ``ip`` id ``ident`` (bytes) cover ``addr`` (a host-order
    32-bit word, 0: none)?"""
    addr &= 0xFFFFFFFF
    if addr == 0 or len(ident) == 0:
        return False
    k, ip = 0, 0
    for part in range(4):
        n, v, k = _digits(ident, k, 3)
        if n < 1 or n > 3 or v > 255:
            return False
        ip = (ip << 8) | v
        if part < 3:
            if k >= len(ident) or ident[k] != 0x2E:
                return False
            k += 1
    bits = 32
    if k < len(ident):
        if ident[k] != 0x2F:
            return False
        n, bits, k = _digits(ident, k + 1, 2)
        if n < 1 or n > 2 or bits > 32 or k != len(ident):
            return False
    mask = 0 if bits == 0 else (0xFFFFFFFF << (32 - bits)) & 0xFFFFFFFF
    return ((ip ^ addr) & mask) == 0


def permits(vec, perm, addr):
    """Does the wire-format ACL vector ``vec`` grant ``perm`` to ``addr``?"""
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
            if ip_match(ident, addr):
                return True
    return False


def parent_cut(path):
    cut = len(path) - 1
    while cut > 0 and path[cut] != 0x2F:
        cut -= 1
    return max(cut, 0)


def ustr(b):
    return struct.pack('>i', len(b)) + b


def vector(entries):
    """``[(perms, scheme, id), ...]`` (bytes or str) -> the wire vector."""
    out = struct.pack('>i', len(entries))
    for perms, scheme, ident in entries:
        if isinstance(scheme, str):
            scheme = scheme.encode()
        if isinstance(ident, str):
            ident = ident.encode()
        out += struct.pack('>i', perms) + ustr(scheme) + ustr(ident)
    return out


def addr_of(dotted):
    """'10.1.2.9' -> the host-order word."""
    a, b, c, d = (int(x) for x in dotted.split('.'))
    return (a << 24) | (b << 16) | (c << 8) | d


def as_i32(word):
    """A 32-bit word as the int32 value an ``addrs`` tensor holds."""
    word &= 0xFFFFFFFF
    return word - (1 << 32) if word >= 1 << 31 else word
