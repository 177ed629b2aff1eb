"""A Python mirror of the front end's staging rules
(csrc/kernels/zk_front.h): front_is_write, front_walk, the table fault,
front_piece_at, the owner table and front_piece.  The host test compares it
with the header built by g++, the GPU tests with the kernels."""

import struct

MAX_PACKET = 16 * 1024 * 1024
INT32_MIN = -2 ** 31
OPS = {'CREATE': 1, 'DELETE': 2, 'EXISTS': 3, 'GET_DATA': 4, 'SET_DATA': 5,
       'GET_ACL': 6, 'SET_ACL': 7, 'GET_CHILDREN': 8, 'SYNC': 9, 'PING': 11,
       'GET_CHILDREN2': 12, 'CHECK': 13, 'MULTI': 14, 'SET_WATCHES': 101,
       'CLOSE_SESSION': -11}
WRITES = (OPS['CREATE'], OPS['DELETE'], OPS['SET_DATA'],
          OPS['CLOSE_SESSION'])


def is_write(op):
    return op in WRITES


def frame(op, body=b'', xid=1):
    """A request frame: length word, xid, opcode, ``body``."""
    b = struct.pack('>ii', xid, op) + body
    return struct.pack('>i', len(b)) + b


def raw_frame(length, body=b''):
    """A length word of any value and whatever follows it."""
    return struct.pack('>i', length) + body


def walk(seg, quota, max_packet=MAX_PACKET):
    """(take, nfr, flag) of one segment's bytes."""
    n = len(seg)
    p = nfr = flag = 0
    quota = min(quota, 0x7fffffff)
    while nfr < quota and n - p >= 4:
        L = struct.unpack_from('>i', seg, p)[0]
        if L < 0 or L > max_packet:
            flag = 1
            break
        if L > n - p - 4:
            break
        wr = L >= 8 and is_write(struct.unpack_from('>i', seg, p + 8)[0])
        if wr and nfr > 0:
            break
        p += 4 + L
        nfr += 1
        if wr:
            break
    return p, nfr, flag


def table_fault(starts, n):
    S = len(starts) - 1
    for s in range(S + 1):
        v = starts[s]
        if (s == 0 and v != 0) or v < 0 or v > n:
            return 1
        if s < S and v > starts[s + 1]:
            return 1
    return 0


def cut(raw, starts, quota, max_packet=MAX_PACKET):
    """(fault, [(take, nfr, flag) per segment]) of a raw stream."""
    S = len(starts) - 1
    if table_fault(starts, len(raw)):
        return 1, [(0, 0, 0)] * S
    return 0, [walk(raw[starts[s]:starts[s + 1]], quota, max_packet)
               for s in range(S)]


def piece_at(off, d):
    """off: the P piece offsets (without the total)."""
    lo = 0
    for i, o in enumerate(off):
        if o <= d:
            lo = i + 1
        else:
            break
    return max(lo - 1, 0)


def owners(wslots):
    """(owner[64], dup_slot)."""
    own = [-1] * 64
    named = [0] * 64
    for s, w in enumerate(wslots):
        if 0 <= w < 64:
            if own[w] < 0:
                own[w] = s
            named[w] += 1
    return own, sum(max(0, c - 1) for c in named)


def _slice(k, a, b, cap):
    if a < 0 or b < a or b > cap:
        return (k, 0, 0)
    return (k, a, b - a)


def pieces(wslots, rep_off=None, slot_offs=(None, None, None), err=None,
           caps=(0, 0, 0, 0)):
    """(dup_slot, [(stream, src, len)] * 4 S), in sending order."""
    own, dup = owners(wslots)
    out = []
    for s, w in enumerate(wslots):
        for k in range(4):
            if err is not None and err != 0:
                out.append((k, 0, 0))
            elif k == 0:
                out.append((0, 0, 0) if rep_off is None else
                           _slice(0, rep_off[s], rep_off[s + 1], caps[0]))
            else:
                so = slot_offs[k - 1]
                if so is None or not 0 <= w < 64 or own[w] != s:
                    out.append((k, 0, 0))
                else:
                    out.append(_slice(k, so[w], so[w + 1], caps[k]))
    return dup, out


# ---- the walk cases, shared by the host and the GPU test ----------------------

def walk_cases():
    """[(name, segment bytes, quota, want or None)]: want is the expected
    (take, nfr, flag) where the case states it outright."""
    G = lambda: frame(OPS['GET_DATA'], b'\x00' * 9)          # 21 bytes
    W = lambda op='SET_DATA': frame(OPS[op], b'\x00' * 13)   # 25 bytes
    g, w = G(), W()
    cases = [
        ('empty', b'', 8, (0, 0, 0)),
        ('1 byte', g[:1], 8, (0, 0, 0)),
        ('2 bytes', g[:2], 8, (0, 0, 0)),
        ('3 bytes', g[:3], 8, (0, 0, 0)),
        ('length alone', g[:4], 8, (0, 0, 0)),
        ('body one short', g[:-1], 8, (0, 0, 0)),
        ('good then one short', g + g[:-1], 8, (len(g), 1, 0)),
        ('length 0', raw_frame(0) + g, 8, (4 + len(g), 2, 0)),
        ('7 bytes', raw_frame(7, b'\x00\x00\x00\x01\xff\xff\xff') + g, 8,
         (11 + len(g), 2, 0)),
        # the opcode bytes of a 7-byte frame spell a write's first three
        ('7 bytes then write', raw_frame(7, b'\x00' * 7) + w, 8,
         (11, 1, 0)),
    ]
    for name, L in (('-1', -1), ('INT32_MIN', INT32_MIN),
                    ('MAX_PACKET + 1', MAX_PACKET + 1)):
        cases.append(('bad %s first' % name, raw_frame(L) + g, 8, (0, 0, 1)))
        cases.append(('bad %s after two' % name, g + g + raw_frame(L) + g, 8,
                      (2 * len(g), 2, 1)))
    # MAX_PACKET itself is a good length whose body is not there yet
    cases.append(('MAX_PACKET first', raw_frame(MAX_PACKET) + g, 8,
                  (0, 0, 0)))
    cases.append(('MAX_PACKET after two', g + g + raw_frame(MAX_PACKET) + g,
                  8, (2 * len(g), 2, 0)))
    cases += [
        ('quota 0', g + g + g, 0, (0, 0, 0)),
        ('quota 1', g + g + g, 1, (len(g), 1, 0)),
        ('quota = frames', g + g + g, 3, (3 * len(g), 3, 0)),
        ('quota before bad', g + raw_frame(-1), 1, (len(g), 1, 0)),
        ('read read write read', g + g + w + g, 8, (2 * len(g), 2, 0)),
        ('write write', w + w, 8, (len(w), 1, 0)),
        ('write read', w + g, 8, (len(w), 1, 0)),
        ('read only', g + g + g + g, 8, (4 * len(g), 4, 0)),
        ('close after reads', g + g + W('CLOSE_SESSION'), 8,
         (2 * len(g), 2, 0)),
        ('close first', frame(OPS['CLOSE_SESSION']) + g, 8, (12, 1, 0)),
        ('create first', W('CREATE') + g, 8, (len(w), 1, 0)),
        ('delete first', W('DELETE') + W('DELETE'), 8, (len(w), 1, 0)),
    ]
    for op in (OPS['PING'], OPS['SYNC'], OPS['SET_WATCHES'], 7, 13, 14):
        f = frame(op, b'\x00' * 5)
        cases.append(('no write %d' % op, f + f + g, 8,
                      (2 * len(f) + len(g), 3, 0)))
    return cases
