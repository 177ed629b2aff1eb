"""A Python mirror of the ordered front end's rules: the cut's ordered rule
(csrc/kernels/zk_front.h front_walk_ordered) and the deferral of the ordered
session serve (csrc/kernels/zk_order_clip.h clip_overflow, clip_deferred,
clip_range).  The host test compares it with the headers built by g++, the
GPU tests with the kernels.  Frames are built with tests/frontmodel.py."""

import struct

import frontmodel as F

OPS = F.OPS
MAX_PACKET = F.MAX_PACKET
TREE_WRITES = (OPS['CREATE'], OPS['DELETE'], OPS['SET_DATA'])
RANK_MASK = 0x7f
CHUNK = 4096                      # the cut kernel's staged window


def is_late(op, has_acl):
    return op in (OPS['GET_CHILDREN'], OPS['GET_CHILDREN2'],
                  OPS['SET_WATCHES']) or (op == OPS['GET_ACL'] and has_acl)


def walk_ordered(seg, quota, has_acl=True, max_packet=MAX_PACKET):
    """(take, nfr, flag, nwr) of one segment's bytes."""
    n = len(seg)
    p = nfr = flag = nwr = phase = 0
    quota = min(quota, 0x7fffffff)
    while nfr < quota and n - p >= 4:
        L = struct.unpack_from('>i', seg, p)[0]
        if L < 0 or L > max_packet:
            flag = 1
            break
        if L > n - p - 4:
            break
        op = struct.unpack_from('>i', seg, p + 8)[0] if L >= 8 else 0
        if phase == 1 and op in TREE_WRITES:
            break
        if is_late(op, has_acl):
            phase = 1
        p += 4 + L
        nfr += 1
        if F.is_write(op):
            nwr += 1
        if op == OPS['CLOSE_SESSION']:
            break
    return p, nfr, flag, nwr


def cut_ordered(raw, starts, quota, has_acl=True, max_packet=MAX_PACKET):
    """(fault, [(take, nfr, flag, nwr) per segment]) of a raw stream."""
    S = len(starts) - 1
    if F.table_fault(starts, len(raw)):
        return 1, [(0, 0, 0, 0)] * S
    return 0, [walk_ordered(raw[starts[s]:starts[s + 1]], quota, has_acl,
                            max_packet) for s in range(S)]


def clip(rank, cls, sub, f_seg, S, passes, nfr=None):
    """(clipf[S], deferred[nfr]) of a whole batch's tables; ``rank`` is
    indexed by ``sub`` for the frames of class 0."""
    ncap = len(cls)
    if nfr is None:
        nfr = ncap
    clipf = [ncap] * S
    for i in range(nfr):
        sg = f_seg[i]
        if not 0 <= sg < S or cls[i] != 0 or not 0 <= sub[i] < ncap:
            continue
        if (rank[sub[i]] & RANK_MASK) >= passes and i < clipf[sg]:
            clipf[sg] = i
    deferred = [1 if 0 <= f_seg[i] < S and i >= clipf[f_seg[i]] else 0
                for i in range(nfr)]
    return clipf, deferred


def ranges(clipf, rep_off, rec_off, off, starts, nfr):
    """[(rep_end, used)] per segment."""
    out = []
    for s in range(len(clipf)):
        r0, r1 = rep_off[s], rep_off[s + 1]
        b0, b1 = starts[s], starts[s + 1]
        end, used = r1, max(b1 - b0, 0)
        c = clipf[s]
        if 0 <= c < nfr:
            end = max(min(rec_off[c], r1), r0)
            used = max(min(off[c] - 4 - b0, used), 0)
        out.append((end, used))
    return out


# ---- the walk cases, shared by the host and the GPU test ----------------------

def walk_cases():
    """[(name, segment bytes, quota, has_acl, want or None)]: want is the
    expected (take, nfr, flag, nwr) where the case states it outright."""
    g = F.frame(OPS['GET_DATA'], b'\x00' * 9)                 # 21 bytes
    w = F.frame(OPS['SET_DATA'], b'\x00' * 13)                # 25 bytes
    cr = F.frame(OPS['CREATE'], b'\x00' * 13)
    de = F.frame(OPS['DELETE'], b'\x00' * 13)
    ls = F.frame(OPS['GET_CHILDREN'], b'\x00' * 9)
    l2 = F.frame(OPS['GET_CHILDREN2'], b'\x00' * 9)
    ac = F.frame(OPS['GET_ACL'], b'\x00' * 8)
    sw = F.frame(OPS['SET_WATCHES'], b'\x00' * 20)
    cl = F.frame(OPS['CLOSE_SESSION'])
    lg, lw = len(g), len(w)
    cases = [
        ('empty', b'', 8, True, (0, 0, 0, 0)),
        ('3 bytes', g[:3], 8, True, (0, 0, 0, 0)),
        ('length alone', g[:4], 8, True, (0, 0, 0, 0)),
        ('body one short', w[:-1], 8, True, (0, 0, 0, 0)),
        ('writes run on', w + cr + g + de + w, 8, True,
         (4 * lw + lg, 5, 0, 4)),
        ('write after a list', w + ls + g + w + g, 8, True,
         (lw + len(ls) + lg, 3, 0, 1)),
        ('write after a list2', l2 + cr, 8, True, (len(l2), 1, 0, 0)),
        ('delete after a list', g + ls + de, 8, True, (lg + len(ls), 2, 0, 0)),
        ('reads after a list', ls + g + ls + g, 8, True,
         (2 * len(ls) + 2 * lg, 4, 0, 0)),
        ('write after GET_ACL, ACL table', w + ac + w, 8, True,
         (lw + len(ac), 2, 0, 1)),
        ('write after GET_ACL, no ACL table', w + ac + w, 8, False,
         (2 * lw + len(ac), 3, 0, 2)),
        ('SET_WATCHES then a set', sw + w, 8, True, (len(sw), 1, 0, 0)),
        ('a set then SET_WATCHES', w + sw + g, 8, True,
         (lw + len(sw) + lg, 3, 0, 1)),
        ('CLOSE_SESSION mid-run', w + g + cl + g + w, 8, True,
         (lw + lg + len(cl), 3, 0, 2)),
        ('CLOSE_SESSION first', cl + g, 8, True, (len(cl), 1, 0, 1)),
        ('CLOSE_SESSION in phase 1', ls + cl + g, 8, True,
         (len(ls) + len(cl), 2, 0, 1)),
        ('quota 0', w + w, 0, True, (0, 0, 0, 0)),
        ('quota 1', w + w + w, 1, True, (lw, 1, 0, 1)),
        ('quota 1, a list', ls + w, 1, True, (len(ls), 1, 0, 0)),
        ('quota 2', w + w + w, 2, True, (2 * lw, 2, 0, 2)),
        ('bad length first', F.raw_frame(-1) + w, 8, True, (0, 0, 1, 0)),
        ('bad length in phase 0', w + w + F.raw_frame(MAX_PACKET + 1) + w, 8,
         True, (2 * lw, 2, 1, 2)),
        ('bad length in phase 1', w + ls + F.raw_frame(F.INT32_MIN) + g, 8,
         True, (lw + len(ls), 2, 1, 1)),
        ('bad length behind the stop', ls + w + F.raw_frame(-1), 8, True,
         (len(ls), 1, 0, 0)),
        ('bad length behind a close', cl + F.raw_frame(-1), 8, True,
         (len(cl), 1, 0, 1)),
        ('length 0 and 7 bytes', F.raw_frame(0) + F.raw_frame(7, b'\x00' * 7)
         + w, 8, True, (15 + lw, 3, 0, 1)),
    ]
    # a length word and an opcode word that straddle the staged window: the
    # frame in question is a write behind a list (the stop depends on its
    # opcode) or a list before a write (the phase does)
    for k in (1, 2, 3):
        pad = F.frame(OPS['GET_DATA'], b'\x00' * (CHUNK - k - 12))
        assert len(pad) == CHUNK - k            # the next length word straddles
        cases.append(('length straddles by %d' % k, pad + w + ls + w, 8, True,
                      (len(pad) + lw + len(ls), 3, 0, 1)))
        pad = F.frame(OPS['GET_DATA'], b'\x00' * (CHUNK - k - 8 - 12))
        assert len(pad) + 8 == CHUNK - k        # the next opcode word does
        pad2 = F.frame(OPS['GET_DATA'],
                       b'\x00' * (CHUNK - k - 8 - 12 - len(ls)))
        cases.append(('write opcode straddles by %d' % k, ls + pad2 + w + g,
                      8, True, (len(ls) + len(pad2), 2, 0, 0)))
        cases.append(('list opcode straddles by %d' % k, pad + ls + w, 8, True,
                      (len(pad) + len(ls), 2, 0, 0)))
    # a body longer than the window is skipped, not staged
    big = F.frame(OPS['SET_DATA'], b'\x07' * (3 * CHUNK + 5))
    cases.append(('long body', big + w + ls + w, 8, True,
                  (len(big) + lw + len(ls), 3, 0, 2)))
    return cases
