"""The payload-size ladder of the size tests (tests/test_gpu_payload_sizes.py,
tests/test_encode_sizes.py) and the host mirrors of the encoders' size rules
(csrc/kernels/encode.hip): which records of a 256-record block K10 / K13
stage through the LDS image and which one thread writes straight to global
memory, and which GET_DATA replies K13 emits from registers, through the
image, or as a hole the waves copy."""

import random

from treemodel import create, exists, get

# csrc/kernels/encode.hip (a changed constant there must change here: the
# coverage assertions of the tests are made through these)
ENC_T = 256                 # :18   records per block
GET_REG_DATA = 128          # :277  GET_DATA replies emitted from registers
STAGE_BYTES = 28 * 1024     # :372  LDS image per block
BIG_HOLE = 256              # :495  smallest aligned interior made a hole
REQ_REG_PATH = 64           # :793  read-request paths emitted from registers
HOLE_TRIP = 16 * 16 * 4     # :555-558 copy_hole_q: a quarter's bytes a trip
STAT_BYTES = 68

PATH_LENS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000)
BIG = 1000000


def ladder(big=False):
    """The data lengths ``D``: every length around each size the data path
    branches on, without (default) or with the one of 1 000 000 bytes."""
    d = list(range(0, 41)) + list(range(120, 141)) + list(range(250, 321)) + \
        list(range(1000, 1073))
    for k in range(11, 17):
        d += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    d += list(range(STAGE_BYTES - 40, STAGE_BYTES + 41, 8))
    d.append(100000)
    if big:
        d.append(BIG)
    return d


def rand_bytes(rng, n):
    """``n`` random bytes (no fill pattern: a shifted copy shows)."""
    return rng.getrandbits(8 * n).to_bytes(n, 'little') if n else b''


def rand_path(rng, n, prefix='/'):
    """A path of exactly ``n`` bytes starting with ``prefix``."""
    abc = 'abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ'
    assert n >= len(prefix)
    return prefix + ''.join(rng.choice(abc) for _ in range(n - len(prefix)))


# ---- staged_emit (K10) ------------------------------------------------------

def staged_runs(offs, sizes):
    """staged_emit's walk over the records at ``offs`` / ``sizes`` (the whole
    batch, blocks of ENC_T): (runs, direct), ``runs`` the [rs, re) staged
    through the image with the bytes the last record's end leaves free in it
    (0: it fills the image exactly), ``direct`` the records one thread
    writes straight to global memory (the ``k == 0`` branch)."""
    runs, direct = [], []
    n = len(offs)
    for r0 in range(0, n, ENC_T):
        r1 = min(r0 + ENC_T, n)
        rs = r0
        while rs < r1:
            a0 = offs[rs] & ~15
            k = sum(1 for i in range(rs, r1)
                    if offs[i] + sizes[i] - a0 + 16 <= STAGE_BYTES)
            if k == 0:
                direct.append(rs)
                rs += 1
                continue
            re = rs + k
            runs.append((rs, re, STAGE_BYTES -
                         (offs[re - 1] + sizes[re - 1] - a0 + 16)))
            rs = re
    return runs, direct


# ---- resp_write (K13) -------------------------------------------------------

def hole_h0(off):
    return (off + 20 + 15) & ~15


def hole_interior(off, dl):
    """Bytes of the 16-byte aligned interior of the [len | data] bytes of a
    successful GET_DATA reply of ``dl`` data bytes whose frame starts at
    stream offset ``off`` (resp_write's h1 - h0)."""
    return ((off + 20 + 4 + dl) & ~15) - hole_h0(off)


def hole_of(off, dl):
    """That reply's hole bytes: its interior when at least BIG_HOLE."""
    h = hole_interior(off, dl)
    return h if h >= BIG_HOLE else 0


def reply_size(dl):
    """Frame bytes of a successful GET_DATA reply of ``dl`` data bytes."""
    return 4 + 16 + 4 + dl + STAT_BYTES


class ReplyCoverage(object):
    """What the GET_DATA replies of the streams fed to it reached: per start
    residue mod 16 the data lengths and the interiors (interiors come in
    steps of 16), so that :meth:`check` can ask for the two values next to
    each bound; the hole counts of the blocks."""

    def __init__(self):
        self.dl = [set() for _ in range(16)]
        self.interior = [set() for _ in range(16)]
        self.block_holes = []

    def add(self, offs, dls):
        """One reply stream: frame starts ``offs`` and, per reply, the data
        length of a successful GET_DATA or None for any other reply."""
        for r0 in range(0, len(offs), ENC_T):
            nh = 0
            for o, dl in zip(offs[r0:r0 + ENC_T], dls[r0:r0 + ENC_T]):
                if dl is None:
                    continue
                self.dl[o & 15].add(dl)
                if dl > GET_REG_DATA:
                    self.interior[o & 15].add(hole_interior(o, dl))
                nh += hole_of(o, dl) > 0
            self.block_holes.append(nh)

    def check(self):
        """At every residue: the register path's last length and the first
        past it; the largest interior that is no hole and the smallest that
        is one; a hole of exactly one trip of copy_hole_q and one of 16
        bytes more.  Some block with a number of holes that is no multiple
        of 4, some block with more than 4."""
        for res in range(16):
            assert {GET_REG_DATA, GET_REG_DATA + 1} <= self.dl[res], \
                ('register path', res)
            assert {BIG_HOLE - 16, BIG_HOLE} <= self.interior[res], \
                ('hole rule', res)
            assert {HOLE_TRIP, HOLE_TRIP + 16} <= self.interior[res], \
                ('1 KiB trip', res)
        assert any(n % 4 for n in self.block_holes), self.block_holes
        assert any(n > 4 for n in self.block_holes), self.block_holes


# ---- the ladder as znodes ---------------------------------------------------

LADDER_DIR = '/bench/L'


def ladder_path(dl):
    return '%s/s%07d' % (LADDER_DIR, dl)


def ladder_tree(gpu, scratch=0, out_cap=20 << 20, cap_frames=1024, **kw):
    """A tree with room for the ladder (a slab of about 4.3 MB) and its
    server and model."""
    from treemodel import TreeModel
    from zkmi.server.engine import GpuServer
    from zkmi.server.tree import GpuTree
    tree = GpuTree(10, 4096, fanout=10, device=gpu, spare=0.0,
                   scratch=scratch, **kw)
    srv = GpuServer(tree, cap_frames, out_cap)
    return TreeModel(tree, srv, gpu)


def create_ladder(m, sizes, seed=7):
    """CREATE one znode of random data per size of ``sizes`` under
    LADDER_DIR, each batch a large one between small neighbours (so it is
    not alone in its 256-request block); one audit at the end.  Returns
    {size: path}."""
    rng = random.Random(seed)
    m.serve([create(LADDER_DIR)], audit=False)
    paths = {}
    small = [dl for dl in sizes if dl < 2000]
    large = [dl for dl in sizes if dl >= 2000]
    # the small ones lead, follow and sit between the large ones
    k = max(len(small) // (len(large) + 1), 1) if large else len(small)
    order = []
    while small or large:
        order += small[:k]
        small = small[k:]
        if large:
            order.append(large.pop(0))
    batch, nbytes = [], 0
    for dl in order + [None]:
        if dl is None or (batch and nbytes + dl > (3 << 20)):
            m.serve(batch, audit=False)
            batch, nbytes = [], 0
        if dl is not None:
            paths[dl] = ladder_path(dl)
            batch.append(create(paths[dl], rand_bytes(rng, dl)))
            nbytes += dl
    m.audit()
    return paths


def read_batch(paths, lead=None):
    """GET_DATA and EXISTS of every ladder node, ``lead`` first."""
    pk = [lead] if lead is not None else []
    for dl in sorted(paths):
        pk.append(get(paths[dl]))
        if dl % 3 == 0:
            pk.append(exists(paths[dl]))
    return pk
