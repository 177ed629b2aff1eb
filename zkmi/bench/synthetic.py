"""GPU-resident synthetic ZooKeeper workload: a 1M-znode tree in HBM and the
full wire pipeline around it.

One :meth:`GetPipeline.step` performs, entirely on the GPU and on the real
ZooKeeper wire format:

  client  K10 encode B GET_DATA requests (paths gathered straight from the
          tree's path arena, xids recorded in the HBM xid->opcode table)
  server  K1 frame-scan the request stream, K12 decode the requests, hash
          lookup in the tree, K13 encode GET_DATA replies (header + data +
          Stat) into the reply stream
  client  K1 frame-scan the reply stream, K2/K3/K4 decode header, opcode
          (via the xid table), data (offset/length) and Stat

plus a device-side check that every reply is OK and carries the node the
request asked for.  Nothing is skipped inside a step, and a step makes no
device-to-host read: K1 reads each stream's length from the device-side
byte count its encoder produced (``total``), so any frame-size mix scans
sync-free and no byte past a stream's end is walked.

:class:`MixPipeline` does the same for the create/set/delete mix with
version CAS and ACL encode (BASELINE config 3).
"""

import time

import numpy as np
import torch

from .. import consts
from ..ops import _lib
from ..ops import batch as B

I64, I32, U8 = torch.int64, torch.int32, torch.uint8

# the largest batch tree_seq_order numbers
_SEQ_MAX = 1 << 24
# K1 tiles a wave on the GPU server's request streams.  Request streams of
# equal-sized frames without length-like words take groups (the groups' walk
# steps over a run of equal frames): GET 4 tiles a wave, the storm's
# identical creates 8.  The others stay at one: SET_DATA versions read as
# frame lengths make phantom chains, which the per-tile maps settle and a
# group's walked tiles do not (README, "Measured and rejected").
_SRV_GROUP = 1
_GET_SRV_GROUP = 4
_STORM_SRV_GROUP = 8


def _len(total):
    """A stream length for K1: the encoder's device total (no host read)."""
    return total



def _next_pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


NODE_FREE = -2           # node_parent of an unused node (zk_tree.h)


def path_owner(paths, world):
    """Owner rank of every path: FNV-1a 32 of the bytes mod ``world`` —
    the host mirror of csrc/kernels/route.hip's router."""
    out = np.empty(len(paths), np.int64)
    by_len = {}
    for i, p in enumerate(paths):
        by_len.setdefault(len(p), []).append(i)
    for ln, ids in by_len.items():
        m = np.frombuffer(b''.join(paths[i] for i in ids),
                          np.uint8).reshape(len(ids), ln) if ln else \
            np.zeros((len(ids), 0), np.uint8)
        h = np.full(len(ids), 2166136261, np.uint64)
        for k in range(ln):
            h = ((h ^ m[:, k]) * np.uint64(16777619)) & np.uint64(0xffffffff)
        out[ids] = (h % np.uint64(world)).astype(np.int64)
    return out


def _i64(u):
    """A 64-bit unsigned seed as the signed int a torch op schema takes."""
    u &= (1 << 64) - 1
    return u - (1 << 64) if u >= (1 << 63) else u


def slot_bytes(data_cap):
    """Bytes of one wire-format node slot (zk_batch.h ZkNodeStore)."""
    return _lib.SLOT_DATA + ((data_cap + 15) & ~15) + 4


class GpuTree(object):
    """``n_nodes`` znodes ``/bench/dDDDDD/nNNNNNNNN`` (``fanout`` children per
    directory) with ``data_bytes`` of random data each.  Node ``v`` has
    ``czxid == v + 1``."""

    def __init__(self, n_nodes=1_000_000, data_bytes=100, fanout=1000,
                 device=None, spare=0.25, seed=0, shard=None, ctime_ms=None,
                 data_dist=None, name_pad=None, scratch=0, watch_cap=0,
                 hash_factor=2, compact_free=False, acl_cap=0,
                 acl_arena_bytes=None):
        dev = torch.device(device) if device is not None else \
            torch.device('cuda', torch.cuda.current_device())
        self.device = dev
        L = _lib.lib()
        ndirs = (n_nodes + fanout - 1) // fanout
        # node order: 0 = /bench, 1..ndirs = dirs, then leaves
        paths = ['/bench'] + ['/bench/d%06d' % d for d in range(ndirs)]
        leaf0 = len(paths)
        # name_pad = (lo, hi): leaf names padded with a uniform lo..hi
        # characters (variable path lengths)
        rng = np.random.default_rng(seed + 17)
        if name_pad is not None:
            pad = rng.integers(name_pad[0], name_pad[1] + 1, n_nodes)
            paths += ['/bench/d%06d/n%09d%s' % (i // fanout, i, 'p' * pad[i])
                      for i in range(n_nodes)]
        else:
            paths += ['/bench/d%06d/n%09d' % (i // fanout, i)
                      for i in range(n_nodes)]
        nst = len(paths)
        parents = np.empty(nst, np.int64)
        parents[0] = -1
        parents[1:leaf0] = 0
        parents[leaf0:] = 1 + np.arange(n_nodes) // fanout
        self.n_static = nst
        self.leaf0 = leaf0
        self.n_leaves = n_nodes
        # data_dist = (lo, hi): leaf data lengths uniform in lo..hi bytes
        # (variable payloads); data_bytes is then the largest
        if data_dist is not None:
            leaf_dl = rng.integers(data_dist[0], data_dist[1] + 1,
                                   n_nodes).astype(np.int32)
            data_bytes = int(data_dist[1])
        self.data_bytes = data_bytes
        self.data_dist = data_dist
        cap = int(nst * (1 + spare)) + 1024
        enc = [p.encode() for p in paths]
        plen = np.fromiter((len(e) for e in enc), np.int32, nst)
        poff = np.zeros(nst, np.int64)
        np.cumsum(plen[:-1], out=poff[1:])
        arena = b''.join(enc)
        # wire-format slots; data capacity >= 128 so sets can grow
        dcap = max(data_bytes, 128)
        sb = slot_bytes(dcap)
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        scratch = (int(scratch) + 15) & ~15
        # every spare node may need a fresh path (up to 64 bytes each, in
        # 16-byte multiples)
        self._alloc(dev, cap, len(arena) + (cap - nst) * 80 + (1 << 16),
                    cap * sb, dcap, scratch, hash_factor, watch_cap, acl_cap,
                    acl_arena_bytes, compact_free,
                    slab_fill=lambda nb: torch.randint(
                        0, 256, (nb,), dtype=U8, device=dev, generator=g),
                    slot_stride=sb)
        self.path_arena[:len(arena)] = torch.frombuffer(
            bytearray(arena), dtype=U8).to(dev)
        self.node_path_off[:nst] = torch.from_numpy(poff).to(dev)
        self.node_path_len[:nst] = torch.from_numpy(plen).to(dev)
        # bytes of each node's path storage (the static paths are packed)
        self.node_path_cap[:nst] = self.node_path_len[:nst]
        self.node_pw[:nst] = torch.from_numpy(
            (poff << 24) | plen.astype(np.int64)).to(dev)
        self.node_parent[:nst] = torch.from_numpy(parents).to(dev)
        if data_dist is not None:
            self.data_len[leaf0:nst] = torch.from_numpy(leaf_dl).to(dev)
        else:
            self.data_len[leaf0:nst] = data_bytes
        nkids = np.zeros(nst, np.int32)
        nkids[0] = ndirs
        nkids[1:leaf0] = np.bincount(np.arange(n_nodes) // fanout,
                                     minlength=ndirs)[:ndirs]
        nk = torch.from_numpy(nkids).to(dev)
        cnt = [0] * _lib.TC_N
        cnt[_lib.TC_NODES], cnt[_lib.TC_ZXID] = nst, nst
        cnt[_lib.TC_PATH_TOP], cnt[_lib.TC_SLAB_TOP] = len(arena), nst * sb
        self.counters.copy_(torch.tensor(cnt, dtype=I64, device=dev))
        now = int(time.time() * 1000) if ctime_ms is None else ctime_ms
        L.tree_fill(self._tensors, 0, nst, nk, now)
        # shard = (rank, world): this replica indexes only the leaves whose
        # path hashes to `rank` (zkmi/parallel/sharded.py routes every read
        # there); the rest stay in the layout, unreachable by lookup
        self.shard = shard
        if shard is not None and shard[1] > 1:
            own = path_owner(enc[leaf0:], shard[1])
            gone = np.nonzero(own != shard[0])[0] + leaf0
            self.node_parent[torch.from_numpy(gone).to(dev)] = NODE_FREE
        L.tree_build(self._tensors, 0, nst)
        torch.cuda.synchronize(dev)

    def _alloc(self, dev, cap, path_cap, slab_cap, dcap, scratch,
               hash_factor, watch_cap, acl_cap, acl_arena_bytes,
               compact_free=False, slab_fill=None, slot_stride=None):
        """The tensors of an empty tree of ``cap`` node slots, a path arena
        of ``path_cap`` bytes and a slab of ``slab_cap`` (+ ``scratch``)
        bytes, with the watch and ACL tables asked for: what the
        constructor and :meth:`load` share.  Counters, index and node table
        are all zero / free of content.  ``slab_fill(bytes)`` makes the slab
        (the constructor's random bytes; default zeros), ``slot_stride``
        lays the slots out back to back (default: offsets all zero, for the
        load to set)."""
        self.device = dev
        self.cap = cap
        self.path_cap = path_cap
        self.path_arena = torch.zeros(self.path_cap, dtype=U8, device=dev)
        self.node_path_off = torch.zeros(cap, dtype=I64, device=dev)
        self.node_path_len = torch.zeros(cap, dtype=I32, device=dev)
        self.node_path_cap = torch.zeros(cap, dtype=I32, device=dev)
        # path word (offset << 24 | length) the hash lookups verify against
        self.node_pw = torch.zeros(cap, dtype=I64, device=dev)
        self.node_parent = torch.full((cap,), -1, dtype=I64, device=dev)
        self.slot = slot_bytes(dcap)
        self.slab_cap = slab_cap
        # hash vals pack node (32 bits) and slot offset / 16 (31 bits)
        assert cap < (1 << 31) and self.slab_cap < (1 << 35), 'tree too big'
        # scratch: bytes past the tree's slab for the snapshots of ordered
        # serving (GpuServer.serve(ordered=True)); the tree's descriptor
        # sees slab[:slab_cap], the reply encoder the whole allocation
        self.slab_all = slab_fill(self.slab_cap + scratch) \
            if slab_fill is not None else \
            torch.zeros(self.slab_cap + scratch, dtype=U8, device=dev)
        self.slab = self.slab_all[:self.slab_cap]
        self.scratch = self.slab_all[self.slab_cap:] if scratch else None
        self.slot_off = torch.zeros(cap, dtype=I64, device=dev) \
            if slot_stride is None else \
            torch.arange(cap, dtype=I64, device=dev) * slot_stride
        self.data_len = torch.zeros(cap, dtype=I32, device=dev)
        self.slot_cap = torch.full((cap,), dcap, dtype=I32, device=dev)
        # hash entries per node slot (a power of two above it): 2 keeps a
        # read-mostly tree's table under half full; a write-heavy one
        # (SEQUENTIAL names never reused) fills with tombstones between
        # rebuilds, and a wider table rebuilds less often
        # (capped at 2^28 entries, 16 GB, unless 2 a slot needs more: the
        # storm's replicated tree at 8 ranks holds ~25M node slots)
        hcap = max(min(_next_pow2(hash_factor * cap), 1 << 28),
                   _next_pow2(2 * cap))
        # 64-byte entries, empty = all zero bytes (csrc/kernels/zk_tree.h)
        self.ht = torch.zeros(_lib.HT_WORDS * hcap, dtype=I64, device=dev)
        self.counters = torch.zeros(_lib.TC_N, dtype=I64, device=dev)
        self.free_list = torch.empty(cap, dtype=I64, device=dev)
        # host-endian cversion / numChildren / pzxid shadows + dirty list
        # cversion << 32 | numChildren per node (one atomic per child write)
        self.cn = torch.zeros(cap, dtype=I64, device=dev)
        # ephemeralOwner per node, host-endian (session expiry scans it)
        self.eph = torch.zeros(cap, dtype=I64, device=dev)
        self.pzxid = torch.zeros(cap, dtype=I64, device=dev)
        self.dirty = torch.zeros(cap, dtype=I32, device=dev)
        self.dirty_list = torch.empty(cap, dtype=I64, device=dev)
        self.hcap = hcap
        # write workloads: the free ring's pending entries re-sorted after
        # every served batch (free_compact)
        self.compact_free = compact_free
        self.free_ws = None
        self.snap_ws = None
        # the tree / node-store descriptor lists torch.ops.zkmi takes
        # (csrc/torch/zkmi_ops.cpp tree() / node_store() field order)
        self.store = [self.slab_all, self.slot_off, self.data_len,
                      self.slot_cap]
        self._tensors = [self.ht, self.node_path_off, self.node_path_len,
                         self.node_parent, self.path_arena, self.counters,
                         self.slab, self.slot_off, self.data_len,
                         self.slot_cap, self.free_list, self.cn,
                         self.pzxid, self.dirty, self.dirty_list,
                         self.node_pw, self.node_path_cap, self.eph]
        # watch table (watch_cap > 0): path-keyed one-shot watches of up to
        # 64 watcher slots (csrc/kernels/zk_tree.h wt_*); every serve of a
        # tree with one fires the watches its writes hit
        self.watch = None
        if watch_cap > 0:
            self.watch = self._watch_table(
                max(_next_pow2(2 * int(watch_cap)), 8))
            self._tensors = self._tensors + list(self.watch)
        # ACL table (acl_cap > 0: room for that many distinct ACLs beside the
        # open one): csrc/kernels/tree_acl.hip.  A server over a tree with
        # one records every CREATE's ACL and serves GET_ACL batches
        self.acl = None
        if acl_cap > 0:
            self._init_acl(int(acl_cap), acl_arena_bytes)

    @classmethod
    def load(cls, image, device=None, spare=0.25, data_cap=128,
             hash_factor=2, watch_cap=0, acl_cap=0, scratch=0,
             acl_arena_bytes=None, nodes=None, path_bytes=None,
             slab_bytes=None):
        """A tree holding the znodes of ``image`` (a device or CPU uint8
        tensor, or ``bytes``: what :meth:`snapshot` or
        ``zkmi.utils.treeimage.pack`` made), record ``i`` at node ``i``,
        with room for ``n * (1 + spare)`` nodes as the constructor has for
        its static ones, ``max(data_cap, data length)`` bytes of data a
        node, and whatever tables are asked for.  ``nodes`` /
        ``path_bytes`` / ``slab_bytes`` set a capacity outright.  The zxid
        counter continues from the image's; ephemerals keep their owner, so
        an :meth:`expire` of that session removes them; watches and
        sessions are not part of an image.  Raises
        ``treeimage.TreeImageError(code, index)`` for an image the device
        refuses.  One host read of the header, one of the outcome."""
        from ..utils import treeimage as TI
        dev = torch.device(device) if device is not None else \
            torch.device('cuda', torch.cuda.current_device())
        if isinstance(image, (bytes, bytearray, memoryview)):
            image = torch.frombuffer(bytearray(image) or bytearray(1),
                                     dtype=U8)[:len(image)]
        if image.dtype != U8 or image.dim() != 1:
            raise ValueError('load: the image is a 1-d uint8 tensor or bytes')
        length = image.numel()
        img = image.to(dev).contiguous()
        if length == 0:
            img = torch.zeros(16, dtype=U8, device=dev)
        # sizing only: the device checks every field it uses itself.  What
        # the header asks for is bounded by what the image can hold (a
        # record's data and path lie inside the body), so a header that
        # lies cannot size the tree past a few times the image: it ends as
        # NO_ROOM or BAD_HEADER on the device
        n, body, path16, max_data = 0, 0, 0, 0
        if length >= TI.HEAD:
            h = TI._HEAD.unpack(bytes(img[:TI.HEAD].cpu().numpy().tobytes()))
            room = length - TI.HEAD
            if 0 <= h[3] <= room // 8 - 1 and \
                    0 <= h[4] <= room - 8 * (h[3] + 1):
                n, body = h[3], h[4]
                path16 = min(max(h[7], 0), body + 16 * n)
                max_data = min(max(h[8], 0), body)
        dcap = int(data_cap)
        cap = int(nodes) if nodes is not None else \
            int(n * (1 + spare)) + 1024
        cap = max(cap, 1)
        # the records' slots: each as large as the largest, but no more in
        # all than the body's bytes over a slot of data_cap each (the data
        # lies inside the body, so this holds whatever the header says); the
        # spare ones what a CREATE allocates at least
        sb = slot_bytes(max(dcap, max_data))
        slab = min(n * sb, n * slot_bytes(dcap) + body + 16 * n) + \
            max(cap - n, 0) * slot_bytes(max(dcap, 128))
        if slab_bytes is not None:
            slab = max((int(slab_bytes) + 15) & ~15, 16)
        if cap >= (1 << 31) or slab >= (1 << 35):
            # (past what a hash val addresses: no tree holds this image)
            raise TI.TreeImageError(TI.NO_ROOM, -1)
        self = cls.__new__(cls)
        self._alloc(dev, cap,
                    max(int(path_bytes), 16) if path_bytes is not None else
                    path16 + max(cap - n, 0) * 80 + (1 << 16),
                    slab, dcap, (int(scratch) + 15) & ~15, hash_factor,
                    watch_cap, acl_cap, acl_arena_bytes)
        self.slot = sb
        self.n_static = n
        self.leaf0 = self.n_leaves = None
        self.data_bytes = max_data
        self.data_dist = None
        self.shard = None
        L = _lib.lib()
        ws = torch.empty(L.tree_load_workspace(n), dtype=U8, device=dev)
        status = torch.zeros(2, dtype=I64, device=dev)
        _lib.tree_load(self._tensors, self.acl, img, length, n, dcap, ws,
                       status)
        code, index = status.cpu().tolist()
        if code != TI.OK:
            raise TI.TreeImageError(code, index)
        return self

    def snapshot(self, out=None):
        """The image of the live znodes (csrc/kernels/zk_snap.h), written on
        the device between batches: a uint8 device tensor of exactly its
        size (one host read of the size).  With ``out`` (a uint8 device
        tensor, 16-byte aligned) nothing is read back: returns ``(out,
        total, status)``, ``total`` a device int64 [2] (image bytes,
        records) and ``status`` a device int64 [2] whose first word is 0, or
        ``treeimage.NO_ROOM`` when the image does not fit ``out`` (nothing
        is written then).  ``total`` and ``status`` are the tree's own two
        tensors, which the next ``snapshot`` call of this tree writes again:
        read or clone them before it.  Capturable with ``out``."""
        L = _lib.lib()
        if self.snap_ws is None:
            self.snap_ws = (
                torch.empty(L.tree_snap_workspace(self.cap), dtype=U8,
                            device=self.device),
                torch.zeros(2, dtype=I64, device=self.device),
                torch.zeros(2, dtype=I64, device=self.device))
        ws, total, status = self.snap_ws
        acl = self.acl or []
        _lib.tree_snap_size(self._tensors, acl, ws, total)
        if out is not None:
            _lib.tree_snap_write(self._tensors, acl, ws, out, out.numel(),
                                 status)
            return out, total, status
        img = torch.empty(int(total[0].item()), dtype=U8, device=self.device)
        _lib.tree_snap_write(self._tensors, acl, ws, img, img.numel(), status)
        return img

    @property
    def tensors(self):
        """The descriptor list of the tree for torch.ops.zkmi."""
        return self._tensors

    def _init_acl(self, acl_cap, arena_bytes):
        """The ACL table's tensors (zk_abi.h ZkAclTable, in the order
        csrc/torch/zkmi_ops.cpp acl_table() takes): a word per node, the
        arena of interned wire-format vectors, the intern index and the
        counters.  ZooKeeper's open ACL sits at arena offset 0 and every
        node starts bound to it (the static nodes answer it, as fakezk's
        pre-made nodes do).  ``arena_bytes`` defaults to 64 per ACL (the
        mix's two-entry digest ACL is 83 bytes, the open one 27)."""
        from .. import jute
        dev = self.device
        raw = B._acl_bytes(jute.DEFAULT_ACL)
        if arena_bytes is None:
            arena_bytes = 64 * acl_cap + 256
        arena_bytes = max(int(arena_bytes), len(raw))
        word = len(raw)                       # offset 0 << 24 | length
        node_acl = torch.full((self.cap,), word, dtype=I64, device=dev)
        arena = torch.zeros(arena_bytes, dtype=U8, device=dev)
        arena[:len(raw)] = torch.frombuffer(bytearray(raw), dtype=U8).to(dev)
        hcap = _next_pow2(2 * (acl_cap + 1))
        key = np.zeros(hcap, np.int64)
        val = np.zeros(hcap, np.int64)
        h = _lib.acl_hash(raw)
        s = (h >> 8) & (hcap - 1)
        key[s], val[s] = _i64(h), word
        ctr = [0] * 8
        ctr[_lib.AC_TOP] = ctr[_lib.AC_OLD_TOP] = len(raw)
        ctr[_lib.AC_ENT] = 1
        ctr[_lib.AC_LIMIT] = acl_cap + 1
        self.acl = [node_acl, arena, torch.from_numpy(key).to(dev),
                    torch.from_numpy(val).to(dev),
                    torch.tensor(ctr, dtype=I64, device=dev)]

    def acl_host(self, v):
        """The decoded ACL of node ``v`` read back from the ACL table, or
        None for a lost binding (host readback; tests)."""
        from .. import jute
        w = int(self.acl[0][v].item())
        if w == _lib.ACL_LOST:
            return None
        off, ln = w >> 24, w & 0xFFFFFF
        raw = bytes(self.acl[1][off:off + ln].cpu().numpy().tobytes())
        return jute.JuteReader(raw, 0).read_acl()

    def _watch_table(self, wh):
        """The tensors of an empty watch table of ``wh`` entries (zk_abi.h
        ZkTree wt_key / wt_mask): per entry the key and the second hash
        word; the data / child masks and then the counter words."""
        dev = self.device
        return (torch.zeros(2 * wh, dtype=I64, device=dev),
                torch.zeros(2 * wh + _lib.WT_STATS, dtype=I64, device=dev))

    @property
    def watch_hcap(self):
        """Entries of the watch table."""
        return self.watch[0].numel() // 2

    def expire(self, session, removed=None, rec=None):
        """Delete every ephemeral node owned by ``session`` (server side of
        session expiry).  ``removed`` (device int64 [1]) accumulates the
        number of nodes removed.

        On a tree with a watch table every removal fires what a DELETE
        fires (the node's data and child watches, its parent's child
        watches).  ``rec`` (device int64 [8 + 5 * k]) takes one record per
        removal that fired a watch, for k of them, and in ``rec[0]`` the
        number wanted: :meth:`GpuServer.expire` turns them into
        notifications.  Without it the fired watches are consumed and
        nobody is told."""
        if removed is None:
            removed = torch.zeros(1, dtype=I64, device=self.device)
        if rec is None:
            _lib.lib().tree_expire(self._tensors, session, self.cap, removed)
        else:
            rec[0:1].zero_()
            _lib.lib().tree_expire(self._tensors, session, self.cap, removed,
                                   rec, (rec.numel() - 8) // 5)
        return removed

    def watch_drop(self, wslot):
        """Clear watcher slot ``wslot``'s bit from every mask of the watch
        table: a closed or expired session's watches go with it (ZooKeeper
        keeps them on the connection), so nothing of it fires into the next
        session bound to the slot."""
        if self.watch is None:
            raise ValueError('watch_drop: the tree keeps no watch table')
        _lib.lib().watch_drop(self._tensors, int(wslot))

    def watch_rehash(self, watch_cap=None):
        """Rebuild the watch table from the entries that still hold a watch
        (a fire empties an entry's masks but leaves the entry, so every path
        ever watched takes one until this runs), into a table for
        ``watch_cap`` watched paths (default: the size it has).  The lost-arm
        count carries over.  Any server over the tree sees the new table at
        once (the descriptor list is updated in place)."""
        if self.watch is None:
            raise ValueError('watch_rehash: the tree keeps no watch table')
        wh = self.watch_hcap if watch_cap is None else \
            max(_next_pow2(2 * int(watch_cap)), 8)
        old = self.watch
        self.watch = self._watch_table(wh)
        self._tensors[18:20] = list(self.watch)
        _lib.lib().watch_rebuild(self._tensors, old[0], old[1])

    def watch_census(self):
        """(entries in use, entries holding a watch, arms lost to a full
        table) of the watch table.  One host read."""
        wh = self.watch_hcap
        key = self.watch[0][0:2 * wh:2]
        m = self.watch[1][:2 * wh].view(wh, 2)
        held = ((m[:, 0] | m[:, 1]) != 0)
        return (int((key != 0).sum().item()), int(held.sum().item()),
                int(self.watch[1][2 * wh + _lib.WS_LOST].item()))

    def rehash(self):
        """Rebuild the hash index from the live nodes (drops tombstones left
        by deleted paths that are never re-created, e.g. SEQUENTIAL names).
        One host read of the node high-water mark."""
        n = int(self.counters[_lib.TC_NODES].item())
        _lib.lib().tree_ht_reset(self._tensors)
        _lib.lib().tree_build(self._tensors, 0, min(n, self.cap))

    def digest(self):
        """(digest, live nodes, hash entries in use, tombstones): the digest
        is an order-independent hash of every live znode's path, czxid,
        mzxid, version, cversion / numChildren, pzxid, ephemeralOwner and
        data (times aside): two replicas of one tree agree on it whatever
        slots and hash entries their nodes sit in.  One host read."""
        out = torch.zeros(4, dtype=I64, device=self.device)
        _lib.lib().tree_digest(self._tensors, out)
        d, live, used, tomb = out.cpu().tolist()
        return d & ((1 << 64) - 1), live, used, tomb

    def free_compact(self):
        """Rebuild the free ring's pending entries as the free nodes in node
        order, on the device (csrc/kernels/tree.hip free_count_k): the next
        batch's creates take nodes from dense runs.  Capturable."""
        L = _lib.lib()
        if self.free_ws is None:
            self.free_ws = torch.empty(L.tree_free_workspace(self.cap),
                                       dtype=I64, device=self.device)
        L.tree_free_compact(self._tensors, self.free_ws)

    def free_order(self):
        """(pending free-ring entries, fraction of neighbours one apart):
        how much of the locality of the nodes the next creates get is left
        (one host read; probes)."""
        c = self.counters.cpu().tolist()
        h, pub = c[_lib.TC_FREE_HEAD], c[_lib.TC_FREE_PUB]
        if pub - h <= 1:
            return pub - h, 1.0
        idx = torch.arange(h, pub, device=self.device) % \
            self.free_list.numel()
        seg = self.free_list[idx]
        near = ((seg[1:] - seg[:-1]).abs() == 1).float().mean().item()
        return pub - h, near

    def sort_free(self):
        """Sort the pending entries of the free ring (the nodes the next
        creates take, in ring order): each workgroup's creates then get
        nodes from one dense run again, however the blocks of earlier
        batches interleaved their frees.  One host read of the ring
        bounds; returns the entries sorted."""
        c = self.counters.cpu().tolist()
        h, pub = c[_lib.TC_FREE_HEAD], c[_lib.TC_FREE_PUB]
        if pub - h <= 1:
            return 0
        idx = torch.arange(h, pub, device=self.device) % \
            self.free_list.numel()
        self.free_list[idx] = torch.sort(self.free_list[idx]).values
        return pub - h

    def find_host(self, path):
        """Node index of ``path`` (host scan of the path table; tests)."""
        n = min(int(self.counters[_lib.TC_NODES].item()), self.cap)
        want = path.encode()
        po = self.node_path_off[:n].cpu().numpy()
        pl = self.node_path_len[:n].cpu().numpy()
        par = self.node_parent[:n].cpu().numpy()
        arena = self.path_arena.cpu().numpy().tobytes()
        for v in range(n):
            if par[v] != -2 and pl[v] == len(want) and \
                    arena[po[v]:po[v] + pl[v]] == want:
                return v
        return -1

    def children_host(self, path):
        """Sorted child names of ``path`` from the node table read back to
        the host (``node_parent``, ``node_pw`` and the path arena; tests and
        debugging), or None when no live node has that path.  The same join
        the device list path does (:meth:`GpuServer.serve_list`)."""
        n = min(int(self.counters[_lib.TC_NODES].item()), self.cap)
        par = self.node_parent[:n].cpu().numpy()
        pw = self.node_pw[:n].cpu().numpy()
        arena = self.path_arena.cpu().numpy().tobytes()
        off, ln = pw >> 24, pw & 0xFFFFFF
        want = path.encode()
        node = -1
        for v in np.nonzero((par != NODE_FREE) & (ln == len(want)))[0]:
            if arena[off[v]:off[v] + ln[v]] == want:
                node = int(v)
                break
        if node < 0:
            return None
        skip = len(want) + 1
        return sorted(arena[off[v] + skip:off[v] + ln[v]].decode()
                      for v in np.nonzero(par == node)[0])

    def node_slot_host(self, v):
        """(data bytes, Stat) of node ``v`` read back from HBM (tests)."""
        from .. import jute
        off = int(self.slot_off[v].item())
        raw = bytes(self.slab[off:off + self.slot].cpu().numpy().tobytes())
        r = jute.JuteReader(raw, 0)
        st = r.read_stat()
        r.off = _lib.SLOT_LEN
        return r.read_buffer(), st


class _SubFrames(object):
    """One engine's class of a mixed batch: the compacted frame table the
    split wrote (``off``, ``length``) and its device ``count``."""

    def __init__(self, off, length, count):
        self.off, self.length, self.count = off, length, count


class SessionSegments(object):
    """The segment table of a session batch (:meth:`GpuServer.
    serve_sessions`; the rule: csrc/kernels/zk_sess.h): the batch is the
    whole frames of ``S`` connections, concatenated; connection s's bytes are
    ``rx[starts[s]:starts[s + 1]]``, its EPHEMERAL creates belong to
    ``sessions[s]`` and its reads arm watcher slot ``wslots[s]`` (-1: none).
    Device tensors: ``starts`` int64 [S + 1] (non-decreasing, ``starts[0]``
    0), ``sessions`` int64 [S], ``wslots`` int32 [S]."""

    def __init__(self, starts, sessions, wslots):
        S = int(sessions.numel())
        if S < 1 or int(starts.numel()) != S + 1 or int(wslots.numel()) != S:
            raise ValueError('SessionSegments: starts [S + 1], sessions [S] '
                             'and wslots [S] with S >= 1')
        self.starts, self.sessions, self.wslots = starts, sessions, wslots
        self.S = S


class OrderDefer(object):
    """Where ``serve_sessions_mixed(ordered=True, defer=...)`` leaves what it
    deferred, for a table of ``S`` segments; all device tensors, nothing is
    read back:

    ``clipf``     int64 [S]: the first deferred frame of segment s, an index
                  in the whole batch's frame table (``cap_frames``: none);
    ``rep_end``   int64 [S]: connection s's replies are ``out[rep_off[s]:
                  rep_end[s]]`` (the placeholders of its deferred frames lie
                  behind and are never sent);
    ``used``      int64 [S]: the request bytes of segment s that were
                  consumed; the rest, from its first deferred frame on, is to
                  be sent again in the next batch;
    ``deferred``  int64 [1]: the frames deferred."""

    def __init__(self, S, device):
        self.S = int(S)
        self.clipf = torch.zeros(self.S, dtype=I64, device=device)
        self.rep_end = torch.zeros(self.S, dtype=I64, device=device)
        self.used = torch.zeros(self.S, dtype=I64, device=device)
        self.deferred = torch.zeros(1, dtype=I64, device=device)


class _SegState(object):
    """What :meth:`GpuServer.serve_sessions` leaves on the device about the
    last session batch's segments."""

    def __init__(self, cap_frames, S, dev):
        self.S = S
        self.f_seg = torch.zeros(cap_frames, dtype=I32, device=dev)
        self.first = torch.zeros(S + 1, dtype=I64, device=dev)
        self.rep_off = torch.zeros(S + 1, dtype=I64, device=dev)
        self.state = torch.zeros(S, dtype=I32, device=dev)
        self.bad = torch.zeros(2, dtype=I64, device=dev)
        self.f_seg_c = None               # per engine class (lazy)

    def class_tables(self):
        """``f_seg`` through the split of a batch of any op mix
        (:meth:`GpuServer.serve_sessions_mixed`): three int32 [cap_frames]
        tables, class c's frame -> segment; allocated on first use."""
        if self.f_seg_c is None:
            cap = int(self.f_seg.numel())
            buf = torch.zeros(3 * cap, dtype=I32, device=self.f_seg.device)
            self.f_seg_c = [buf[c * cap:(c + 1) * cap] for c in range(3)]
        return self.f_seg_c

    def table(self, segs, cls=None):
        """The segment table as the session ops take it, ``[f_seg, sessions,
        wslots, seg_state, bad]``, of :class:`SessionSegments` ``segs``: the
        whole batch's, or with ``cls`` engine class ``cls``'s."""
        f_seg = self.f_seg if cls is None else self.class_tables()[cls]
        return [f_seg, segs.sessions, segs.wslots, self.state, self.bad]


def _table_args(table):
    """The keywords through which a session op takes a
    :class:`GpuSessionTable` (or none)."""
    if table is None:
        return {'table': None, 'server_id': 0, 'span': 0}
    return {'table': table._tensors, 'server_id': table.server_id,
            'span': table.span}


class GpuServer(object):
    """Server half of the pipeline: frame-scan + decode requests, apply them
    to a :class:`GpuTree`, encode replies."""

    def __init__(self, tree, cap_frames, out_cap, window=2048,
                 seq_order=True, group=_SRV_GROUP, fused_rows=False):
        self.tree = tree
        # fused_rows: :meth:`serve` scans the requests with K1's rows pass
        # deferred and the serve kernel reads the scan's tile lists (one
        # launch less; csrc/kernels/zk_frame_rows.h).  Only where the serve
        # is the frame table's first reader: unordered, no SEQUENTIAL
        # numbering, no ACL table, no watch resume.
        if fused_rows and (tree.acl is not None or
                           (seq_order and cap_frames <= _SEQ_MAX)):
            raise ValueError('fused_rows: the serve must be the first '
                             'reader of the frame table (no seq_order, no '
                             'ACL table)')
        self.fused_rows = fused_rows
        self.window = window              # K1 entry window of the requests
        # SEQUENTIAL creates numbered in stream order before each serve
        # (csrc/kernels/tree_seq.hip: five launches); a server whose
        # batches never carry one (the GET pipeline, the write mixes
        # without SEQUENTIAL) skips them.  Off, a SEQUENTIAL create still
        # gets a unique number, in arrival order.
        self.seq_order = seq_order and cap_frames <= _SEQ_MAX
        self.seq_ws = None
        self.seqno = None
        # batches of GET_DATA / EXISTS only (the GET pipeline): the serve's
        # read-only instance (no claim / free / dirty-parent barriers; any
        # other op is refused UNIMPLEMENTED)
        self.read_only = False
        dev = tree.device
        self.rt = B.alloc_request_table(cap_frames, dev)
        # CREATE replies carry the created path from the tree's arena
        # (a SEQUENTIAL name differs from the requested one)
        self.resp = B.ResponseBatch(
            torch.empty(cap_frames, dtype=I32, device=dev),
            torch.empty(cap_frames, dtype=I32, device=dev),
            torch.empty(cap_frames, dtype=I32, device=dev),
            torch.empty(cap_frames, dtype=I64, device=dev),
            torch.empty(cap_frames, dtype=I64, device=dev),
            torch.zeros(cap_frames, dtype=I64, device=dev),
            torch.zeros(cap_frames, dtype=I32, device=dev),
            tree.path_arena,
            torch.zeros(cap_frames, dtype=I32, device=dev), None,
            torch.empty(cap_frames, dtype=I64, device=dev))
        # the serve kernel sizes the replies itself (presized K13 encode)
        self.presized = B.response_workspace(cap_frames, dev)
        self.out = torch.empty(out_cap, dtype=U8, device=dev)
        self.cap_frames = cap_frames
        self.scanner = B.FrameScanner(cap_frames, dev, window=window,
                                      group=group)
        self.ows = None                   # ordered-serve workspace (lazy)
        self.total_err = B._total_err(dev)  # the reply encode's scalars
        self.notif = None
        self.seg = None                   # the last session batch's segments
        self.notif_slots = None           # (slot_first, slot_off) of its
        self._grouped = None              # notifications (buffers: lazy)
        self.resume_notif = None          # the last SET_WATCHES catch-up
        self.resume_slots = None          # (slot_first, slot_off) of a
        self._rs = None                   # session batch's (buffers: lazy)
        self.close_notif = None           # what the last close pass fired
        self.close_slots = None           # (slot_first, slot_off) of it
        self._cl = None                   # (buffers: lazy)
        if tree.watch is not None:
            self._init_watch(cap_frames, dev)

    # -- watches --------------------------------------------------------------

    def _init_watch(self, cap, dev):
        """Buffers of the watch events of one batch: the masks each write
        fired (5 words per request), then per event the watcher slot,
        notification type and path, and their K13 encode as xid -1
        notification frames (``NOTIFICATION``, state SyncConnected)."""
        ecap = 3 * cap + 64
        self.ecap = ecap
        self.fired = torch.zeros(5 * cap, dtype=I64, device=dev)
        self.wbsum = torch.empty((cap + 255) // 256, dtype=I64, device=dev)
        self.ev_slot = torch.empty(ecap, dtype=I32, device=dev)
        self.ev_type = torch.empty(ecap, dtype=I32, device=dev)
        self.ev_poff = torch.empty(ecap, dtype=I64, device=dev)
        self.ev_plen = torch.empty(ecap, dtype=I32, device=dev)
        # [events written (<= ecap), events fired]
        self.ev_total = torch.zeros(2, dtype=I64, device=dev)
        # [events written, re-armed, events, listed paths dropped]
        self.rs_out = torch.zeros(4, dtype=I64, device=dev)
        self.notif_err = None             # K13's error flag of the last
        self.resume_err = None            # notification / catch-up encode
        self.exp_rec = None               # expiry records (lazy)
        # notification frame: 4 + 16 header + type + state + path
        self.maxpath = int(self.tree.node_path_len.max().item()) + 16
        self.notif_buf = torch.empty(ecap * (28 + 4 + self.maxpath) + 64,
                                     dtype=U8, device=dev)
        self._nresp = self._notif_batch(self.ev_poff, self.ev_plen,
                                        self.tree.path_arena, self.ev_type,
                                        self.ev_total[0:1], ecap, dev)

    @staticmethod
    def _notif_batch(poff, plen, arena, ntype, count, cap, dev):
        """ResponseBatch of `cap` notification records (xid -1, zxid -1)."""
        return B.ResponseBatch(
            torch.full((cap,), consts.OP_CODES['NOTIFICATION'], dtype=I32,
                       device=dev),
            torch.full((cap,), consts.XID_NOTIFICATION, dtype=I32,
                       device=dev),
            torch.zeros(cap, dtype=I32, device=dev),
            torch.full((cap,), -1, dtype=I64, device=dev),
            torch.full((cap,), -1, dtype=I64, device=dev),
            poff, plen, arena, ntype, count)

    def _notify(self, op=None, err=None, count=None, fired=None):
        """Expand the fired masks of the last serve (or the records of an
        expiry: ``op`` .. ``fired``) into events (request order) and encode
        them: ``self.notif = (stream, bytes, slot per frame, events)`` — the
        watchers' notification frames, all on the device.  Events past
        ``self.ecap`` are not written (their watches are spent all the
        same) and the encoder's error flag is kept: :meth:`watch_stats`
        reports both."""
        L = _lib.lib()
        if op is None:
            r = self.resp
            op, err, count, fired = r.opcode, r.err, r.count, self.fired
        L.watch_events(op, err, count, self.cap_frames, fired,
                       self.wbsum, self.ev_slot, self.ev_type, self.ev_poff,
                       self.ev_plen, self.ev_total)
        out, rec_off, total, nerr = B.encode_responses(
            self._nresp, self.tree.store, self.notif_buf.numel(),
            out=self.notif_buf)
        self.notif_rec_off = rec_off
        self.notif_err = nerr
        self.notif = (out, total, self.ev_slot, self.ev_total[0:1])

    def expire(self, session, wslot=None, removed=None):
        """Expire ``session``: its ephemerals are removed as one txn
        (:meth:`GpuTree.expire`) and, on a tree with a watch table, the
        watches the removals fire become ``self.notif`` as a served batch's
        do (NodeDeleted to the data and child watchers of each removed node,
        one a watcher; NodeChildrenChanged to its parent's), in no
        particular order.  ``wslot``: the expired session's watcher slot;
        its own watches are dropped first (:meth:`GpuTree.watch_drop`), as
        ZooKeeper drops a closed session's, so it is told nothing and the
        slot's next session inherits nothing.  Returns ``removed``.

        Room for ``cap_frames`` removals that fire a watch; more are counted
        in :meth:`watch_stats` and their events lost."""
        tree = self.tree
        if tree.watch is None:
            return tree.expire(session, removed)
        dev = tree.device
        if wslot is not None:
            tree.watch_drop(wslot)
        if self.exp_rec is None:
            cap = self.cap_frames
            self.exp_rec = torch.zeros(8 + 5 * cap, dtype=I64, device=dev)
            self.exp_op = torch.full((cap,), consts.OP_CODES['DELETE'],
                                     dtype=I32, device=dev)
            self.exp_err = torch.zeros(cap, dtype=I32, device=dev)
        removed = tree.expire(session, removed, rec=self.exp_rec)
        self._notify(self.exp_op, self.exp_err, self.exp_rec[0:1],
                     self.exp_rec[8:])
        return removed

    def watch_stats(self):
        """The watch path's loss counters (one host read), all 0 on a
        server that lost nothing:

        ``lost_arms``       watches that found no entry in a full table since
                            the tree was built (:meth:`GpuTree.watch_rehash`
                            is the remedy); their watchers will not be told
        ``events_fired``,   of the last serve / expiry: more fired than
        ``events_written``  written means ``ecap`` overflowed and the rest
                            were dropped, their watches spent
        ``encode_err``      the notification encoder's error flag of the last
                            serve / expiry (2: ``notif_buf`` too small)
        ``expiry_dropped``  removals of the last :meth:`expire` whose fired
                            watches found no record
        ``resume_dropped``, paths of the last SET_WATCHES catch-up that were
        ``resume_err``      neither answered nor re-armed; its encoder's flag
        """
        wh = self.tree.watch_hcap
        ev = self.ev_total.cpu().tolist()
        st = {'lost_arms':
              int(self.tree.watch[1][2 * wh + _lib.WS_LOST].item()),
              'events_fired': ev[1], 'events_written': ev[0],
              'encode_err': 0 if self.notif_err is None
              else int(self.notif_err.item()),
              'expiry_dropped': 0, 'resume_dropped': 0, 'resume_err': 0}
        if self.exp_rec is not None:
            st['expiry_dropped'] = max(
                0, int(self.exp_rec[0].item()) - self.cap_frames)
        if self.resume_err is not None:
            rs = self.rs_out.cpu().tolist()
            st['resume_dropped'] = rs[3] + rs[2] - rs[0]
            st['resume_err'] = int(self.resume_err.item())
        return st

    def _resume(self, rx, ft, wslot):
        """SET_WATCHES catch-up of the batch's SET_WATCHES frames for
        watcher ``wslot`` (csrc/kernels/tree_watch.hip wt_resume_k): events for
        what changed after relZxid, encoded with the request bytes as path
        arena; the other watches are re-armed."""
        L = _lib.lib()
        dev = self.tree.device
        # a listed path takes at least the 4 bytes of its length in its
        # frame: no list of this stream is longer than its bytes / 4
        cap = max(self.ecap, int(rx.numel()) // 4)
        ev_type = torch.empty(cap, dtype=I32, device=dev)
        ev_poff = torch.empty(cap, dtype=I64, device=dev)
        ev_plen = torch.empty(cap, dtype=I32, device=dev)
        ent = torch.empty(cap, dtype=I64, device=dev)
        L.watch_resume(self.tree.tensors, rx, ft.off, ft.length, ft.count,
                       self.cap_frames, wslot, ent, ev_type, ev_poff, ev_plen,
                       self.rs_out)
        nb = self._notif_batch(ev_poff, ev_plen, rx, ev_type,
                               self.rs_out[0:1], cap, dev)
        # paths of a SET_WATCHES are bounded by its frame: ZooKeeper paths
        buf = torch.empty(cap * 32 + int(rx.numel()) + 64, dtype=U8,
                          device=dev)
        out, _, total, rerr = B.encode_responses(nb, self.tree.store,
                                                 buf.numel(), out=buf)
        self.resume_err = rerr
        self.resume_notif = (out, total, self.rs_out)

    def serve(self, rx, n, session=0, terminate=False, ordered=False,
              passes=4, wslot=-1, resume=False):
        """Serve the request stream ``rx[:n]`` for ``session`` (the owner of
        any EPHEMERAL node it creates).  ``n`` is a host length or the
        request encoder's device total (no host read).  Returns the reply
        stream buffer, its device total, the encoder error flag and the
        request frame table.

        ``ordered``: requests on one path are applied in stream order when
        one of them writes it (``passes`` launches; a path with more than
        ``passes`` requests in the batch has the excess answered
        SYSTEMERROR, see :meth:`order_stats`).  Reads and sets followed by
        a write to their path snapshot their reply into the tree's
        ``scratch``.  Without it requests of a batch are concurrent.

        On a tree with an ACL table (``GpuTree(acl_cap=...)``) every
        successful CREATE's ACL is recorded after the serve (two launches,
        csrc/kernels/tree_acl.hip).  A GET_ACL in the batch is answered
        UNIMPLEMENTED here: GET_ACL batches go through :meth:`serve_acl`,
        batches that mix it (or the list ops) with these through
        :meth:`serve_mixed`."""
        for _ in self.serve_steps(rx, n, session, terminate, ordered, passes,
                                  wslot, resume):
            pass
        return self.result

    def serve_steps(self, rx, n, session=0, terminate=False, ordered=False,
                    passes=4, wslot=-1, resume=False, frames=None):
        """:meth:`serve` as a generator yielding once, between the request
        decode and the tree; the return tuple lands in ``self.result`` (a
        pipelined caller interleaves another connection's work there).

        ``frames``: a frame table of ``rx`` to serve instead of scanning
        ``rx[:n]`` (``off``, ``length`` and a device ``count``:
        :meth:`serve_mixed` passes the serve's class of the batch); the
        reply frame starts then go to ``self.mix_rec_off[0]``."""
        L = _lib.lib()
        if self.fused_rows and (ordered or resume or self.seq_order or
                                self.tree.acl is not None or
                                frames is not None):
            raise ValueError('fused_rows: the serve must be the first '
                             'reader of the frame table (not ordered, no '
                             'seq_order, no ACL table, no watch resume)')
        if frames is not None:
            ft, tiles = frames, None
        else:
            ft = self.scanner.scan(rx, n, rows=not self.fused_rows)
            # (None for a request stream of one tile at most: the plain serve)
            tiles = self.scanner.pending
        # ordered serving ranks the batch from K12's request table; the
        # plain serve parses each frame in registers instead
        rt = B.decode_requests(rx, ft, out=self.rt) if ordered else None
        yield
        r = self.resp
        r.count = ft.count
        out = [r.opcode, r.xid, r.err, r.node, r.zxid, r.path_off,
               r.path_len, r.slot, self.presized[0], self.presized[1]]
        now = int(time.time() * 1000)
        seqno = self._seq_order(rx, ft) if self.seq_order else None
        if ordered:
            if self.ows is None:
                self.ows = torch.empty(
                    L.tree_order_workspace(self.cap_frames), dtype=U8,
                    device=self.tree.device)
            L.tree_serve_ordered(self.tree.tensors, rx, rt.tensors(),
                                 ft.count, self.cap_frames, out, session,
                                 now, self.ows, passes, self.tree.scratch,
                                 wslot, self.fired if self.tree.watch
                                 is not None else None, seqno)
        else:
            fired = self.fired if self.tree.watch is not None else None
            if tiles is not None:
                # the rows-deferred scan's consumer: it writes ft's rows
                L.tree_serve_tiles(self.tree.tensors, rx, tiles.n_dev,
                                   tiles.ncap, tiles.ws, ft.off, ft.length,
                                   ft.count, self.cap_frames, out, session,
                                   now, wslot, fired, seqno, self.read_only)
                tiles.consumed()
            else:
                L.tree_serve_frames(self.tree.tensors, rx, ft.off, ft.length,
                                    ft.count, self.cap_frames, out, session,
                                    now, wslot, fired, seqno, self.read_only)
            # the finish and K13's block-sum scan: one launch
            L.tree_finish_scan(self.tree.tensors, ft.count, 0, True,
                               self.cap_frames, self.presized[1],
                               self.total_err[0])
        if self.tree.acl is not None and not self.read_only:
            # the batch's successful CREATEs bind their ACLs
            _lib.tree_acl_record(self.tree.acl, rx, ft.off, ft.length,
                                 ft.count, self.cap_frames, r.opcode, r.err,
                                 r.node, self._acl_workspace())
        out, rec_off, total, err = B.encode_responses(
            r, self.tree.store, self.out.numel(), out=self.out,
            presized=self.presized, terminate=terminate,
            total_err=self.total_err, prescanned=not ordered,
            rec_off=self.mix_rec_off[0] if frames is not None else None)
        if self.tree.compact_free:
            self.tree.free_compact()
        self.last_rec_off = rec_off         # reply frame starts (R2 splits)
        self.result = (out, total, err, ft)
        if self.tree.watch is not None:
            self._notify()
            if resume:
                if wslot < 0:
                    raise ValueError('resume needs the watcher slot')
                self._resume(rx, ft, wslot)

    # -- session batches ------------------------------------------------------

    def _notify_grouped(self):
        """:meth:`_notify` for a session batch: the events of the last serve
        grouped by watcher slot (csrc/kernels/tree_sess.hip; request order
        inside a slot) before K13 encodes them, so every watcher's
        notifications are one slice of the stream.  ``self.notif`` as
        :meth:`_notify` leaves it, slot-major; the slices come from
        ``self.notif_slots`` once :func:`_lib.sess_ranges` ran."""
        L = _lib.lib()
        dev = self.tree.device
        if self._grouped is None:
            ecap = self.ecap
            g = {'slot': torch.zeros(ecap, dtype=I32, device=dev),
                 'type': torch.zeros(ecap, dtype=I32, device=dev),
                 'poff': torch.zeros(ecap, dtype=I64, device=dev),
                 'plen': torch.zeros(ecap, dtype=I32, device=dev),
                 'ws': torch.empty(_lib.sess_group_workspace(ecap),
                                   dtype=I64, device=dev),
                 'first': torch.zeros(_lib.SESS_SLOTS + 1, dtype=I64,
                                      device=dev),
                 'off': torch.zeros(_lib.SESS_SLOTS + 1, dtype=I64,
                                    device=dev),
                 'total_err': B._total_err(dev)}
            g['resp'] = self._notif_batch(g['poff'], g['plen'],
                                          self.tree.path_arena, g['type'],
                                          self.ev_total[0:1], ecap, dev)
            g['rec_off'] = torch.zeros(ecap, dtype=I64, device=dev)
            self._grouped = g
        g = self._grouped
        r = self.resp
        L.watch_events(r.opcode, r.err, r.count, self.cap_frames, self.fired,
                       self.wbsum, self.ev_slot, self.ev_type, self.ev_poff,
                       self.ev_plen, self.ev_total)
        _lib.sess_group_events(self.ev_slot, self.ev_type, self.ev_poff,
                               self.ev_plen, self.ev_total, g['ws'],
                               g['slot'], g['type'], g['poff'], g['plen'],
                               g['first'])
        out, rec_off, total, nerr = B.encode_responses(
            g['resp'], self.tree.store, self.notif_buf.numel(),
            out=self.notif_buf, total_err=g['total_err'],
            rec_off=g['rec_off'])
        self.notif_rec_off = rec_off
        self.notif_err = nerr
        self.notif = (out, total, g['slot'], self.ev_total[0:1])
        self.notif_slots = (g['first'], g['off'])

    def _resume_sessions(self, rx, ft, seg_table, rec_off, total, err):
        """The SET_WATCHES catch-up of the session batch just served
        (csrc/kernels/tree_resume.hip; the rules: zk_resume.h): every
        SET_WATCHES frame of ``ft`` for its own segment's watcher slot,
        against the tree as the batch left it.  Leaves ``self.resume_notif``
        and ``self.resume_slots``; nothing is read back.  The buffers are
        allocated on first use and grown when a larger ``rx`` comes."""
        dev = self.tree.device
        sg = self.seg
        # a listed path takes at least the 4 bytes of its length in its
        # frame: no batch lists more paths than its bytes / 4, so the entry
        # and the event room (ecap of each) cannot overflow
        need = max(1, int(rx.numel()) // 4)
        b = self._rs
        if b is None or b['ecap'] < need:
            ecap = need
            rec = lambda: [torch.zeros(ecap, dtype=I32, device=dev),
                           torch.zeros(ecap, dtype=I32, device=dev),
                           torch.zeros(ecap, dtype=I64, device=dev),
                           torch.zeros(ecap, dtype=I32, device=dev)]
            b = {'ecap': ecap, 'ev': rec(), 'g': rec(),
                 'ev_total': torch.zeros(2, dtype=I64, device=dev),
                 'ws': torch.empty(_lib.watch_resume_sessions_workspace(
                     self.cap_frames, ecap), dtype=I64, device=dev),
                 'first': torch.zeros(_lib.SESS_SLOTS + 1, dtype=I64,
                                      device=dev),
                 'off': torch.zeros(_lib.SESS_SLOTS + 1, dtype=I64,
                                    device=dev),
                 'stats': torch.zeros(8, dtype=I64, device=dev),
                 'total_err': B._total_err(dev),
                 'rec_off': torch.zeros(ecap, dtype=I64, device=dev),
                 # as _resume sizes it: 32 bytes of frame around a path, and
                 # the paths are the request's own bytes (rx <= 4 ecap + 3)
                 'buf': torch.empty(ecap * 32 + 4 * ecap + 4 + 64, dtype=U8,
                                    device=dev)}
            g = b['g']
            b['resp'] = self._notif_batch(g[2], g[3], rx, g[1],
                                          b['ev_total'][0:1], ecap, dev)
            self._rs = b
        b['resp'].path_arena = rx           # the encode arena: the requests
        _lib.watch_resume_sessions(
            self.tree.tensors, rx, ft.off, ft.length, ft.count,
            self.cap_frames, seg_table, b['ws'], b['ev'], b['ev_total'],
            b['g'], b['first'], b['stats'])
        out, _, rtotal, rerr = B.encode_responses(
            b['resp'], self.tree.store, b['buf'].numel(), out=b['buf'],
            total_err=b['total_err'], rec_off=b['rec_off'])
        _lib.sess_ranges(sg.first, rec_off, ft.count, self.cap_frames, total,
                         err, sg.rep_off, b['first'], b['rec_off'],
                         b['ev_total'][0:1], b['total_err'][0],
                         b['total_err'][1], b['off'])
        self.resume_notif = (out, rtotal, b['g'][0], b['ev_total'][0:1])
        self.resume_slots = (b['first'], b['off'])

    def resume_stats(self):
        """Of the last session batch served with ``resume=True`` (one host
        read): ``events`` the catch-up found and ``events_written`` (fewer:
        the event room overflowed), watches ``rearmed``, paths ``listed`` by
        the frames that were caught up, ``dropped`` (listed paths past the
        entry room, neither answered nor re-armed), ``no_slot`` (paths of
        live SET_WATCHES frames whose segment's watcher slot is outside
        0..63) and ``encode_err`` (the catch-up encoder's flag; 2:
        the notification buffer is too small)."""
        b = self._rs
        if b is None:
            raise ValueError('resume_stats: no session batch was resumed')
        v = torch.cat([b['stats'][:len(_lib.RESUME_STATS)],
                       b['total_err'][1].to(I64)]).cpu().tolist()
        st = dict(zip(_lib.RESUME_STATS, v))
        st['encode_err'] = v[-1]
        return st

    def resume_counters(self):
        """The device counters :meth:`resume_stats` reads (int64 [8], in
        ``_lib.RESUME_STATS`` order), for a caller that folds them into a
        read of its own (the front end's report); no host read."""
        if self._rs is None:
            raise ValueError('resume_counters: no session batch was resumed')
        return self._rs['stats']

    def serve_sessions(self, rx, n, segs, ordered=False, passes=4,
                       terminate=False, table=None, resume=False,
                       close=False):
        """Serve ``rx[:n]``, the concatenated whole frames of the
        ``segs.S`` connections of :class:`SessionSegments` ``segs``, as ONE
        batch: one K1 scan and one serve (``passes`` of them when
        ``ordered``), each frame for its own segment's session and watcher
        slot (csrc/kernels/tree_sess.hip, the serve's MS instances).  ``n``
        is a host length or a device total; nothing is read back and the
        call is capturable where :meth:`serve` is.  Returns ``(out, total,
        err, frame table)`` like :meth:`serve`, and leaves

        ``self.seg``          ``.f_seg`` (segment per frame), ``.first``
                              (first frame per segment, [S + 1]),
                              ``.rep_off`` ([S + 1]: connection s's replies
                              are ``out[rep_off[s]:rep_off[s + 1]]``),
                              ``.state`` ([S]: 1 = session not alive) and
                              ``.bad`` ([2]);
        ``self.notif``        as :meth:`serve` does, but slot-major;
        ``self.notif_slots``  ``(slot_first, slot_off)``, both [65]: watcher
                              w's notifications are ``notif_buf[slot_off[w]:
                              slot_off[w + 1]]``, in request order.

        A frame that crosses a segment boundary, a ``starts`` that does not
        begin at 0 or descends: every request of the batch is answered
        SYSTEMERROR and nothing is touched (:meth:`session_stats`).
        ``table``: a :class:`GpuSessionTable`; a segment whose session (other
        than 0) it does not hold alive has its requests answered
        SESSION_EXPIRED, without effect.  (A SEQUENTIAL create refused this
        way leaves a gap in its parent's cversion, as any failed numbered
        create does.)

        The list ops and GET_ACL are not served here (UNIMPLEMENTED): a
        session batch that mixes them in goes through
        :meth:`serve_sessions_mixed` (``ordered`` there as here, for the
        serve's class).  How a connection's notification slices are
        interleaved with its reply slice on the socket is the front end's
        business.

        ``resume``: the SET_WATCHES catch-up (csrc/kernels/tree_resume.hip),
        on a tree with a watch table (``ValueError`` without one).  Off, a
        SET_WATCHES frame gets its header-only reply and nothing else.  On,
        the reply is the same and every SET_WATCHES frame of the batch is
        caught up for its own segment's watcher slot ``wslots[s]`` by the
        session rule of :meth:`serve`'s ``resume`` (a listed data watch:
        node gone NodeDeleted, mzxid > relZxid NodeDataChanged, else
        re-armed; an exist watch: node there NodeCreated, else re-armed; a
        child watch: node gone NodeDeleted, pzxid > relZxid
        NodeChildrenChanged, else re-armed), each frame with its own
        relZxid, any number of them anywhere in a segment.  The catch-up
        reads the tree as the batch leaves it: it is as if every SET_WATCHES
        frame of the batch came after all its other frames, in stream order
        among themselves — so a write by another connection of the batch to
        a listed path is an event of the catch-up when its zxid is past the
        frame's relZxid, and never fires the re-armed watch (as
        ``serve(resume=True)`` treats the writes of its own batch).  Nothing
        is caught up, re-armed or sent for a refused batch, a segment whose
        session is not alive, a frame of no segment, a segment whose
        ``wslots`` value is outside 0..63 (its paths are counted ``no_slot``)
        or a frame that is not a well-formed SET_WATCHES.  It leaves, with no
        host read,

        ``self.resume_notif``  ``(buf, total, slots, count)``: the catch-up's
                               xid -1 frames grouped by watcher slot, inside
                               a slot in stream order (frame order, then the
                               data, exist and child lists, then list
                               order); the paths are the request's own bytes.
                               Apart from ``self.notif``, which stays the
                               batch's write-fired events;
        ``self.resume_slots``  ``(slot_first, slot_off)``, both [65]: watcher
                               w's catch-up is ``buf[slot_off[w]:slot_off[w +
                               1]]``.  A front end writes that slice before
                               the slot's slice of ``self.notif``: what the
                               catch-up reports happened before the batch's
                               re-armed watches could fire;

        and :meth:`resume_stats` reads its counters.  Its buffers are sized
        from ``rx.numel()``, allocated on first use and grown when a larger
        ``rx`` comes; a call that does not grow them is capturable where the
        call without ``resume`` is.

        ``close``: serve the batch's CLOSE_SESSION frames
        (csrc/kernels/tree_close.hip; the rules: zk_close.h).  Off, such a
        frame is answered UNIMPLEMENTED and nothing else.  On, a
        CLOSE_SESSION frame of a live segment of a sound table is answered OK
        (the same 20 bytes, its own xid) and closes its segment: the
        segment's session and watcher slot join the list of one
        :meth:`close_sessions` pass that runs after the serve, and after the
        ``resume`` catch-up when both are set — as if every CLOSE_SESSION
        frame of the batch came after all its other frames, in segment order
        among themselves (the k-th closing segment's removals carry zxid
        base + k + 1, base the counter after the batch's own zxids).  So
        frames of a segment after its CLOSE_SESSION are served (the
        reference client sends it only when nothing is outstanding);
        ephemerals the closing connection creates in the same batch go with
        it, while another connection's read in that batch still sees them;
        the batch's write-fired notifications addressed to a closing watcher
        stay in ``self.notif``, but nothing of the close pass is addressed
        to one, and what the catch-up re-armed for it is dropped.  A refused
        frame closes nothing: an unsound table (SYSTEMERROR), a segment
        whose session is not alive (SESSION_EXPIRED), a body shorter than 8
        bytes (BAD_ARGUMENTS).  With ``table`` the closed sessions' entries
        die: their next batch is answered SESSION_EXPIRED.  It leaves
        ``self.close_notif`` / ``self.close_slots`` as
        :meth:`close_sessions` does (a front end writes a watcher's
        ``resume_notif`` slice, then its ``notif`` slice, then its
        ``close_notif`` slice), ``self.close_removed`` (int64 [S]: nodes
        removed for the k-th closing segment) and the counters of
        :meth:`close_stats`; nothing is read back."""
        if self.fused_rows or self.read_only:
            raise ValueError('serve_sessions: no session form of the '
                             'read-only or the fused-rows serve')
        if not isinstance(segs, SessionSegments):
            raise TypeError('serve_sessions: segs is a SessionSegments')
        tree = self.tree
        if resume and tree.watch is None:
            raise ValueError('serve_sessions: resume needs a watch table')
        if self.seg is None or self.seg.S != segs.S:
            self.seg = _SegState(self.cap_frames, segs.S, tree.device)
        sg = self.seg
        ft = self.scanner.scan(rx, n)
        _lib.sess_assign(ft.off, ft.length, ft.count, self.cap_frames,
                         segs.starts, segs.sessions, sg.f_seg, sg.first,
                         sg.state, sg.bad, **_table_args(table))
        out, rec_off, total, err = self._serve_class(
            rx, ft, sg.table(segs), segs, ordered, passes, None, close, None,
            terminate)
        self.last_rec_off = rec_off
        self.result = (out, total, err, ft)
        self._sessions_tail(rx, ft, segs, rec_off, total, err, table, resume,
                            close, None)
        return self.result

    def _serve_class(self, rx, frames, seg_table, segs, ordered, passes,
                     defer, close, rec_off, terminate):
        """The serve of one class of a session batch's frames through to its
        reply encode: ``frames`` with their segment table ``seg_table``
        (:meth:`_SegState.table` of ``segs``) — the whole batch
        (:meth:`serve_sessions`) or the serve's class
        (:meth:`serve_sessions_mixed`).  ``defer``: the deferral's tables for
        ``tree_serve_ordered_sessions`` or None; ``rec_off``: where the
        encode leaves the frame starts (None: its own).  Returns what
        ``encode_responses`` returns."""
        L = _lib.lib()
        tree = self.tree
        cap = self.cap_frames
        r = self.resp
        r.count = frames.count
        out = [r.opcode, r.xid, r.err, r.node, r.zxid, r.path_off,
               r.path_len, r.slot, self.presized[0], self.presized[1]]
        now = int(time.time() * 1000)
        seqno = self._seq_order(rx, frames) if self.seq_order else None
        fired = self.fired if tree.watch is not None else None
        if ordered:
            rt = B.decode_requests(rx, frames, out=self.rt)
            if self.ows is None:
                self.ows = torch.empty(L.tree_order_workspace(cap), dtype=U8,
                                       device=tree.device)
            _lib.tree_serve_ordered_sessions(
                tree.tensors, rx, rt.tensors(), frames.count, cap, out, now,
                self.ows, passes, tree.scratch, fired, seqno, seg_table,
                defer)
        else:
            _lib.tree_serve_frames_sessions(
                tree.tensors, rx, frames.off, frames.length, frames.count,
                cap, out, now, fired, seqno, seg_table)
            L.tree_finish_scan(tree.tensors, frames.count, 0, True, cap,
                               self.presized[1], self.total_err[0])
        if tree.acl is not None:
            _lib.tree_acl_record(tree.acl, rx, frames.off, frames.length,
                                 frames.count, cap, r.opcode, r.err, r.node,
                                 self._acl_workspace())
        if close:
            self._close_frames(rx, frames, seg_table, segs.S)
        enc = B.encode_responses(
            r, tree.store, self.out.numel(), out=self.out,
            presized=self.presized, terminate=terminate,
            total_err=self.total_err, prescanned=not ordered,
            rec_off=rec_off)
        if tree.compact_free:
            tree.free_compact()
        return enc

    def _sessions_tail(self, rx, ft, segs, rec_off, total, err, table,
                       resume, close, defer):
        """What follows a session batch's replies (``rec_off`` / ``total`` /
        ``err``: the whole batch's reply stream over frame table ``ft``): the
        write-fired events, the reply and notification ranges, the
        SET_WATCHES catch-up, the deferral's ranges (``defer``: the
        :class:`OrderDefer` or None) and the close pass."""
        sg = self.seg
        cap = self.cap_frames
        if self.tree.watch is not None:
            self._notify_grouped()
            g = self._grouped
            _lib.sess_ranges(sg.first, rec_off, ft.count, cap, total, err,
                             sg.rep_off, g['first'], g['rec_off'],
                             self.ev_total[0:1], g['total_err'][0],
                             g['total_err'][1], g['off'])
            if resume:
                self._resume_sessions(rx, ft, sg.table(segs), rec_off, total,
                                      err)
        else:
            _lib.sess_ranges(sg.first, rec_off, ft.count, cap, total, err,
                             sg.rep_off)
        if defer is not None:
            _lib.order_clip_ranges(defer.clipf, sg.rep_off, rec_off, ft.off,
                                   segs.starts, ft.count, cap, defer.rep_end,
                                   defer.used)
        if close:
            self._close_batch(segs, table)

    def session_stats(self):
        """Of the last :meth:`serve_sessions` or
        :meth:`serve_sessions_mixed` (one host read): ``bad`` (torn
        frames + faults of the segment table; not 0: the batch was refused),
        ``first_bad_segment`` (-1: none) and ``expired_segments`` (segments
        whose session the table did not hold alive)."""
        if self.seg is None:
            raise ValueError('session_stats: no session batch was served')
        sg = self.seg
        v = torch.cat([sg.bad, (sg.state == 1).sum().view(1)]).cpu().tolist()
        return {'bad': v[0], 'first_bad_segment': v[1],
                'expired_segments': v[2]}

    # -- closing many sessions ------------------------------------------------

    def _close_buffers(self, S):
        """The close passes' buffers for lists of up to ``S`` sessions
        (csrc/kernels/tree_close.hip), allocated on first use and grown when
        a longer list comes; on a tree with a watch table also those of the
        events the removals fire, apart from the batch's own (``self.notif``
        keeps what the batch's writes fired)."""
        tree = self.tree
        dev = tree.device
        cap = self.cap_frames
        need = _lib.close_workspace(cap, S, tree.cap)
        b = self._cl
        if b is None:
            b = {'ws': None, 'stats': torch.zeros(8, dtype=I64, device=dev),
                 'removed': None}
            if tree.watch is not None:
                ecap = self.ecap
                rec = lambda: [torch.zeros(ecap, dtype=I32, device=dev),
                               torch.zeros(ecap, dtype=I32, device=dev),
                               torch.zeros(ecap, dtype=I64, device=dev),
                               torch.zeros(ecap, dtype=I32, device=dev)]
                b.update({
                    'ev': rec(), 'g': rec(),
                    'ev_total': torch.zeros(2, dtype=I64, device=dev),
                    'group_ws': torch.empty(_lib.sess_group_workspace(ecap),
                                            dtype=I64, device=dev),
                    'first': torch.zeros(_lib.SESS_SLOTS + 1, dtype=I64,
                                         device=dev),
                    'off': torch.zeros(_lib.SESS_SLOTS + 1, dtype=I64,
                                       device=dev),
                    'total_err': B._total_err(dev),
                    'rec_off': torch.zeros(ecap, dtype=I64, device=dev),
                    'buf': torch.empty(self.notif_buf.numel(), dtype=U8,
                                       device=dev),
                    # every record is a removal: a DELETE that succeeded
                    'op': torch.full((cap,), consts.OP_CODES['DELETE'],
                                     dtype=I32, device=dev),
                    'err': torch.zeros(cap, dtype=I32, device=dev),
                    # sess_ranges' reply half: one segment without a frame
                    'nil': (torch.zeros(2, dtype=I64, device=dev),
                            torch.zeros(1, dtype=I64, device=dev),
                            torch.zeros(1, dtype=I32, device=dev),
                            torch.zeros(2, dtype=I64, device=dev))})
                g = b['g']
                b['resp'] = self._notif_batch(g[2], g[3], tree.path_arena,
                                              g[1], b['ev_total'][0:1], ecap,
                                              dev)
            self._cl = b
        if b['ws'] is None or b['ws'].numel() < need:
            b['ws'] = torch.empty(need, dtype=I64, device=dev)
        if b['removed'] is None or b['removed'].numel() < S:
            b['removed'] = torch.zeros(S, dtype=I64, device=dev)
        return b

    def _close_frames(self, rx, frames, seg_table, S):
        """Pass 1 of a session batch served with ``close``: between the serve
        of ``frames`` and the encode of its replies."""
        b = self._close_buffers(S)
        _lib.close_frames(self.tree.tensors, rx, frames.off, frames.length,
                          frames.count, self.cap_frames, seg_table,
                          self.resp.err, self.cap_frames, b['ws'], b['stats'])

    def _close_batch(self, segs, table):
        """Passes 2-7 of a session batch served with ``close``, over the list
        :meth:`_close_frames` left on the device."""
        b = self._close_buffers(segs.S)
        self.close_removed = b['removed'][:segs.S]
        self.close_removed.zero_()
        self._close_pass(segs.S, None, None, table, self.close_removed)

    def _close_pass(self, S, sids, wslots, table, removed):
        """Passes 2-7 and, on a tree with a watch table, the events: the
        records of the removals' fired watches expanded, grouped by watcher
        slot and encoded, as :meth:`_notify_grouped` does a batch's."""
        tree = self.tree
        b = self._close_buffers(S)
        cap = self.cap_frames
        _lib.close_sessions(
            tree.tensors, sids, wslots, S, cap, b['ws'], removed, b['stats'],
            **_table_args(table))
        if tree.watch is None:
            return
        rec = b['ws'][:8 + 5 * cap]
        ev, g = b['ev'], b['g']
        _lib.lib().watch_events(b['op'], b['err'], rec[0:1], cap, rec[8:],
                                self.wbsum, ev[0], ev[1], ev[2], ev[3],
                                b['ev_total'])
        _lib.sess_group_events(ev[0], ev[1], ev[2], ev[3], b['ev_total'],
                               b['group_ws'], g[0], g[1], g[2], g[3],
                               b['first'])
        out, _, total, _ = B.encode_responses(
            b['resp'], tree.store, b['buf'].numel(), out=b['buf'],
            total_err=b['total_err'], rec_off=b['rec_off'])
        nil = b['nil']
        _lib.sess_ranges(nil[0], nil[1], nil[1], 1, nil[1], nil[2], nil[3],
                         b['first'], b['rec_off'], b['ev_total'][0:1],
                         b['total_err'][0], b['total_err'][1], b['off'])
        self.close_notif = (out, total, g[0], b['ev_total'][0:1])
        self.close_slots = (b['first'], b['off'])

    def close_sessions(self, sids, wslots=None, table=None, removed=None):
        """End the sessions ``sids`` (device int64 [K]) in ONE pass
        (csrc/kernels/tree_close.hip; the rules: zk_close.h): the sessions a
        front end's timer expired, or that it closes for reasons of its own.
        What K calls of :meth:`expire` (and one of
        :meth:`GpuSessionTable.close`) do with K sweeps of the node table
        and of the watch table, in one sweep of each; no host read.

        Session ``sids[k]``'s ephemerals are removed as its own closeSession
        txn, zxid base + k + 1, and the zxid counter moves by K: the tree is
        the one ``expire(sids[0]) ... expire(sids[K - 1])`` leaves.  An id
        listed twice removes at its first position, id 0 and an id that owns
        nothing remove nothing; each still takes its zxid.  Returns
        ``removed`` (device int64 [K], accumulated): the nodes removed for
        each listed session.

        ``wslots`` (device int32 [K]): the sessions' watcher slots.  On a
        tree with a watch table their bits are dropped from every mask
        before anything is removed (a value outside 0..63 drops nothing), so
        a closing session is told nothing and the next session bound to its
        slot inherits nothing; the watches the removals fire for the others
        are left in

        ``self.close_notif``  ``(buf, total, slots, count)``: the xid -1
                              frames grouped by watcher slot, in no defined
                              order inside a slot (as :meth:`expire`'s);
        ``self.close_slots``  ``(slot_first, slot_off)``, both [65]: watcher
                              w's are ``buf[slot_off[w]:slot_off[w + 1]]``.

        Room for ``cap_frames`` removals that fire a watch; more are counted
        by :meth:`close_stats` and their events lost.  ``table``: a
        :class:`GpuSessionTable`; the listed ids' entries close (an id it
        does not hold touches nothing)."""
        K = int(sids.numel())
        dev = self.tree.device
        if removed is None:
            removed = torch.zeros(K, dtype=I64, device=dev)
        if K == 0:
            return removed
        self._close_pass(K, sids, wslots, table, removed)
        return removed

    def close_stats(self):
        """Of the last close pass (:meth:`close_sessions`, or a session batch
        served with ``close=True``), one host read: ``frames`` (closing
        CLOSE_SESSION frames; 0 for the direct form), ``sessions`` (K),
        ``removed`` (nodes, all sessions), ``events_fired`` /
        ``events_written`` (fewer written: the event room overflowed),
        ``records_dropped`` (removals whose fired watches found no record:
        past ``cap_frames``) and ``encode_err`` (the events' encoder's flag;
        2: the notification buffer is too small)."""
        b = self._cl
        if b is None:
            raise ValueError('close_stats: no close pass has run')
        parts = [b['stats'][:3]]
        if self.tree.watch is not None:
            parts += [b['ev_total'], b['ws'][0:1],
                      b['total_err'][1].to(I64)]
        v = torch.cat(parts).cpu().tolist() + [0, 0, 0, 0]
        return dict(zip(_lib.CLOSE_STATS,
                        [v[0], v[1], v[2], v[4], v[3],
                         max(0, v[5] - self.cap_frames), v[6]]))

    def serve_list(self, rx, n, wslot=-1, terminate=False, max_frame=None,
                   out=None):
        """Serve a batch of list requests — GET_CHILDREN / GET_CHILDREN2
        frames only, ``rx[:n]`` (``n`` a host length or a device total) —
        from the tree (csrc/kernels/tree_list.hip: two sweeps of the node
        table per batch, no child links).  Returns ``(out, total, err,
        frame_table)`` like :meth:`serve`; the replies are in request order.

        Any other op in the batch is answered UNIMPLEMENTED, a truncated
        frame BAD_ARGUMENTS, a missing path NO_NODE — ``/`` included, which
        has no node in this tree (every op on it is NO_NODE).  The order of
        the names inside a reply is unspecified, as ZooKeeper's is.  A
        request with ``watch`` set that finds its node arms the child watch
        of watcher slot ``wslot`` (0..63; needs a tree with a watch table);
        a NO_NODE arms nothing.  A reply frame longer than ``max_frame``
        bytes (default: K1's 16 MiB cap) is answered SYSTEMERROR.  ``err``
        2 with ``total`` 0: the replies did not fit ``out`` (default: the
        server's reply buffer) and nothing was written.  Mixed batches go
        through :meth:`serve_mixed`.

        A sharded tree (``shard`` with world > 1) raises: its parents count
        children it does not index."""
        tree = self.tree
        if tree.shard is not None and tree.shard[1] > 1:
            raise ValueError('serve_list: a sharded tree does not index '
                             'every child of its parents')
        self._list_buffers()
        if out is None:
            out = self.out
        if max_frame is None:
            max_frame = consts.MAX_PACKET
        ft = self.scanner.scan(rx, n)
        total, err = self.list_total_err
        _lib.tree_list(tree.tensors, rx, ft.off, ft.length, ft.count,
                       self.cap_frames, wslot, max_frame, self.list_want,
                       self.list_ws, out, out.numel(), self.list_rec_off,
                       total, err, terminate)
        self.last_rec_off = self.list_rec_off
        self.result = (out, total, err, ft)
        return self.result

    def _list_buffers(self):
        """The list engine's buffers, allocated on first use."""
        if getattr(self, 'list_want', None) is not None:
            return
        dev = self.tree.device
        self.list_want = torch.full((self.tree.cap,), _lib.LIST_IDLE,
                                    dtype=I32, device=dev)
        self.list_ws = torch.empty(
            _lib.tree_list_workspace(self.cap_frames), dtype=U8, device=dev)
        self.list_rec_off = torch.empty(self.cap_frames, dtype=I64,
                                        device=dev)
        self.list_total_err = B._total_err(dev)

    def _acl_buffers(self):
        """The GET_ACL engine's buffers, allocated on first use."""
        if getattr(self, 'acl_rec_off', None) is not None:
            return
        dev = self.tree.device
        self.acl_rec_off = torch.empty(self.cap_frames, dtype=I64,
                                       device=dev)
        self.acl_total_err = B._total_err(dev)

    def _acl_workspace(self):
        if getattr(self, 'acl_ws', None) is None:
            self.acl_ws = torch.empty(
                _lib.tree_acl_workspace(self.cap_frames), dtype=U8,
                device=self.tree.device)
        return self.acl_ws

    def serve_acl(self, rx, n, terminate=False, out=None):
        """Serve a batch of GET_ACL frames, ``rx[:n]`` (``n`` a host length
        or a device total), from the tree and its ACL table
        (csrc/kernels/tree_acl.hip).  Returns ``(out, total, err,
        frame_table)`` like :meth:`serve`; the replies are in request order:
        the node's ACL as its CREATE sent it (the open ACL for the static
        nodes), then its Stat.

        Any other op in the batch is answered UNIMPLEMENTED, a truncated
        frame BAD_ARGUMENTS, a missing path NO_NODE (``/`` included: it has
        no node in this tree), and a node whose ACL found no room in the
        table SYSTEMERROR (see :meth:`acl_stats`); all header only.  ``err``
        2 with ``total`` 0: the replies did not fit ``out`` (default: the
        server's reply buffer) and nothing was written.  Mixed batches go
        through :meth:`serve_mixed`.

        Raises ``ValueError`` on a tree without an ACL table."""
        tree = self.tree
        if tree.acl is None:
            raise ValueError('serve_acl: the tree keeps no ACL table '
                             '(GpuTree(acl_cap=...))')
        self._acl_buffers()
        if out is None:
            out = self.out
        ft = self.scanner.scan(rx, n)
        total, err = self.acl_total_err
        _lib.tree_acl_get(tree.tensors, tree.acl, rx, ft.off, ft.length,
                          ft.count, self.cap_frames, self._acl_workspace(),
                          out, out.numel(), self.acl_rec_off, total, err,
                          terminate)
        self.last_rec_off = self.acl_rec_off
        self.result = (out, total, err, ft)
        return self.result

    def _mix_buffers(self):
        """The split's and the merge's buffers and the two engines' scratch
        streams, allocated on first use."""
        if getattr(self, 'mix_cls', None) is not None:
            return
        dev = self.tree.device
        cap = self.cap_frames
        self.mix_cls = torch.empty(cap, dtype=I32, device=dev)
        self.mix_sub = torch.empty(cap, dtype=I32, device=dev)
        self.mix_foff = torch.empty(3 * cap, dtype=I64, device=dev)
        self.mix_flen = torch.empty(3 * cap, dtype=I32, device=dev)
        self.mix_counts = torch.zeros(3, dtype=I64, device=dev)
        self.mix_frames = [
            _SubFrames(self.mix_foff[c * cap:(c + 1) * cap],
                       self.mix_flen[c * cap:(c + 1) * cap],
                       self.mix_counts[c:c + 1]) for c in range(3)]
        self.mix_split_ws = torch.empty(
            max(_lib.tree_mix_split_workspace(cap), 16), dtype=U8, device=dev)
        self.mix_merge_ws = torch.empty(
            max(_lib.tree_mix_merge_workspace(cap), 16), dtype=U8, device=dev)
        self._list_buffers()
        self._acl_buffers()
        # the serve's frame starts, then the merged ones
        self.mix_rec_off = (torch.empty(cap, dtype=I64, device=dev),
                            torch.empty(cap, dtype=I64, device=dev))
        self.mix_total_err = B._total_err(dev)
        # (a tree without an ACL table: the GET_ACL class stays empty)
        self.acl_total_err[0].zero_()
        self.acl_total_err[1].zero_()
        self.mix_scratch = (
            torch.empty(self.out.numel(), dtype=U8, device=dev)
            if self.tree.acl is not None else None,
            torch.empty(self.out.numel(), dtype=U8, device=dev))
        self.mix_out = torch.empty(self.out.numel(), dtype=U8, device=dev)

    def serve_mixed(self, rx, n, session=0, terminate=False, wslot=-1,
                    resume=False, max_frame=None, out=None):
        """Serve the request stream ``rx[:n]`` (``n`` a host length or a
        device total) whatever ops it mixes — what a session pipelines on one
        connection, what ``Client.bulk`` encodes — into one reply stream in
        request order.  Returns ``(out, total, err, frame_table)`` like
        :meth:`serve`, with the whole batch's frame table; ``out`` defaults
        to a buffer of the server's reply capacity (``self.mix_out``, not
        ``self.out``: the serve's own stream lands there).

        One K1 scan, then the split of the frame table by engine
        (csrc/kernels/tree_mix.hip): GET_CHILDREN / GET_CHILDREN2 to the
        list engine, GET_ACL to the ACL engine (on a tree with an ACL table),
        everything else — unknown opcodes, frames without an opcode word and
        GET_ACL on a tree without an ACL table included — to the fused serve,
        each answering as :meth:`serve_list`, :meth:`serve_acl` and
        :meth:`serve` (unordered) do.  The merge puts the three reply
        streams back into request order; ``self.last_rec_off`` holds the
        merged frame starts.

        The batch contract: the engines run in the fixed order serve,
        GET_ACL, list, each over its requests in request order.  So the
        writes of a batch are concurrent as in :meth:`serve` (``session``,
        ``wslot`` and ``resume`` as there; ``self.notif`` is what the
        batch's writes fired), and a GET_ACL or a list of a batch sees the
        tree after all of that batch's writes: a list of a parent shows the
        child created in the same batch and misses the one deleted in it, a
        GET_ACL returns the ACL of a node created in the same batch.  A
        ``watch=1`` list arms the child watch of slot ``wslot`` after the
        batch's writes: they do not fire it, the next batch's do.  In-batch
        ordering (``serve(ordered=True)``) is not offered.

        ``max_frame``: as in :meth:`serve_list`.  ``err`` is the first
        non-zero one of the serve's, the ACL engine's and the list engine's
        encoders (each stream has the server's reply capacity), else 2 when
        the merged stream does not fit ``out``; then ``total`` is 0 and
        ``out`` is untouched.

        A class without a member still costs its engine's launches: nothing
        is read back that could skip them.  After the first call has
        allocated the buffers a call without ``resume`` reads nothing back
        and allocates nothing; it can be captured in a HIP graph on one
        stream.

        Raises ``ValueError`` on a ``fused_rows`` server (the split must be
        the frame table's first reader) and on a sharded tree (``shard``
        with world > 1), as :meth:`serve_list` does."""
        tree = self.tree
        if self.fused_rows:
            raise ValueError('serve_mixed: a fused_rows server defers the '
                             'frame table\'s rows to the serve; the split '
                             'must be their first reader')
        if tree.shard is not None and tree.shard[1] > 1:
            raise ValueError('serve_mixed: a sharded tree does not index '
                             'every child of its parents')
        self._mix_buffers()
        cap = self.cap_frames
        if out is None:
            out = self.mix_out
        if max_frame is None:
            max_frame = consts.MAX_PACKET
        ft = self.scanner.scan(rx, n)
        _lib.tree_mix_split(rx, ft.off, ft.length, ft.count, cap,
                            tree.acl is not None, self.mix_cls, self.mix_sub,
                            self.mix_foff, self.mix_flen, self.mix_counts,
                            self.mix_split_ws)
        fa, fc, fl = self.mix_frames
        for _ in self.serve_steps(rx, n, session, False, False, 4, wslot,
                                  resume, frames=fa):
            pass
        a_out, a_total, a_err, _ = self.result
        c_out, l_out = self.mix_scratch
        c_total, c_err = self.acl_total_err
        if tree.acl is not None:
            _lib.tree_acl_get(tree.tensors, tree.acl, rx, fc.off, fc.length,
                              fc.count, cap, self._acl_workspace(), c_out,
                              c_out.numel(), self.acl_rec_off, c_total,
                              c_err, False)
        else:
            c_out = l_out
        l_total, l_err = self.list_total_err
        _lib.tree_list(tree.tensors, rx, fl.off, fl.length, fl.count, cap,
                       wslot, max_frame, self.list_want, self.list_ws, l_out,
                       l_out.numel(), self.list_rec_off, l_total, l_err,
                       False)
        total, err = self.mix_total_err
        _lib.tree_mix_merge(
            self.mix_cls, self.mix_sub, ft.count, self.mix_counts, cap,
            [a_out, c_out, l_out],
            [self.mix_rec_off[0], self.acl_rec_off, self.list_rec_off],
            [a_total, c_total, l_total], [a_err, c_err, l_err], out,
            out.numel(), self.mix_rec_off[1], total, err, self.mix_merge_ws,
            terminate)
        self.last_rec_off = self.mix_rec_off[1]
        self.result = (out, total, err, ft)
        return self.result

    def serve_sessions_mixed(self, rx, n, segs, terminate=False, table=None,
                             max_frame=None, out=None, resume=False,
                             close=False, ordered=False, passes=4,
                             defer=None):
        """Serve ``rx[:n]``, the concatenated whole frames of the ``segs.S``
        connections of :class:`SessionSegments` ``segs``, whatever ops they
        mix, as ONE batch: :meth:`serve_sessions` for every op of
        :meth:`serve_mixed`.  ``rx``, ``n``, ``segs`` and ``table`` as in
        :meth:`serve_sessions`; ``max_frame`` and ``out`` (default
        ``self.mix_out``) as in :meth:`serve_mixed`.  Returns ``(out, total,
        err, frame table)`` with the whole batch's frame table, and leaves
        ``self.seg`` (``f_seg``, ``first``, ``rep_off``, ``state``, ``bad``),
        ``self.notif``, ``self.notif_slots`` and ``self.last_rec_off`` (the
        merged frame starts) as those two do.  Nothing is read back, nothing
        is allocated after the first call (of a segment count), and the call
        can be captured on one stream where :meth:`serve_mixed` can.

        The batch contract.  One K1 scan and one segment assign over the
        whole frame table; the split of :meth:`serve_mixed`, the frames'
        segments carried through it (csrc/kernels/tree_sess.hip
        sess_split_seg_k); the engines in :meth:`serve_mixed`'s fixed order —
        serve (unordered), GET_ACL, list — each over its class's frames in
        request order, each frame for its own segment's session and watcher
        slot.  So a list or a GET_ACL from any connection sees the tree
        after all writes of the batch, from every connection.  A ``watch=1``
        list arms the child watch of its own segment's ``wslots[s]``, after
        the batch's writes (they do not fire it); a value outside 0..63 arms
        nothing.  ``self.seg.rep_off[s]`` slices the merged stream:
        connection s's replies are ``out[rep_off[s]:rep_off[s + 1]]``;
        ``notif_buf[slot_off[w]:slot_off[w + 1]]`` is watcher w's
        notifications, in request order.

        Refusals.  An unsound table (``bad != 0``: a torn frame, a
        ``starts`` that does not begin at 0 or descends) answers every
        request of the batch SYSTEMERROR, list and GET_ACL frames included;
        a segment whose session ``table`` does not hold alive has all its
        requests answered SESSION_EXPIRED.  For the list and ACL engines
        both are header-only replies with the xid the engine parsed: a
        refused frame looks nothing up, claims no parent and arms nothing.
        Refusal takes precedence over BAD_ARGUMENTS and UNIMPLEMENTED, as in
        the serve.

        ``err`` and overflow follow :meth:`serve_mixed`'s rule: the first
        non-zero one of the three engines' encoders, else 2 when the merged
        stream does not fit ``out``; then ``total`` is 0, ``out`` is
        untouched and ``rep_off`` is all zero.  On a tree without an ACL
        table GET_ACL goes to the serve (UNIMPLEMENTED), as in
        :meth:`serve_mixed`.

        ``resume``: the SET_WATCHES catch-up, as in :meth:`serve_sessions`
        (``self.resume_notif``, ``self.resume_slots``, :meth:`resume_stats`;
        ``ValueError`` on a tree without a watch table).  It runs once over
        the whole frame table and its segments, after the three engines: the
        tree it reads is the one the whole batch leaves, a listed path that
        any connection of the batch wrote is an event of the catch-up and
        never hits the re-armed watch, and a ``watch=1`` list of the batch is
        armed before it.  Off, a SET_WATCHES frame gets its header-only
        reply and nothing else; on, the replies are the same.

        ``close``: the batch's CLOSE_SESSION frames are served, as in
        :meth:`serve_sessions` (``self.close_notif``, ``self.close_slots``,
        ``self.close_removed``, :meth:`close_stats`).  The frame is of the
        serve's class; the close pass runs once, after the three engines and
        after the ``resume`` catch-up, so a list or a GET_ACL of the batch
        still sees a closing connection's ephemerals.

        ``ordered``: the serve's class goes through the ordered session serve
        (``serve_sessions(ordered=True)``: K12's request table over the
        class's frames, the ranking, ``passes`` serve launches), so requests
        of the serve's class that conflict (zk_tree_serve_ordered's rule: the
        same path with a writer among them, a create / delete and its
        parent's path) are applied as a serial execution in batch order
        would, whichever segments they come from; a read that a later write
        of the batch overtakes is answered from a snapshot (a tree with a
        scratch tail).  GET_ACL and the list ops still run after the serve,
        over the tree as all the batch's writes leave it, and the catch-up
        and the close pass keep their place: in-batch order covers the
        serve's class only.  :meth:`order_stats` works after the call.  A
        request whose rank is >= ``passes`` is answered SYSTEMERROR, without
        effect, as in :meth:`serve_sessions`.

        ``defer`` (an :class:`OrderDefer` of ``segs.S`` segments; only with
        ``ordered``): deferral instead of that refusal.  The frame whose rank
        the passes cannot reach and every later frame of its segment, of any
        class, leave the batch before the first pass: they are frames of no
        segment, so nothing of them is parsed, looked up, claimed, armed,
        fired, closed or caught up, and their SYSTEMERROR placeholders lie
        behind ``defer.rep_end[s]`` in the segment's slice.  The caller
        sends ``out[rep_off[s]:rep_end[s]]`` and serves the segment's bytes
        from ``defer.used[s]`` on again in a later batch.  The frames that
        stay are served as if the deferred ones had not been sent.  (A
        deferred SEQUENTIAL create has taken its number, which stays out of
        use: a gap in the parent's cversion, as every refused numbered create
        leaves — the serve's instance for these passes does not hand a
        deferred frame's number back as a batch refused as a whole does, so
        the name it gets in a later batch is past every name of this one.  A
        batch whose table is unsound is refused as a whole and defers
        nothing.)

        Raises ``ValueError`` on a ``fused_rows`` or ``read_only`` server
        and on a sharded tree, as the two entry points do."""
        tree = self.tree
        if self.fused_rows or self.read_only:
            raise ValueError('serve_sessions_mixed: no session form of the '
                             'read-only or the fused-rows serve')
        if tree.shard is not None and tree.shard[1] > 1:
            raise ValueError('serve_sessions_mixed: a sharded tree does not '
                             'index every child of its parents')
        if not isinstance(segs, SessionSegments):
            raise TypeError('serve_sessions_mixed: segs is a SessionSegments')
        if resume and tree.watch is None:
            raise ValueError('serve_sessions_mixed: resume needs a watch '
                             'table')
        if defer is not None:
            if not ordered:
                raise ValueError('serve_sessions_mixed: defer needs ordered')
            if not isinstance(defer, OrderDefer) or defer.S != segs.S:
                raise ValueError('serve_sessions_mixed: defer is an '
                                 'OrderDefer of segs.S segments')
        self._mix_buffers()
        cap = self.cap_frames
        if self.seg is None or self.seg.S != segs.S:
            self.seg = _SegState(cap, segs.S, tree.device)
        sg = self.seg
        seg_c = sg.class_tables()
        if out is None:
            out = self.mix_out
        if max_frame is None:
            max_frame = consts.MAX_PACKET
        ft = self.scanner.scan(rx, n)
        _lib.sess_assign(ft.off, ft.length, ft.count, cap, segs.starts,
                         segs.sessions, sg.f_seg, sg.first, sg.state, sg.bad,
                         **_table_args(table))
        _lib.tree_mix_split(rx, ft.off, ft.length, ft.count, cap,
                            tree.acl is not None, self.mix_cls, self.mix_sub,
                            self.mix_foff, self.mix_flen, self.mix_counts,
                            self.mix_split_ws)
        _lib.sess_split_segments(sg.f_seg, self.mix_cls, self.mix_sub,
                                 ft.count, cap, seg_c)
        fa, fc, fl = self.mix_frames
        # the serve's class, as serve_sessions serves a batch
        clip = None if defer is None else [
            self.mix_cls, self.mix_sub, ft.count, sg.f_seg, *seg_c,
            defer.clipf, defer.deferred]
        a_out, _, a_total, a_err = self._serve_class(
            rx, fa, sg.table(segs, 0), segs, ordered, passes, clip, close,
            self.mix_rec_off[0], False)
        # the two read engines, after the batch's writes
        c_out, l_out = self.mix_scratch
        c_total, c_err = self.acl_total_err
        if tree.acl is not None:
            _lib.tree_acl_get_sessions(
                tree.tensors, tree.acl, rx, fc.off, fc.length, fc.count, cap,
                sg.table(segs, 1), self._acl_workspace(), c_out,
                c_out.numel(), self.acl_rec_off, c_total, c_err, False)
        else:
            c_out = l_out
        l_total, l_err = self.list_total_err
        _lib.tree_list_sessions(
            tree.tensors, rx, fl.off, fl.length, fl.count, cap,
            sg.table(segs, 2), max_frame, self.list_want, self.list_ws, l_out,
            l_out.numel(), self.list_rec_off, l_total, l_err, False)
        total, err = self.mix_total_err
        _lib.tree_mix_merge(
            self.mix_cls, self.mix_sub, ft.count, self.mix_counts, cap,
            [a_out, c_out, l_out],
            [self.mix_rec_off[0], self.acl_rec_off, self.list_rec_off],
            [a_total, c_total, l_total], [a_err, c_err, l_err], out,
            out.numel(), self.mix_rec_off[1], total, err, self.mix_merge_ws,
            terminate)
        rec_off = self.mix_rec_off[1]
        self.last_rec_off = rec_off
        self.result = (out, total, err, ft)
        self._sessions_tail(rx, ft, segs, rec_off, total, err, table, resume,
                            close, defer)
        return self.result

    def acl_stats(self):
        """(entries, arena bytes used, lost) of the tree's ACL table: the
        distinct ACLs stored (the open one included), the bytes they take
        (the whole arena once a vector did not fit: the arena is a bump
        allocator), and the created nodes whose ACL found no room (they
        answer GET_ACL with SYSTEMERROR).  One host read."""
        acl = self.tree.acl
        if acl is None:
            raise ValueError('acl_stats: the tree keeps no ACL table')
        c = acl[4].cpu().tolist()
        return (c[_lib.AC_ENT], min(c[_lib.AC_TOP], acl[1].numel()),
                c[_lib.AC_LOST])

    def _seq_order(self, rx, ft):
        """Number the batch's SEQUENTIAL creates in stream order (parent's
        cversion before the batch + rank among its sequential creates
        here): returns the int64 [cap_frames] words for the serve (parent
        node << 32 | number; -1 none)."""
        L = _lib.lib()
        dev = self.tree.device
        if self.seq_ws is None:
            n = self.cap_frames
            self.seq_ws = torch.empty(L.tree_seq_workspace(n), dtype=U8,
                                      device=dev)
            self.seq_ws[:L.tree_seq_zeroed(n)].zero_()
            self.seqno = torch.empty(n, dtype=I64, device=dev)
        L.tree_seq_order(self.tree.tensors, rx, ft.off, ft.length, ft.count,
                         self.cap_frames, self.seq_ws, self.seqno)
        return self.seqno

    def order_counters(self):
        """The device words :meth:`order_stats` reads — int64 [2]: the
        largest rank, the scratch bytes asked for (more than the scratch
        tail holds: a snapshot found no room) — for a caller that folds them
        into a read of its own (the front end's report); no host read."""
        if self.ows is None:
            raise ValueError('order_counters: no ordered serve has run')
        o = _lib.lib().tree_order_stats_offset(self.cap_frames)
        return self.ows[o:o + 16].view(torch.int64)

    def order_stats(self):
        """(largest same-path rank, scratch bytes used) of the last ordered
        serve (host read).  A rank >= the passes used means refusals."""
        o = _lib.lib().tree_order_stats_offset(self.cap_frames)
        v = self.ows[o:o + 16].cpu().view(torch.int64).tolist()
        return v[0], v[1]


class GetPipeline(object):
    """Batched get() over the synthetic tree (BASELINE config 2)."""

    # client encode | server decode | tree + encode | client decode
    PHASES = 4

    def __init__(self, tree, batch, seed=0, streams=1, stagger=False,
                 priority=False):
        self.tree = tree
        self.batch = batch
        dev = tree.device
        self.dev = dev
        self.subs = []
        if streams > 1:
            # `streams` independent pipelined connections, each with its own
            # HIP stream, buffers and xid table, sharing the (read-only)
            # tree.  Their phases are issued round-robin (see step), so one
            # connection's latency-bound kernels (frame-scan walks, scans)
            # overlap another's bandwidth-bound ones.  `stagger`: connection
            # k runs k * PHASES / streams phases behind connection 0 (the
            # steady state of pipelined connections), so the frame scans of
            # one meet the encoders and tree of another instead of their own
            # copies; a step still issues PHASES phases of every connection,
            # and a connection's reply check lands in the step() call that
            # runs its last phase.
            per = [batch // streams + (1 if k < batch % streams else 0)
                   for k in range(streams)]
            self.subs = [GetPipeline(tree, m, seed=seed * streams + k)
                         for k, m in enumerate(per)]
            # priority: connection 0's stream is a high-priority one (its
            # small kernels take the next free slots, the others fill in)
            self.streams = [torch.cuda.Stream(
                dev, priority=-1 if priority and k == 0 else 0)
                for k in range(len(per))]
            self.stagger = stagger
            self._gens = None
            self.last = None
            return
        self.xt = B.XidTable(bits=max(20, (batch - 1).bit_length() + 1),
                             device=dev)
        n = batch
        # request descriptors (reused every step)
        self.opcode = torch.full((n,), consts.OP_CODES['GET_DATA'],
                                 dtype=I32, device=dev)
        self.arg = torch.zeros(n, dtype=I32, device=dev)
        self.zero64 = torch.zeros(n, dtype=I64, device=dev)
        self.zero32 = torch.zeros(n, dtype=I32, device=dev)
        self.acl_off = torch.zeros(1, dtype=I64, device=dev)
        self.acl_len = torch.zeros(1, dtype=I32, device=dev)
        self.acl_arena = torch.zeros(16, dtype=U8, device=dev)
        maxpath = int(tree.node_path_len.max().item())
        self.tx = torch.empty(n * (17 + maxpath) + 64, dtype=U8, device=dev)
        dmax = max(tree.data_bytes, 128)
        # K1 windows: the largest request / reply frame of this workload
        self.server = GpuServer(tree, n, n * (4 + 16 + 4 + dmax + 68) + 64,
                                window=B.frame_window(17 + maxpath),
                                seq_order=False, group=_GET_SRV_GROUP,
                                # (a tree with an ACL table keeps the whole
                                # step on the plain path, reply side too)
                                fused_rows=tree.acl is None)
        self.server.read_only = True
        self.rwindow = B.frame_window(4 + 16 + 4 + dmax + 68)
        lo, hi = tree.data_dist or (tree.data_bytes, tree.data_bytes)
        self.rscanner = B.FrameScanner(n, dev, window=self.rwindow,
                                       frame_hint=4 + 16 + 4 + 68 +
                                       (lo + hi) // 2)
        self.reply = B.alloc_replies(n, dev)
        self.xid_base = 0
        self.last = None
        self.seed = seed
        self.step_no = 0
        self.idx = torch.empty(n, dtype=I64, device=dev)
        self.xid = torch.empty(n, dtype=I32, device=dev)
        self.poff = torch.empty(n, dtype=I64, device=dev)
        self.plen = torch.empty(n, dtype=I32, device=dev)
        # the encode's sizes pass, written by the generator
        self.sizes = torch.empty(n, dtype=I64, device=dev)
        self.bsum = torch.empty((n + 255) // 256, dtype=I64, device=dev)
        self.gstate = None      # device {seed, step} (see capture)

    def _device_seed(self):
        """Draw each step's requests from a device-resident {seed, step}
        pair advanced on the device, so a captured graph replays NEW
        batches (a host seed would be frozen into the graph)."""
        for p in self.subs or [self]:
            if p.gstate is None:
                p.gstate = torch.tensor([p.seed, p.step_no], dtype=I64,
                                        device=self.dev)

    def capture(self, acc):
        """Capture one step (validated into ``acc``, which every replay adds
        to) as a HIP graph: a step's ~50 launches over two streams replay
        with one host call.  Run at least one eager step first (buffers
        are sized then).  Returns the graph; ``graph.replay()`` is a step.
        """
        self._device_seed()
        torch.cuda.synchronize(self.dev)
        g = torch.cuda.CUDAGraph()
        # thread-local: another thread's HIP calls (a process group's
        # watchdog) do not invalidate this capture
        with torch.cuda.graph(g, capture_error_mode='thread_local'):
            self.step(acc=acc)
        self.graph = g
        return g

    def step(self, validate=True, acc=None):
        """One batch.  With ``validate`` the number of correct replies is
        added to ``acc`` (device int64 [1]; a fresh one when None), which is
        returned.  Request generation and the reply check are one fused
        kernel each (csrc/kernels/bench.hip)."""
        if validate and acc is None:
            acc = torch.zeros(1, dtype=I64, device=self.dev)
        if not self.subs:
            for _ in self._phases(validate, acc):
                pass
            return acc if validate else None
        cur = torch.cuda.current_stream(self.dev)
        if self.stagger:
            for s in self.streams:
                s.wait_stream(cur)
            self._validate, self._acc = validate, acc
            if self._gens is None:
                ns = len(self.subs)
                self._gens = [p._forever(self, k * self.PHASES // ns)
                              for k, p in enumerate(self.subs)]
            for _ in range(self.PHASES):
                for s, g in zip(self.streams, self._gens):
                    with torch.cuda.stream(s):
                        next(g)
            for s in self.streams:
                cur.wait_stream(s)
            return acc if validate else None
        live = []
        for p, s in zip(self.subs, self.streams):
            s.wait_stream(cur)
            live.append((s, p._phases(validate, acc)))
        while live:
            nxt = []
            for s, g in live:
                with torch.cuda.stream(s):
                    if next(g, StopIteration) is not StopIteration:
                        nxt.append((s, g))
            live = nxt
        for s in self.streams:
            cur.wait_stream(s)
        return acc if validate else None

    def _forever(self, parent, lag):
        """Phases of step after step, one per next(), starting ``lag`` idle
        phases late; the validation flag and counter are the parent's at
        the time of the check."""
        for _ in range(lag):
            yield
        while True:
            for _ in self._phases(None, None, parent):
                yield           # after each of the first PHASES - 1 phases
            yield               # after the last

    def _phases(self, validate, acc, parent=None):
        """The step as a generator on the caller's current stream, yielding
        between its PHASES phases (client encode, server frame scan and
        decode, tree and reply encode, client decode and check); a
        multi-stream step interleaves the connections' phases."""
        t = self.tree
        n = self.batch
        L = _lib.lib()
        seed = (self.seed * 0x9E3779B97F4A7C15 + self.step_no) & (2**64 - 1)
        self.step_no += 1
        L.bench_gen_get(n, _i64(seed), t.leaf0, t.n_leaves, self.xid_base,
                        t.node_pw, self.idx, self.xid, self.poff, self.plen,
                        self.gstate, self.sizes, self.bsum)
        xid = self.xid
        self.xid_base = (self.xid_base + n) & 0x7fffffff
        rb = B.RequestBatch(n, self.opcode, xid, self.arg, self.poff,
                            self.plen, self.zero64, self.zero32, self.zero32,
                            t.path_arena, t.slab, self.acl_off,
                            self.acl_len, self.acl_arena)
        tx, rec_off, total, err = B.encode_requests(
            rb, self.xt, out=self.tx,
            presized=(self.sizes, self.bsum))
        yield
        srv = self.server.serve_steps(tx, _len(total))
        next(srv)
        yield
        for _ in srv:
            pass
        rx, rtotal, rerr, _ = self.server.result
        yield
        # K1 without its rows pass on both streams: the serve and the decode
        # read the scans' tile lists (11 launches a connection, not 13)
        ft = self.rscanner.scan(rx, _len(rtotal),
                                rows=not self.server.fused_rows)
        if parent is not None:
            validate, acc = parent._validate, parent._acc
        # the reply check rides in the decode kernel (acc: 1..64 slots)
        chk = (self.idx, xid, t.data_len, acc, t.slab_all,
               t.slot_off) if validate else None
        # the device step counter advances in the checking decode (one
        # launch less per step), else on its own
        rep = B.decode_replies(rx, ft, self.xt, out=self.reply, check=chk,
                               tick=self.gstate if validate else None,
                               tiles=self.rscanner.pending)
        if self.gstate is not None and not validate:
            self.gstate[1:].add_(1)
        self.last = (self.idx, rep, rx, ft)


class ListPipeline(object):
    """Batched list() over the synthetic tree's directories: a fixed
    K10-encoded batch of ``batch`` GET_CHILDREN2 requests, request ``k`` on
    directory ``k % ndirs`` (``ndirs`` below the batch size: several
    requests per directory, the duplicate path of the list kernels).

    A step is :meth:`GpuServer.serve_list` on the request stream, then the
    client half on the replies: K1, K2-K8 decode, and the children vectors
    expanded to one (offset, length) row per name.  The device check adds to
    ``bad`` every reply that is not a clean OK, whose child count differs
    from its Stat's numChildren, and a step whose string bytes differ from
    the tree's (counted on the host when the pipeline is built); a good
    step adds ``batch`` to ``acc``.  No host read inside a step."""

    def __init__(self, tree, batch, ndirs=None):
        self.tree = tree
        self.batch = n = batch
        self.dev = dev = tree.device
        L = _lib.lib()
        all_dirs = tree.leaf0 - 1
        ndirs = all_dirs if ndirs is None else min(int(ndirs), all_dirs)
        self.ndirs = ndirs
        didx = 1 + (np.arange(n, dtype=np.int64) % ndirs)
        # each directory's children and name bytes, from the node table
        nn = min(int(tree.counters[_lib.TC_NODES].item()), tree.cap)
        par = tree.node_parent[:nn].cpu().numpy()
        ln = (tree.node_pw[:nn].cpu().numpy() & 0xFFFFFF)
        kid = par >= 0
        cnt = np.bincount(par[kid], minlength=nn)
        nbytes = np.bincount(par[kid], weights=(ln[kid] - ln[par[kid]] + 3),
                             minlength=nn).astype(np.int64)
        self.want_children = int(cnt[didx].sum())
        self.want_bytes = int(nbytes[didx].sum())
        frame = 4 + 16 + 4 + nbytes[didx] + 68
        out_cap = int(frame.sum()) + 64
        idx = torch.from_numpy(didx).to(dev)
        self.xt = B.XidTable(bits=max(20, (n - 1).bit_length() + 1),
                             device=dev)
        z64 = torch.zeros(n, dtype=I64, device=dev)
        z32 = torch.zeros(n, dtype=I32, device=dev)
        rb = B.RequestBatch(
            n, torch.full((n,), consts.OP_CODES['GET_CHILDREN2'], dtype=I32,
                          device=dev),
            torch.arange(n, dtype=I32, device=dev), z32,
            tree.node_path_off[idx].contiguous(),
            tree.node_path_len[idx].contiguous(), z64, z32, z32,
            tree.path_arena, tree.slab, torch.zeros(1, dtype=I64, device=dev),
            torch.zeros(1, dtype=I32, device=dev),
            torch.zeros(16, dtype=U8, device=dev))
        maxpath = int(tree.node_path_len[idx].max().item())
        tx = torch.empty(n * (17 + maxpath) + 64, dtype=U8, device=dev)
        self.tx, _, self.tx_total, _ = B.encode_requests(rb, self.xt, out=tx)
        self.server = GpuServer(tree, n, out_cap,
                                window=B.frame_window(17 + maxpath),
                                seq_order=False)
        self.rscanner = B.FrameScanner(
            n, dev, window=B.frame_window(int(frame.max())))
        self.reply = B.alloc_replies(n, dev)
        self.reply.aux0.zero_()
        # one row per child name; the names sit in the reply buffer, 4 bytes
        # of length each at least, so this bounds them whatever the replies
        self.str_cap = out_cap // 4 + 1
        self.soff = torch.empty(self.str_cap, dtype=I64, device=dev)
        self.slen = torch.empty(self.str_cap, dtype=I32, device=dev)
        self.row_base = torch.empty(n, dtype=I64, device=dev)
        self.nstr = torch.zeros(1, dtype=I64, device=dev)
        self.scan_ws = torch.empty(L.scan_workspace(n), dtype=I64, device=dev)
        self.bad = torch.zeros(1, dtype=I64, device=dev)
        self.last = None

    def capture(self, acc):
        """One step as a HIP graph (run an eager step first)."""
        return _capture_steps(self, acc)

    def server_step(self):
        """The server half alone: K1 on the requests and the list kernels."""
        return self.server.serve_list(self.tx, self.tx_total)

    def step(self, validate=True, acc=None):
        if validate and acc is None:
            acc = torch.zeros(1, dtype=I64, device=self.dev)
        L = _lib.lib()
        n = self.batch
        rx, rtotal, rerr, _ = self.server_step()
        ft = self.rscanner.scan(rx, _len(rtotal))
        rep = self.reply
        # (rows past the frames K1 found keep a zero count: nothing of a
        # short stream is expanded)
        rep.aux0.zero_()
        B.decode_replies(rx, ft, self.xt, out=rep)
        L.scan_excl(rep.aux0, self.row_base, self.nstr, self.scan_ws)
        L.expand_strings(rx, rep.pay_off, rep.aux0, self.row_base, self.soff,
                         self.slen)
        self.last = (rep, rx, ft, rtotal)
        if not validate:
            return None
        bad = ((rep.err != 0) | (rep.status != 0) |
               (rep.aux0 != rep.stat32[4])).sum()
        bad = bad + (ft.count[0] != n).to(I64) + (rerr[0] != 0).to(I64)
        bad = bad + (rep.pay_len.sum() != self.want_bytes).to(I64)
        bad = bad + (self.nstr[0] != self.want_children).to(I64)
        self.bad.add_(bad)
        acc.add_(n * (bad == 0).to(I64))
        return acc

    def diagnose(self):
        """Host view of the last step's replies (after a failed check)."""
        rep, rx, ft, rtotal = self.last
        return {'frames': ft.host_result(), 'total': int(rtotal.item()),
                'err': rep.err.unique().cpu().tolist(),
                'children': int(rep.aux0.sum().item()),
                'want_children': self.want_children,
                'string_bytes': int(rep.pay_len.sum().item()),
                'want_bytes': self.want_bytes, 'bad': int(self.bad.item())}


class AclPipeline(object):
    """Batched getACL() over the synthetic tree: ``batch`` GET_ACL requests
    on live leaves drawn at random (with ``seed``) when the pipeline is
    built; the tree needs an ACL table (``GpuTree(acl_cap=...)``).

    A step is the K10 encode of the requests, :meth:`GpuServer.serve_acl`,
    then the client half on the replies: K1, K2-K8 decode, and the ACL
    vectors expanded to one (perms, scheme, id) row per entry.  The device
    check adds to ``bad`` every reply that is not a clean OK, whose entry
    count or whose first entry's perms differ from the node's ACL in the
    table (read back to the host when the pipeline is built); a good step
    adds ``batch`` to ``acc``.  No host read inside a step."""

    def __init__(self, tree, batch, seed=0):
        if tree.acl is None:
            raise ValueError('AclPipeline: the tree keeps no ACL table')
        self.tree = tree
        self.batch = n = batch
        self.dev = dev = tree.device
        L = _lib.lib()
        nn = min(int(tree.counters[_lib.TC_NODES].item()), tree.cap)
        par = tree.node_parent[:nn].cpu().numpy()
        live = np.nonzero(par[tree.leaf0:] != NODE_FREE)[0] + tree.leaf0
        rng = np.random.default_rng(seed + 29)
        nidx = live[rng.integers(0, len(live), n)]
        # what each reply must carry: its node's vector in the table
        words = tree.acl[0][:nn].cpu().numpy()[nidx]
        arena = tree.acl[1].cpu().numpy().tobytes()
        cnt = np.zeros(n, np.int32)
        p0 = np.zeros(n, np.int32)
        nbytes = np.zeros(n, np.int64)
        for wd in np.unique(words):
            if wd == _lib.ACL_LOST:
                raise ValueError('AclPipeline: a node with a lost ACL')
            off, ln = int(wd) >> 24, int(wd) & 0xFFFFFF
            m = words == wd
            cnt[m] = int.from_bytes(arena[off:off + 4], 'big')
            p0[m] = int.from_bytes(arena[off + 4:off + 8], 'big')
            nbytes[m] = ln
        self.want_cnt = torch.from_numpy(cnt).to(dev)
        self.want_p0 = torch.from_numpy(p0).to(dev)
        self.want_entries = int(cnt.sum())
        frame = 4 + 16 + nbytes + 68
        out_cap = int(frame.sum()) + 64
        idx = torch.from_numpy(nidx).to(dev)
        self.idx = idx
        self.xt = B.XidTable(bits=max(20, (n - 1).bit_length() + 1),
                             device=dev)
        z64 = torch.zeros(n, dtype=I64, device=dev)
        z32 = torch.zeros(n, dtype=I32, device=dev)
        self.rb = B.RequestBatch(
            n, torch.full((n,), consts.OP_CODES['GET_ACL'], dtype=I32,
                          device=dev),
            torch.arange(n, dtype=I32, device=dev), z32,
            tree.node_path_off[idx].contiguous(),
            tree.node_path_len[idx].contiguous(), z64, z32, z32,
            tree.path_arena, tree.slab, torch.zeros(1, dtype=I64, device=dev),
            torch.zeros(1, dtype=I32, device=dev),
            torch.zeros(16, dtype=U8, device=dev))
        maxpath = int(tree.node_path_len[idx].max().item())
        self.tx = torch.empty(n * (16 + maxpath) + 64, dtype=U8, device=dev)
        self.server = GpuServer(tree, n, out_cap,
                                window=B.frame_window(16 + maxpath),
                                seq_order=False)
        self.rscanner = B.FrameScanner(
            n, dev, window=B.frame_window(int(frame.max())))
        self.reply = B.alloc_replies(n, dev)
        self.reply.aux0.zero_()
        # one row per ACL entry; an entry is 12 bytes of the reply stream at
        # least, so this bounds them whatever the replies
        self.row_cap = out_cap // 12 + 1
        self.perms = torch.zeros(self.row_cap, dtype=I32, device=dev)
        self.soff = torch.empty(self.row_cap, dtype=I64, device=dev)
        self.slen = torch.empty(self.row_cap, dtype=I32, device=dev)
        self.ioff = torch.empty(self.row_cap, dtype=I64, device=dev)
        self.ilen = torch.empty(self.row_cap, dtype=I32, device=dev)
        self.row_base = torch.zeros(n, dtype=I64, device=dev)
        self.nrows = torch.zeros(1, dtype=I64, device=dev)
        self.scan_ws = torch.empty(L.scan_workspace(n), dtype=I64, device=dev)
        self.bad = torch.zeros(1, dtype=I64, device=dev)
        self.last = None

    def capture(self, acc):
        """One step as a HIP graph (run an eager step first)."""
        return _capture_steps(self, acc)

    def encode(self):
        """The client's request stream (K10): ``(tx, device total)``."""
        tx, _, total, _ = B.encode_requests(self.rb, self.xt, out=self.tx)
        return tx, total

    def server_step(self, tx, total):
        """The server half alone: K1 on the requests and the ACL kernels."""
        return self.server.serve_acl(tx, _len(total))

    def step(self, validate=True, acc=None):
        if validate and acc is None:
            acc = torch.zeros(1, dtype=I64, device=self.dev)
        L = _lib.lib()
        n = self.batch
        tx, total = self.encode()
        rx, rtotal, rerr, _ = self.server_step(tx, total)
        ft = self.rscanner.scan(rx, _len(rtotal))
        rep = self.reply
        # (rows past the frames K1 found keep a zero count: nothing of a
        # short stream is expanded)
        rep.aux0.zero_()
        B.decode_replies(rx, ft, self.xt, out=rep)
        L.scan_excl(rep.aux0, self.row_base, self.nrows, self.scan_ws)
        L.expand_acl(rx, rep.pay_off, rep.aux0, self.row_base, self.perms,
                     self.soff, self.slen, self.ioff, self.ilen)
        self.last = (rep, rx, ft, rtotal)
        if not validate:
            return None
        first = self.perms[self.row_base.clamp(0, self.row_cap - 1)]
        bad = ((rep.err != 0) | (rep.status != 0) |
               (rep.aux0 != self.want_cnt) | (first != self.want_p0)).sum()
        bad = bad + (ft.count[0] != n).to(I64) + (rerr[0] != 0).to(I64)
        bad = bad + (self.nrows[0] != self.want_entries).to(I64)
        self.bad.add_(bad)
        acc.add_(n * (bad == 0).to(I64))
        return acc

    def diagnose(self):
        """Host view of the last step's replies (after a failed check)."""
        rep, rx, ft, rtotal = self.last
        return {'frames': ft.host_result(), 'total': int(rtotal.item()),
                'err': rep.err.unique().cpu().tolist(),
                'entries': int(rep.aux0.sum().item()),
                'want_entries': self.want_entries,
                'bad': int(self.bad.item())}


def _arena(strings, dev):
    """Pack host strings into (arena u8, off i64, len i32) device tensors."""
    enc = [x.encode() for x in strings]
    ln = np.fromiter((len(e) for e in enc), np.int32, len(enc))
    off = np.zeros(len(enc), np.int64)
    if len(enc) > 1:
        np.cumsum(ln[:-1], out=off[1:])
    blob = b''.join(enc) or b'\0'
    arena = torch.frombuffer(bytearray(blob), dtype=U8).to(dev)
    return arena, torch.from_numpy(off).to(dev), torch.from_numpy(ln).to(dev)


def _acl_table(acls, dev):
    blobs = [B._acl_bytes(a) for a in acls]
    raw = b''.join(blobs)
    lens = np.array([len(b) for b in blobs], np.int32)
    offs = np.zeros(len(blobs), np.int64)
    np.cumsum(lens[:-1], out=offs[1:])
    arena = torch.frombuffer(bytearray(raw), dtype=U8).to(dev)
    return (arena, torch.from_numpy(offs).to(dev),
            torch.from_numpy(lens).to(dev))


# ACLs the mix alternates between (K10 encodes them from the pre-encoded
# vectors; the server rejects an empty one with INVALID_ACL)
MIX_ACLS = (
    [{'perms': consts.PERM_ALL, 'id': {'scheme': 'world', 'id': 'anyone'}}],
    [{'perms': ['READ'], 'id': {'scheme': 'world', 'id': 'anyone'}},
     {'perms': consts.PERM_ALL, 'id': {'scheme': 'digest',
                               'id': 'bench:kQq8nOxk1NC8y2GdzFjp0v4ZbVY='}}],
)


class _GraphCycle(object):
    """HIP graphs replayed in turn (a workload whose steps rotate through a
    few shapes: one captured graph per shape).  ``counter``: the name of the
    pipeline's host step counter; capturing advanced it without running a
    step, so it is put back and then advanced by each replay — an eager step
    after replays continues where they left the device state."""

    def __init__(self, graphs, pipe=None, counter=None):
        self.graphs = graphs
        self.i = 0
        self.pipe = pipe
        self.counter = counter

    def replay(self):
        self.graphs[self.i].replay()
        self.i = (self.i + 1) % len(self.graphs)
        if self.counter:
            setattr(self.pipe, self.counter,
                    getattr(self.pipe, self.counter) + 1)


def _capture_steps(pipe, acc, k=1, counter=None):
    """Capture ``k`` consecutive steps of ``pipe`` as HIP graphs (run one
    eager step first: buffers are sized then).  A replay is a step."""
    dev = pipe.tree.device
    torch.cuda.synchronize(dev)
    s0 = getattr(pipe, counter) if counter else None
    graphs = []
    for _ in range(k):
        g = torch.cuda.CUDAGraph()
        # thread-local: another thread's HIP calls do not invalidate it
        with torch.cuda.graph(g, capture_error_mode='thread_local'):
            pipe.step(acc=acc)
        graphs.append(g)
    if counter:
        setattr(pipe, counter, s0)
    if k == 1 and not counter:
        return graphs[0]
    return _GraphCycle(graphs, pipe, counter)


class _Driver(object):
    """Client half shared by the write pipelines: K10 encode of a request
    batch (xids recorded in the HBM xid table), the GPU server, then K1 +
    K2-K8 decode of the reply stream."""

    def __init__(self, tree, batch, max_path, data_bytes, seed,
                 seq_order=False, group=_SRV_GROUP):
        self.tree = tree
        self.batch = batch
        self.dev = dev = tree.device
        self.xt = B.XidTable(bits=max(20, (batch - 1).bit_length() + 1),
                             device=dev)
        self.tx = torch.empty(batch * (33 + max_path + data_bytes + 128) + 64,
                              dtype=U8, device=dev)
        dmax = max(tree.data_bytes, 128, data_bytes)
        # K1 windows from the largest frames (CREATE with data and a
        # two-entry ACL; a GET_DATA-sized reply)
        self.server = GpuServer(
            tree, batch, batch * (4 + 16 + 4 + max(dmax, max_path + 16) + 68)
            + 64, window=B.frame_window(33 + max_path + data_bytes + 128),
            seq_order=seq_order, group=group)
        self.rwindow = B.frame_window(4 + 16 + 4 + max(dmax, max_path + 16)
                                      + 68)
        self.reply = B.alloc_replies(batch, dev)
        self.rscanner = None
        # the session's next xid, on the device: a captured step replays
        # with new xids
        self.xid_dev = torch.zeros(1, dtype=I64, device=dev)
        self.iota = torch.arange(batch, dtype=I64, device=dev)
        self.passes = 0          # > 0: ordered serving in that many passes

    def xids(self, n):
        x = torch.empty(n, dtype=I32, device=self.dev)
        _lib.lib().bench_xids(n, self.xid_dev, x)     # (one fused launch)
        self.xid_dev.add_(n)
        return x

    def create_dirs(self, levels, acl):
        """CREATE persistent directories, one batch per level (a parent must
        exist before its children's batch runs).  ``acl`` = (arena, off,
        len) pre-encoded ACL table."""
        dev = self.dev
        aarena, aoff, alen = acl
        for level in levels:
            n = len(level)
            arena, off, ln = _arena(level, dev)
            z32 = torch.zeros(n, dtype=I32, device=dev)
            rb = B.RequestBatch(
                n, torch.full((n,), consts.OP_CODES['CREATE'], dtype=I32,
                              device=dev),
                self.xids(n), z32, off, ln,
                torch.zeros(n, dtype=I64, device=dev), z32, z32, arena,
                arena, aoff, alen, aarena)
            rep, _ = self.run(rb)
            errs = rep.err[:n]
            if not bool(((errs == 0) |
                         (errs == consts.ERR_CODES['NODE_EXISTS'])).all()):
                raise RuntimeError('directory create failed: %r' % (
                    errs.unique().cpu().tolist(),))

    def run(self, rb, session=0):
        """One batch through encode -> server -> decode.  Both streams are
        scanned over their encoders' device totals: no device-to-host read."""
        tx, _, total, _ = B.encode_requests(rb, self.xt, out=self.tx)
        rx, rtotal, _, _ = self.server.serve(tx, _len(total),
                                             session=session,
                                             ordered=self.passes > 0,
                                             passes=max(self.passes, 1))
        if self.rscanner is None:
            self.rscanner = B.FrameScanner(self.batch, self.dev,
                                           window=self.rwindow)
        ft = self.rscanner.scan(rx, _len(rtotal))
        rep = B.decode_replies(rx, ft, self.xt, out=self.reply)
        return rep, rx


class MixPipeline(object):
    """create / set(version CAS) / delete mix with ACL encode (BASELINE
    config 3) over the synthetic tree.

    Every step issues ``m = batch // 3`` of each op on three rotating
    generations of ``m`` nodes ``/mix/dDDDD/gG_KKKKKKKKK``: step ``s``
    CREATEs generation ``s % 3`` (alternating two ACL vectors), SET_DATAs
    generation ``s-1`` with expected version 0 (every 16th with a stale
    version, which must fail with BAD_VERSION) and DELETEs generation ``s-2``
    with its exact current version.  Node slots, paths and hash entries are
    recycled through the tree's free ring, so the tree size is steady.
    Every reply is checked on the device against its expected error code,
    xid and opcode (and version 1 for successful sets)."""

    def __init__(self, tree, batch, data_bytes=100, ndirs=1024, seed=0):
        m = max(batch // 3, 1)
        self.m = m
        self.n = 3 * m
        dev = tree.device
        self.tree = tree
        self.ndirs = ndirs
        paths = ['/mix/d%05d/g%d_%09d' % (k % ndirs, g, k)
                 for g in range(3) for k in range(m)]
        maxp = max(len(p) for p in paths)
        self.drv = _Driver(tree, self.n, maxp, data_bytes, seed)
        self.path_arena, poff, plen = _arena(paths, dev)
        g = torch.Generator(device=dev)
        g.manual_seed(seed + 7)
        nblk = 1024
        self.data_arena = torch.randint(0, 256, (nblk * data_bytes + 16,),
                                        dtype=U8, device=dev, generator=g)
        self.acl_arena, self.acl_off, self.acl_len = _acl_table(MIX_ACLS, dev)
        k = torch.arange(m, dtype=I64, device=dev)
        stale = (k % 16) == 15
        ops = consts.OP_CODES
        self.opcode = torch.cat([
            torch.full((m,), ops['CREATE'], dtype=I32, device=dev),
            torch.full((m,), ops['SET_DATA'], dtype=I32, device=dev),
            torch.full((m,), ops['DELETE'], dtype=I32, device=dev)])
        self.arg = torch.cat([torch.zeros(m, dtype=I64, device=dev),
                              torch.where(stale, 7, 0),
                              torch.where(stale, 0, 1)]).to(I32)
        self.data_off = torch.cat([(k % nblk) * data_bytes,
                                   ((k + 7) % nblk) * data_bytes,
                                   torch.zeros(m, dtype=I64, device=dev)])
        self.data_len = torch.cat([
            torch.full((2 * m,), data_bytes, dtype=I32, device=dev),
            torch.zeros(m, dtype=I32, device=dev)])
        self.acl_id = torch.cat([(k % 2).to(I32),
                                 torch.zeros(2 * m, dtype=I32, device=dev)])
        bad = consts.ERR_CODES['BAD_VERSION']
        self.want_err = torch.cat([
            torch.zeros(m, dtype=I32, device=dev),
            torch.where(stale, bad, 0).to(I32),
            torch.zeros(m, dtype=I32, device=dev)])
        self.is_set_ok = torch.cat([
            torch.zeros(m, dtype=torch.bool, device=dev), ~stale,
            torch.zeros(m, dtype=torch.bool, device=dev)])
        # path offsets per rotation r = s % 3: (create, set, delete) gens
        po = poff.view(3, m)
        self.path_off = [torch.cat([po[r], po[(r - 1) % 3], po[(r - 2) % 3]])
                         for r in range(3)]
        self.path_len = plen[:m].repeat(3)
        self.s = -2
        self.drv.create_dirs(
            [['/mix'], ['/mix/d%05d' % d for d in range(ndirs)]],
            (self.acl_arena, self.acl_off, self.acl_len))
        # prime: s = -2 creates generation 1, s = -1 creates 2 and sets 1
        self.step(validate=False, n=m)
        self.step(validate=False, n=2 * m)

    def capture(self, acc):
        """Three HIP graphs, one per rotation of the generations (step s
        creates s % 3, sets s - 1, deletes s - 2), replayed in turn."""
        return _capture_steps(self, acc, 3, counter='s')

    def _batch(self, n, r):
        d = self.drv
        return B.RequestBatch(n, self.opcode[:n], d.xids(n), self.arg[:n],
                              self.path_off[r][:n], self.path_len[:n],
                              self.data_off[:n], self.data_len[:n],
                              self.acl_id[:n], self.path_arena,
                              self.data_arena, self.acl_off, self.acl_len,
                              self.acl_arena)

    def step(self, validate=True, n=None, acc=None):
        n = self.n if n is None else n
        rb = self._batch(n, self.s % 3)
        rep, _ = self.drv.run(rb)
        self.last = (rb, rep)
        self.s += 1
        if not validate:
            return None
        ok = ((rep.status[:n] == 0) & (rep.err[:n] == self.want_err[:n]) &
              (rep.xid[:n] == rb.xid) & (rep.opcode[:n] == rb.opcode) &
              (~self.is_set_ok[:n] | (rep.stat32[0, :n] == 1)))
        if acc is None:
            return ok.sum()
        acc[:1] += ok.sum()
        return acc

    def diagnose(self):
        rb, rep = self.last
        n = rb.n
        bad = rep.err[:n] != self.want_err[:n]
        e, c = torch.unique(rep.err[:n][bad], return_counts=True)
        return {'wrong_err': dict(zip(e.cpu().tolist(), c.cpu().tolist())),
                'status_bad': int((rep.status[:n] != 0).sum().item()),
                'counters': self.tree.counters.cpu().tolist()}


class ChainPipeline(object):
    """In-batch ordering workload: every step sends, for each of ``m`` paths
    ``/chain/dDDDD/cKKKKKKKKK``, the chain CREATE (``data_bytes // 2``
    bytes) -> SET_DATA (version 0, ``data_bytes``) -> GET_DATA -> DELETE
    (version 1) back to back in one batch, as one session pipelining them
    would.  The server must apply each chain in order (ordered serving, 4
    passes): every reply is checked on the device — all OK, the set and the
    get see version 1, and the get returns the set's data length.  Nodes
    are recycled through the free ring (each step deletes what it created).
    """

    def __init__(self, tree, batch, data_bytes=100, ndirs=1024, seed=0):
        m = max(batch // 4, 1)
        self.m = m
        self.n = n = 4 * m
        dev = tree.device
        self.tree = tree
        self.data_bytes = data_bytes
        need = 2 * m * (80 + ((data_bytes + 15) & ~15))
        if tree.scratch is None or tree.scratch.numel() < need:
            raise ValueError('ChainPipeline needs GpuTree(scratch >= %d)'
                             % need)
        paths = ['/chain/d%05d/c%09d' % (k % ndirs, k) for k in range(m)]
        maxp = max(len(p) for p in paths)
        self.drv = _Driver(tree, n, maxp, data_bytes, seed)
        self.drv.passes = 4
        self.path_arena, poff, plen = _arena(paths, dev)
        g = torch.Generator(device=dev)
        g.manual_seed(seed + 11)
        nblk = 1024
        self.data_arena = torch.randint(0, 256, (nblk * data_bytes + 16,),
                                        dtype=U8, device=dev, generator=g)
        self.acl_arena, self.acl_off, self.acl_len = _acl_table(MIX_ACLS, dev)
        ops = consts.OP_CODES

        def il(a, b, c, d):      # interleave per path: [a0 b0 c0 d0 a1 ...]
            return torch.stack([a, b, c, d], 1).reshape(-1)
        k = torch.arange(m, dtype=I64, device=dev)
        full = lambda v, dt: torch.full((m,), v, dtype=dt, device=dev)  # noqa
        self.opcode = il(full(ops['CREATE'], I32), full(ops['SET_DATA'], I32),
                         full(ops['GET_DATA'], I32), full(ops['DELETE'], I32))
        self.arg = il(full(0, I32), full(0, I32), full(0, I32), full(1, I32))
        self.path_off = il(poff, poff, poff, poff)
        self.path_len = il(plen, plen, plen, plen)
        self.data_off = il((k % nblk) * data_bytes,
                           ((k + 7) % nblk) * data_bytes, full(0, I64),
                           full(0, I64))
        self.data_len = il(full(data_bytes // 2, I32), full(data_bytes, I32),
                           full(0, I32), full(0, I32))
        self.acl_id = il((k % 2).to(I32), full(0, I32), full(0, I32),
                         full(0, I32))
        self.is_set = self.opcode == ops['SET_DATA']
        self.is_get = self.opcode == ops['GET_DATA']
        self.drv.create_dirs(
            [['/chain'], ['/chain/d%05d' % d for d in range(ndirs)]],
            (self.acl_arena, self.acl_off, self.acl_len))
        self.last = None

    def capture(self, acc):
        """One step as a HIP graph (every step has the same shape)."""
        return _capture_steps(self, acc)

    def step(self, validate=True, acc=None):
        n = self.n
        d = self.drv
        rb = B.RequestBatch(n, self.opcode, d.xids(n), self.arg,
                            self.path_off, self.path_len, self.data_off,
                            self.data_len, self.acl_id, self.path_arena,
                            self.data_arena, self.acl_off, self.acl_len,
                            self.acl_arena)
        rep, _ = d.run(rb)
        self.last = (rb, rep)
        if not validate:
            return None
        ver1 = rep.stat32[0, :n] == 1
        ok = ((rep.status[:n] == 0) & (rep.err[:n] == 0) &
              (rep.xid[:n] == rb.xid) & (rep.opcode[:n] == rb.opcode) &
              (~(self.is_set | self.is_get) | ver1) &
              (~self.is_get | ((rep.stat32[3, :n] == self.data_bytes) &
                               (rep.pay_len[:n] == self.data_bytes))))
        if acc is None:
            return ok.sum()
        acc[:1] += ok.sum()
        return acc

    def diagnose(self):
        rb, rep = self.last
        n = rb.n
        bad = rep.err[:n] != 0
        e, c = torch.unique(rep.err[:n][bad], return_counts=True)
        return {'wrong_err': dict(zip(e.cpu().tolist(), c.cpu().tolist())),
                'order_stats': self.drv.server.order_stats()}


class NestPipeline(object):
    """createWithEmptyParents in one batch (lib/client.js:412-481): every
    step sends, for each of ``m`` trees ``/nest/dDDDD/pKKKKKKKKK``, the
    depth-3 chain CREATE p -> CREATE p/c -> CREATE p/c/g -> EXISTS p ->
    DELETE p/c/g -> DELETE p/c -> DELETE p (7 requests) back to back in ONE
    batch, as one session pipelining them would.  The creates depend on
    their parents, the EXISTS on its children's writes and the deletes on
    their children being gone: the ordered GPU server must honour
    parent / child order (passes by the longest conflict chain, 6 here).
    Every reply is checked on the device: all OK, and the parent's EXISTS
    sees exactly one child (numChildren 1, cversion 1).  The tree is left
    as it was (every step deletes what it created)."""

    PER = 7

    def __init__(self, tree, batch, ndirs=1024, seed=0):
        m = max(batch // self.PER, 1)
        self.m = m
        self.n = n = self.PER * m
        dev = tree.device
        self.tree = tree
        need = 2 * m * (80 + 16)
        if tree.scratch is None or tree.scratch.numel() < need:
            raise ValueError('NestPipeline needs GpuTree(scratch >= %d)'
                             % need)
        base = ['/nest/d%05d/p%09d' % (k % ndirs, k) for k in range(m)]
        paths = [b + sfx for b in base for sfx in ('', '/c', '/c/g')]
        maxp = max(len(p) for p in paths)
        self.drv = _Driver(tree, n, maxp, 16, seed)
        self.drv.passes = 8
        self.path_arena, poff, plen = _arena(paths, dev)
        poff = poff.view(m, 3)
        plen = plen.view(m, 3)
        self.data_arena = torch.full((16,), 0x6e, dtype=U8, device=dev)
        self.acl_arena, self.acl_off, self.acl_len = _acl_table(MIX_ACLS[:1],
                                                                dev)
        ops = consts.OP_CODES
        col = lambda *c: torch.stack(c, 1).reshape(-1)     # noqa: E731
        full = lambda v, dt: torch.full((m,), v, dtype=dt, device=dev)  # noqa
        self.opcode = col(*(full(ops[o], I32) for o in (
            'CREATE', 'CREATE', 'CREATE', 'EXISTS', 'DELETE', 'DELETE',
            'DELETE')))
        # path per request: p, c, g, p, g, c, p
        self.path_off = col(poff[:, 0], poff[:, 1], poff[:, 2], poff[:, 0],
                            poff[:, 2], poff[:, 1], poff[:, 0])
        self.path_len = col(plen[:, 0], plen[:, 1], plen[:, 2], plen[:, 0],
                            plen[:, 2], plen[:, 1], plen[:, 0])
        self.arg = col(full(0, I32), full(0, I32), full(0, I32),
                       full(0, I32), full(-1, I32), full(-1, I32),
                       full(-1, I32))
        self.data_off = torch.zeros(n, dtype=I64, device=dev)
        self.data_len = col(full(4, I32), full(4, I32), full(4, I32),
                            *(full(0, I32) for _ in range(4)))
        self.acl_id = torch.zeros(n, dtype=I32, device=dev)
        self.is_exists = self.opcode == ops['EXISTS']
        self.drv.create_dirs(
            [['/nest'], ['/nest/d%05d' % d for d in range(ndirs)]],
            (self.acl_arena, self.acl_off, self.acl_len))
        self.last = None

    def capture(self, acc):
        """One step as a HIP graph (every step has the same shape)."""
        return _capture_steps(self, acc)

    def step(self, validate=True, acc=None):
        n = self.n
        d = self.drv
        rb = B.RequestBatch(n, self.opcode, d.xids(n), self.arg,
                            self.path_off, self.path_len, self.data_off,
                            self.data_len, self.acl_id, self.path_arena,
                            self.data_arena, self.acl_off, self.acl_len,
                            self.acl_arena)
        rep, _ = d.run(rb)
        self.last = (rb, rep)
        if not validate:
            return None
        one_child = (rep.stat32[4, :n] == 1) & (rep.stat32[1, :n] == 1)
        ok = ((rep.status[:n] == 0) & (rep.err[:n] == 0) &
              (rep.xid[:n] == rb.xid) & (rep.opcode[:n] == rb.opcode) &
              (~self.is_exists | one_child))
        if acc is None:
            return ok.sum()
        acc[:1] += ok.sum()
        return acc

    def diagnose(self):
        rb, rep = self.last
        n = rb.n
        bad = rep.err[:n] != 0
        e, c = torch.unique(rep.err[:n][bad], return_counts=True)
        return {'wrong_err': dict(zip(e.cpu().tolist(), c.cpu().tolist())),
                'order_stats': self.drv.server.order_stats()}


class GpuSessionTable(object):
    """The GPU server's session table in HBM and its handshake (K9 server
    side, csrc/kernels/session.hip): ConnectRequest frames in,
    ConnectResponse frames out, new / resumed / expired decided on the
    device.  Session ids are ``server_id << 56 | (index + 1)`` in allocation
    order, so the server's host side knows the id it handed out without a
    read-back."""

    MIN_TO, MAX_TO = 4000, 40000        # 2 and 20 ticks of 2 s

    def __init__(self, tree, cap=1 << 16, server_id=1, secret=0x5A4B1D,
                 members=1):
        dev = tree.device
        self.tree = tree
        self.dev = dev
        self.cap = cap
        self.server_id = server_id
        self.secret = secret
        # an ensemble of `members` servers replicates its session table:
        # member m's sessions live in slots (m - 1) * span ... (see
        # session.hip); one server's table has no partition
        self.span = cap // members if members > 1 else 0
        self.sid = torch.zeros(cap, dtype=I64, device=dev)
        self.passwd = torch.zeros(cap * 16, dtype=U8, device=dev)
        self.timeout = torch.zeros(cap, dtype=I32, device=dev)
        self.state = torch.zeros(cap, dtype=I32, device=dev)
        self.next = torch.zeros(1, dtype=I64, device=dev)
        self.allocated = 0              # host mirror of `next`
        self._tensors = [self.sid, self.passwd, self.timeout, self.state,
                         self.next]
        self.scanner = B.FrameScanner(64, dev, window=256)
        self.resp = torch.empty(64 * _lib.CR_RESP_BYTES, dtype=U8, device=dev)
        self.resp_sid = torch.empty(64, dtype=I64, device=dev)
        self.outcome = torch.empty(64, dtype=I32, device=dev)

    def sid_of(self, index):
        return (self.server_id << 56) | (index + 1)

    def connect(self, rx, nbytes, n_new):
        """Serve the ConnectRequest stream ``rx[:nbytes]`` (at most 64
        frames); ``n_new`` = how many of them ask for a new session (host
        bookkeeping of the allocation counter).  Returns (response stream
        [41 * frames], bound session ids, outcome codes)."""
        ft = self.scanner.scan(rx, nbytes)
        _lib.lib().session_connect(
            rx, ft.off, ft.length, ft.count, 64, self._tensors,
            self.server_id, _i64(self.secret), self.MIN_TO, self.MAX_TO,
            self.tree.counters[_lib.TC_ZXID:], self.resp, self.resp_sid,
            self.outcome, self.span)
        self.allocated += n_new
        return self.resp, self.resp_sid, self.outcome

    def close(self, sids):
        """Expire / close sessions (device int64 tensor of ids)."""
        _lib.lib().session_close(self._tensors, sids, self.server_id,
                                 self.span)

    def install(self, records):
        """Replicate other members' sessions into this table (device int64
        [k, 4]: sid, timeout, password bytes 0-7 and 8-15; this member's own
        records are skipped) — the receiving end of R3."""
        _lib.lib().session_install(self._tensors, records, self.server_id,
                                   self.span)


class StormPipeline(object):
    """EPHEMERAL|SEQUENTIAL create storm with session expire AND resume
    (BASELINE config 5; lib/zk-session.js:147-205, :265-339,
    test/nasty.test.js:40-103).

    Session ``k`` lives three steps:

      step 2k    born: the client K9-encodes a ConnectRequest with
                 sessionId 0, the GPU server's handshake kernel allocates
                 the session (K9 server side), the client K9-decodes the
                 ConnectResponse; the session creates ``batch`` ephemeral
                 sequential nodes ``/storm/dDDDDD/e-<seq>``; session ``k-1``
                 expires and the server removes its ephemerals, which must
                 be exactly its TWO batches (the one made before its resume
                 survived it)
      step 2k+1  its connection drops; a new one resumes it: ConnectRequest
                 with the id and password from the last ConnectResponse,
                 all on the device; the server answers RESUMED with the same
                 id and password.  In the same handshake batch the client
                 also tries the session that expired at step 2k, which must
                 get the expired answer (id 0).  The resumed session creates
                 its second batch.

    Every check (replies, handshake outcome, ids, password, removed count)
    runs on the device; a step makes no device-to-host read.  The hash
    index needs no rebuild: the expiry moves live entries back over the
    holes it leaves and empties the rest (csrc/kernels/zk_tree.h ht_shift),
    and the next batch's names take over the tombstones their probes pass,
    so never-reused SEQUENTIAL names leave a bounded number of tombstones
    (~0.6 % of the index at the bench's size,
    tools/microbench/storm_census.py).

    Across GPUs (a process group of ``world`` > 1 ranks: the members of one
    ensemble, each rank's GPU server a member) the session MOVES, as
    ``lib/zk-session.js:265-339`` reattaches it to another backend and
    ``test/multi-node.test.js:233-350`` checks that its ephemeral survives:
    session k of rank r is born on member r, and its records {id, timeout,
    password} go to every member (R3: one ``all_gather_into_tensor`` of
    the step's new sessions, installed into each member's replicated
    table).  At step 2k+1 rank r's client resumes it on member (r+1) %
    world: its ConnectRequests travel there and the ConnectResponses back
    through two small all-gathers, member r+1 answers RESUMED with the same
    id and password, and the session's second batch is created on member
    r+1.  Its first batch survives the move on member r; at its expiry
    every member drops what the session created there (so each removes two
    sessions' batches: its own session's first and its neighbour's second)
    and closes it in its table, so the expired resume tried at the next
    move is refused on any member.

    The members hold ONE replicated tree (every rank builds the same tree,
    seed 0, and applies every committed write): a step's write batches of
    all members are all-gathered as encoded CREATE frames and every member
    applies them in rank order — the step's commit order, the zxid order a
    ZooKeeper leader imposes — so sequential names, zxids and ephemeral
    owners come out the same on every member.  The member a client is
    attached to answers it (its reply stream comes back through an
    all-gather after a move).  A znode created through member r is then
    readable and deletable on member r+1 (:meth:`cross_read`; the
    reference's test/multi-node.test.js:107-165 write visibility and
    :233-350 ephemeral-survives-failover), and an expiry removes the
    session's nodes on every member.  The work of a write grows with the
    members (each applies W batches a step): ``stats['replicated_writes']``
    counts what this member applied."""

    TIMEOUT = 30000
    HS_SLOT = 128            # handshake bytes a rank sends per all-gather

    def __init__(self, tree, batch, ndirs=1024, data_bytes=16, seed=0,
                 group=None, coll_device=None):
        import torch.distributed as dist
        dev = tree.device
        self.tree = tree
        self.dev = dev
        self.n = batch
        self.ndirs = ndirs
        on = dist.is_available() and dist.is_initialized()
        self.dist = dist
        self.group = group
        self.world = W = dist.get_world_size(group) if on else 1
        self.rank = dist.get_rank(group) if on else 0
        self.coll = torch.device(coll_device) if coll_device else dev
        self.drv = _Driver(tree, batch, 32, data_bytes, seed,
                           seq_order=True, group=_STORM_SRV_GROUP)
        self.sessions = GpuSessionTable(tree, server_id=self.rank + 1,
                                        members=W)
        if W > 1:
            # the current session of every member on the device (member m's
            # k-th session is (m + 1) << 56 | k + 1, k = kdev): serve and
            # expiry take theirs through the tree's TC_SESS word, so a
            # captured step replays with the next generation's ids
            self.sid_base = torch.tensor([(m + 1) << 56 for m in range(W)],
                                         dtype=I64, device=dev)
            self.sess_tab = torch.zeros(W, dtype=I64, device=dev)
            # this step's new sessions of every member ([W, 4] records),
            # the generation before's (expired at the next birth), and the
            # handshake slots
            self.recs = torch.zeros(W, 4, dtype=I64, device=dev)
            self.prev_recs = torch.zeros(W, 4, dtype=I64, device=dev)
            self.hs_out = torch.zeros(self.HS_SLOT, dtype=U8, device=dev)
            self.hs_all = torch.zeros(W * self.HS_SLOT, dtype=U8, device=dev)
        prefixes = ['/storm/d%05d/e-' % (k % ndirs) for k in range(batch)]
        self.path_arena, self.path_off, self.path_len = _arena(prefixes, dev)
        self.data_arena = torch.full((data_bytes + 16,), 0x5a, dtype=U8,
                                     device=dev)
        self.acl_arena, self.acl_off, self.acl_len = _acl_table(MIX_ACLS[:1],
                                                                dev)
        flags = consts.CREATE_FLAGS['EPHEMERAL'] | \
            consts.CREATE_FLAGS['SEQUENTIAL']
        self.opcode = torch.full((batch,), consts.OP_CODES['CREATE'],
                                 dtype=I32, device=dev)
        self.arg = torch.full((batch,), flags, dtype=I32, device=dev)
        self.data_off = torch.zeros(batch, dtype=I64, device=dev)
        self.data_len = torch.full((batch,), data_bytes, dtype=I32,
                                   device=dev)
        self.acl_id = torch.zeros(batch, dtype=I32, device=dev)
        self.want_len = self.path_len + 10
        self.removed = torch.zeros(1, dtype=I64, device=dev)
        # client-side credentials, device only: [cur, prev] session ids and
        # passwords (what the last ConnectResponses carried)
        self.cred_sid = torch.zeros(2, dtype=I64, device=dev)
        self.cred_pw = torch.zeros(32, dtype=U8, device=dev)
        self.last_zxid = torch.zeros(1, dtype=I64, device=dev)
        self.chk = torch.zeros(1, dtype=I64, device=dev)
        self.hs_ok = torch.ones(1, dtype=torch.bool, device=dev)
        # one member: the handshake beside the request encode, the expiry
        # beside the reply decode, on this second stream
        self.side = torch.cuda.Stream(dev)
        self.cr_tx = torch.empty(256, dtype=U8, device=dev)
        self.cr_ws = torch.empty(_lib.lib().scan_workspace(2),
                                 dtype=I64, device=dev)
        self.rscan = B.FrameScanner(4, dev, window=256)
        # K9 encode arguments per handshake shape (m requests, pwl bytes)
        self.zero_sid = torch.zeros(1, dtype=I64, device=dev)
        self.zero_pw = torch.zeros(8, dtype=U8, device=dev)
        self.cr_args = {}
        for m, pwl in ((1, 8), (1, 16), (2, 16)):
            self.cr_args[(m, pwl)] = (
                torch.zeros(m, dtype=I32, device=dev),
                torch.full((m,), self.TIMEOUT, dtype=I32, device=dev),
                torch.arange(m, dtype=I64, device=dev) * pwl,
                torch.full((m,), pwl, dtype=I32, device=dev),
                torch.empty(m, dtype=I64, device=dev),
                torch.empty(m, dtype=I64, device=dev),
                torch.zeros(1, dtype=I64, device=dev))
        self.k = -1                       # index of the current session
        # ... and on the device (a captured step replays with the next
        # session's ids: serve / expire take them from the tree's TC_SESS)
        self.kdev = torch.full((1,), -1, dtype=I64, device=dev)
        self.sid0 = self.sessions.sid_of(0)
        self._capturing = False
        self.step_no = 0
        self.stats = {'born': 0, 'resumed': 0, 'expired': 0,
                      'expired_resume_refused': 0, 'cross_rank_resumes': 0}
        # replicated tree (see the class docs): the step's stream slots
        self.req_bytes = None       # a batch's encoded bytes (constant)
        self.rep_bytes = None
        self.len_ok = torch.ones(1, dtype=torch.bool, device=dev)
        if W > 1:
            self.stats['replicated_writes'] = 0
        self.first = None           # the current session's first batch
        self.drv.create_dirs(
            [['/storm'], ['/storm/d%05d' % d for d in range(ndirs)]],
            (self.acl_arena, self.acl_off, self.acl_len))
        self.step(validate=False)            # session 0 born, first batch

    # -- the client / server handshake, all on the device ---------------------

    def _gather(self, out, inp):
        """``all_gather_into_tensor`` on the collective device."""
        if self.coll == self.dev:
            self.dist.all_gather_into_tensor(out, inp, group=self.group)
            return out
        o = torch.empty(out.shape, dtype=out.dtype, device=self.coll)
        self.dist.all_gather_into_tensor(o, inp.to(self.coll),
                                         group=self.group)
        out.copy_(o)
        return out

    def sid(self, member, k):
        """Session id of member ``member``'s k-th session (every member
        allocates one a birth step, so ids are known on every rank)."""
        return ((member + 1) << 56) | (k + 1)

    def _handshake(self, resume):
        """K9 client encode -> K9 server handshake -> K9 client decode.
        Birth: one request (id 0, 8 zero password bytes as zkstream sends,
        lib/zk-session.js:59).  Resume: [current session, the session that
        expired last step] with their ids and passwords — on the next
        member when the ensemble spans GPUs (the frames go there and the
        answers come back through all-gathers)."""
        L = _lib.lib()
        # the first session has no expired predecessor to try
        m = 2 if resume and self.k >= 1 else 1
        pwl = 16 if resume else 8
        if resume:
            sid = self.cred_sid[:m]
            arena = self.cred_pw[:16 * m]
        else:
            sid = self.zero_sid
            arena = self.zero_pw
        proto, tmo, pwo, pwlt, sizes, off, total = self.cr_args[(m, pwl)]
        zx = self.last_zxid.expand(m).contiguous()
        L.encode_connect_requests(proto, zx, tmo, sid, pwo, pwlt, arena, m,
                                  sizes, off, total, self.cr_ws, self.cr_tx)
        nbytes = m * (32 + pwl)
        rb = m * _lib.CR_RESP_BYTES
        W = self.world
        if resume and W > 1:
            # to member r + 1: every rank's frames gathered, each serves
            # the previous rank's, the answers gathered back
            S = self.HS_SLOT
            self.hs_out[:nbytes].copy_(self.cr_tx[:nbytes])
            self._gather(self.hs_all, self.hs_out)
            src = (self.rank - 1) % W
            rx = self.hs_all[src * S:src * S + nbytes].clone()
            resp, bound, outcome = self.sessions.connect(rx, nbytes, 0)
            self.hs_out[:rb].copy_(resp[:rb])
            self._gather(self.hs_all, self.hs_out)
            dst = (self.rank + 1) % W
            resp = self.hs_all[dst * S:dst * S + rb].clone()
            ft = self.rscan.scan(resp, rb)
            o = B.decode_connect_responses(resp, ft, m)
            # (`outcome`: how this member answered the previous rank's
            # client — every member checks the one it served, the client
            # checks the answer it got)
            return o, bound, outcome, resp
        resp, bound, outcome = self.sessions.connect(
            self.cr_tx[:nbytes], nbytes, 0)
        ft = self.rscan.scan(resp[:rb], rb)
        o = B.decode_connect_responses(resp, ft, m)
        return o, bound, outcome, resp

    @property
    def capturable(self):
        """One member, or an ensemble whose all-gathers run on RCCL on the
        pipeline's device (a host backend cannot be captured)."""
        if self.world == 1:
            return True
        return self.coll == self.dev and \
            self.dist.get_backend(self.group) == 'nccl'

    def capture(self, acc):
        """Capture the steady state's two step shapes (a birth that expires
        the session before, a resume that also tries the expired one) as
        HIP graphs; ``replay()`` runs the next step.  Session ids live on
        the device (``kdev`` -> the tree's TC_SESS word; across members the
        table of every member's current id), so a replay serves, expires
        and checks the next session; the host keeps only its bookkeeping
        (counts).  Across members the all-gathers are captured with the
        rest (RCCL; see ``capturable``)."""
        if not self.capturable:
            raise RuntimeError('storm capture: the process group cannot be '
                               'captured (host backend)')
        while self.step_no < 2 or self.step_no % 2:
            self.step(acc=acc)
        torch.cuda.synchronize(self.dev)
        keep = (self.step_no, self.k, dict(self.stats),
                self.sessions.allocated)
        graphs = []
        self._capturing = True
        try:
            for _ in range(2):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode='thread_local'):
                    self.step(acc=acc)
                graphs.append(g)
        finally:
            self._capturing = False
        (self.step_no, self.k, self.stats,
         self.sessions.allocated) = keep
        return _StormCycle(self, graphs)

    def _advance(self):
        """The host side of a step (eager and replayed alike): step and
        session counters, stats.  Returns resume."""
        s = self.step_no
        self.step_no += 1
        resume = s % 2 == 1
        if self.world > 1:
            self.stats['replicated_writes'] += self.world * self.n
            self.stats['cross_rank_resumes'] += int(resume)
        if resume:
            self.stats['resumed'] += 1
            self.stats['expired_resume_refused'] += int(self.k >= 1)
        else:
            self.k += 1
            self.sessions.allocated += 1
            self.stats['born'] += 1
            if self.k >= 1:
                self.stats['expired'] += 1
        return resume

    def step(self, validate=True, acc=None):
        t = self.tree
        n = self.n
        resume = self._advance()
        if not resume:
            self.kdev.add_(1)
        # this step's session on the device (one member: its own; the
        # ensemble passes host ids, see _replicated_run)
        sess_dev = t.counters[_lib.TC_SESS:_lib.TC_SESS + 1]
        torch.add(self.kdev, self.sid0, out=sess_dev)
        if self.world == 1:
            return self._step_two_streams(resume, sess_dev, validate, acc)
        torch.add(self.sid_base, self.kdev + 1, out=self.sess_tab)
        o, bound, outcome, resp = self._handshake(resume)
        self._check_handshake(resume, sess_dev, o, bound, outcome, resp)
        rb = self._batch()
        rep = self._replicated_run(rb, resume)
        self.last = (rb, rep)
        if not resume:
            # the new session's first batch: the created paths (offsets into
            # the reply stream kept with them), for cross_read
            self.first = (self.my_rx.clone(), rep.pay_off[:n].clone(),
                          rep.pay_len[:n].clone())
        self._check_replies(rb, rep)
        expire_ok = True
        if not resume and self.k >= 1:
            # the generation before expires on every member, which holds
            # all members' sessions' nodes (the replicated tree): each of
            # them created two batches — here its first batch (our
            # session) and its second (the previous member's, which moved
            # here); every member closes all of them
            self.removed.zero_()
            for m in range(self.world):
                # member m's session of the generation before
                torch.sub(self.sess_tab[m:m + 1], 1, out=sess_dev)
                t.expire(_lib.SESS_DEV, self.removed)
            self.sessions.close(self.prev_recs[:, 0].contiguous())
            expire_ok = self.removed[0] == 2 * n * self.world
        return self._tally(validate, acc, expire_ok)

    def _check_handshake(self, resume, sess_dev, o, bound, outcome, resp):
        """The outcome check (and, at a birth, the credentials' update) in
        one launch: a resume comes back RESUMED with the same id, password
        and timeout, the expired one beside it refused; a birth is NEW with
        member r's k-th session id (csrc/kernels/bench.hip)."""
        want = sess_dev if self.world == 1 else \
            self.sess_tab[self.rank:self.rank + 1]
        _lib.lib().bench_storm_hs(
            resume, resume and self.k >= 1, self.TIMEOUT, o['status'],
            o['sessionId'], o['timeOut'], outcome, bound, resp, want,
            self.cred_sid, self.cred_pw, self.hs_ok)
        if not resume and self.world > 1:
            # R3: every member's new session to every member
            self.prev_recs.copy_(self.recs)
            mine = torch.cat([o['sessionId'][0:1],
                              o['timeOut'][0:1].to(I64),
                              resp[24:40].view(I64)])
            self._gather(self.recs.view(-1), mine)
            self.sessions.install(self.recs)

    def _batch(self):
        n = self.n
        return B.RequestBatch(n, self.opcode, self.drv.xids(n), self.arg,
                              self.path_off, self.path_len, self.data_off,
                              self.data_len, self.acl_id, self.path_arena,
                              self.data_arena, self.acl_off, self.acl_len,
                              self.acl_arena)

    def _check_replies(self, rb, rep):
        """The replies' check (counted into chk) and the batch's largest
        zxid (into last_zxid), one fused pass (csrc/kernels/bench.hip)."""
        self.chk.zero_()
        _lib.lib().bench_check_writes(self.n, rep.status, rep.err, rep.xid,
                                      rb.xid, rep.pay_len, self.want_len, -1,
                                      rep.zxid, self.chk, self.last_zxid)

    def _expire_prev(self, sess_dev):
        """The previous session expires: both of its batches go (its id, the
        current one's less one, through TC_SESS); `removed` counts them."""
        sess_dev.sub_(1)
        self.removed.zero_()
        self.tree.expire(_lib.SESS_DEV, self.removed)
        self.sessions.close(sess_dev)        # (the expired id, on the device)

    def _tally(self, validate, acc, expire_ok):
        if not validate:
            return None
        good = torch.where(self.hs_ok[0] & self.len_ok[0] & expire_ok,
                           self.chk[0], 0)
        if acc is None:
            return good
        acc[:1] += good
        return acc

    def _step_two_streams(self, resume, sess_dev, validate, acc):
        """One member's step on two streams: the handshake (K9 encode, the
        server's session table, K1 + K9 decode, its check) on the side
        stream beside the request encode; the serve once both are done; then
        the expiry of the previous session on the side stream beside the
        reply-stream scan, decode and check.  The tree is touched by one
        stream at a time (the handshake reads the zxid counter before the
        serve, the expiry writes the tree after it, the reply decode never
        reads it)."""
        d = self.drv
        cur = torch.cuda.current_stream(self.dev)
        side = self.side
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            o, bound, outcome, resp = self._handshake(resume)
            self._check_handshake(resume, sess_dev, o, bound, outcome, resp)
        rb = self._batch()
        tx, _, total, _ = B.encode_requests(rb, d.xt, out=d.tx)
        cur.wait_stream(side)
        rx, rtotal, _, _ = d.server.serve(tx, _len(total),
                                          session=_lib.SESS_DEV,
                                          ordered=d.passes > 0,
                                          passes=max(d.passes, 1))
        expiring = not resume and self.k >= 1
        if expiring:
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._expire_prev(sess_dev)
        if d.rscanner is None:
            d.rscanner = B.FrameScanner(self.n, self.dev, window=d.rwindow)
        ft = d.rscanner.scan(rx, _len(rtotal))
        rep = B.decode_replies(rx, ft, d.xt, out=d.reply)
        self.last = (rb, rep)
        self._check_replies(rb, rep)
        expire_ok = True
        if expiring:
            cur.wait_stream(side)
            expire_ok = self.removed[0] == 2 * self.n
        return self._tally(validate, acc, expire_ok)

    # -- the replicated tree --------------------------------------------------

    def _stream_len(self, total, attr):
        """The byte length of a batch's encoded stream: the same every step
        (fixed-size records), read from the device once; later steps check
        it on the device (len_ok)."""
        v = getattr(self, attr)
        if v is None:
            v = int(total.item())
            setattr(self, attr, v)
            return v
        self.len_ok &= total.view(-1)[0] == v
        return v

    def _replicated_run(self, rb, resume):
        """Every member's batch applied on every member, in rank order; the
        reply stream of the client this member answers goes back to it."""
        d = self.drv
        W, r, n = self.world, self.rank, self.n
        tx, _, total, _ = B.encode_requests(rb, d.xt, out=d.tx)
        S = self._stream_len(total, 'req_bytes')
        if not hasattr(self, 'tx_all'):
            self.tx_all = torch.empty(W * S, dtype=U8, device=self.dev)
        self._gather(self.tx_all, tx[:S])
        # the client this member answers: its own, or after a move the
        # previous member's
        ans = (r - 1) % W if resume else r
        sess_dev = self.tree.counters[_lib.TC_SESS:_lib.TC_SESS + 1]
        for m in range(W):
            sess_dev.copy_(self.sess_tab[m:m + 1])
            rx, rtotal, _, _ = d.server.serve(
                self.tx_all[m * S:(m + 1) * S], S, session=_lib.SESS_DEV,
                ordered=d.passes > 0, passes=max(d.passes, 1))
            if m == ans:
                R = self._stream_len(rtotal, 'rep_bytes')
                if not hasattr(self, 'rep_out'):
                    self.rep_out = torch.empty(R + 64, dtype=U8,
                                               device=self.dev)
                    self.rep_all = torch.empty(W * R, dtype=U8,
                                               device=self.dev)
                    self.my_rx = torch.empty(R + 64, dtype=U8,
                                             device=self.dev)
                self.rep_out[:R].copy_(rx[:R])
        R = self.rep_bytes
        if resume:
            # my answers come from the member my session moved to
            self._gather(self.rep_all, self.rep_out[:R])
            src = (r + 1) % W
            self.my_rx[:R].copy_(self.rep_all[src * R:(src + 1) * R])
        else:
            self.my_rx[:R].copy_(self.rep_out[:R])
        if d.rscanner is None:
            d.rscanner = B.FrameScanner(self.n, self.dev, window=d.rwindow)
        ft = d.rscanner.scan(self.my_rx, R)
        return B.decode_replies(self.my_rx, ft, d.xt, out=d.reply)

    def cross_read(self):
        """Write visibility across members: this rank's client reads its
        current session's FIRST batch (created through the member the
        session was born on) with EXISTS at the NEXT member — the requests
        go there and the replies come back through all-gathers.  Returns
        the device count of nodes found with this session as their
        ephemeral owner (every member calls it together)."""
        if self.world < 2 or self.first is None:
            raise RuntimeError('cross_read needs an ensemble across GPUs '
                               'and a born session')
        d = self.drv
        W, r, n, dev = self.world, self.rank, self.n, self.dev
        arena, poff, plen = self.first
        z32 = torch.zeros(n, dtype=I32, device=dev)
        rb = B.RequestBatch(n, torch.full((n,), consts.OP_CODES['EXISTS'],
                                          dtype=I32, device=dev),
                            d.xids(n), z32, poff, plen,
                            torch.zeros(n, dtype=I64, device=dev), z32, z32,
                            arena, arena, self.acl_off, self.acl_len,
                            self.acl_arena)
        tx, _, total, _ = B.encode_requests(rb, d.xt, out=d.tx)
        S = int(total.item())
        sizes = self._gather(torch.empty(W, dtype=I64, device=dev),
                             torch.tensor([S], dtype=I64, device=dev)).cpu()
        Smax = int(sizes.max())
        buf = torch.zeros(Smax, dtype=U8, device=dev)
        buf[:S].copy_(tx[:S])
        allq = torch.empty(W * Smax, dtype=U8, device=dev)
        self._gather(allq, buf)
        # serve the previous rank's reads here (member r + 1 of its client)
        src = (r - 1) % W
        rx, rtotal, _, _ = d.server.serve(
            allq[src * Smax:src * Smax + int(sizes[src])], int(sizes[src]),
            session=self.sid(src, self.k))
        R = int(rtotal.item())
        ra = self._gather(torch.empty(W, dtype=I64, device=dev),
                          torch.tensor([R], dtype=I64, device=dev)).cpu()
        Rmax = int(ra.max())
        out = torch.zeros(Rmax, dtype=U8, device=dev)
        out[:R].copy_(rx[:R])
        alla = torch.empty(W * Rmax, dtype=U8, device=dev)
        self._gather(alla, out)
        dst = (r + 1) % W
        mine = alla[dst * Rmax:dst * Rmax + int(ra[dst])].clone()
        sc = B.FrameScanner(n, dev, window=256)
        ft = sc.scan(mine, int(ra[dst]))
        rep = B.decode_replies(mine, ft, d.xt)
        owner = self.sid(r, self.k)
        found = ((rep.status[:n] == 0) & (rep.err[:n] == 0) &
                 (rep.stat64[4][:n] == owner)).sum()
        return found

    def diagnose(self):
        rb, rep = self.last
        n = self.n
        e, c = torch.unique(rep.err[:n], return_counts=True)
        return {'removed': int(self.removed.item()),
                'handshakes_ok': bool(self.hs_ok.item()),
                'outcome': self.sessions.outcome[:2].cpu().tolist(),
                'err_hist': dict(zip(e.cpu().tolist(), c.cpu().tolist())),
                'status_bad': int((rep.status[:n] != 0).sum().item()),
                'pay_len_bad': int((rep.pay_len[:n] != self.want_len)
                                   .sum().item()),
                'stats': dict(self.stats),
                'counters': self.tree.counters.cpu().tolist()}


class _StormCycle(object):
    """The storm's two captured step shapes replayed in turn, the host
    bookkeeping of each step done first (see StormPipeline.capture)."""

    def __init__(self, pipe, graphs):
        self.pipe = pipe
        self.graphs = graphs

    def replay(self):
        resume = self.pipe._advance()
        self.graphs[1 if resume else 0].replay()


class WatchPipeline(object):
    """Watch fan-out across the node driven by real writes (BASELINE config
    4's data path, R1 at scale).  Every rank's GPU server keeps a watch
    table (:class:`GpuTree` ``watch_cap``); one step on rank ``r``:

      arm     the watcher session (slot 0) sends ``batch`` GET_DATA with
              watch=1 for distinct nodes (K10 -> K1 -> lookup + arm -> K13
              -> K1 + K2-K4, every reply checked on the device)
      write   the writer session (slot 1) SET_DATAs the same nodes; each
              write fires its node's watch (lib/zk-session.js:558-574): the
              server expands the fired masks and K13-encodes one
              NodeDataChanged notification frame (xid -1) per node, in
              write order; the writes' replies are checked too
      R1      the notification streams of all ranks travel in equal-size
              slots ({bytes, frames} header + frames) through one
              ``all_gather_into_tensor`` (RCCL over xGMI with ``nccl``;
              :meth:`~zkmi.parallel.fanout.FrameFanout.gather_slots`, the
              one R1 path's sync-free transport); every rank concatenates
              them (``seg_unpack``), K1 + K8
              decodes ALL ranks' notifications and checks each on the
              device: NodeDataChanged, SyncConnected, and the path of the
              node that rank's writer set at that position

    One step delivers ``world * batch`` notifications to every rank:
    ``world**2 * batch`` deliveries node-wide (:attr:`per_step`).
    ``coll_device='cpu'`` runs the all-gather on host tensors (gloo
    rehearsal).  A step makes no device-to-host read; on one GPU, or with
    the all-gather on it, steps are captured as HIP graphs
    (:meth:`capture`)."""

    def __init__(self, tree, batch, seed=0, group=None, coll_device=None):
        import torch.distributed as dist
        if tree.watch is None:
            raise ValueError('WatchPipeline needs GpuTree(watch_cap=...)')
        self.dist = dist
        self.group = group
        on = dist.is_available() and dist.is_initialized()
        self.world = W = dist.get_world_size(group) if on else 1
        self.rank = dist.get_rank(group) if on else 0
        self.tree = tree
        # distinct nodes per step: at most the tree's leaves
        self.n = n = min(batch, tree.n_leaves)
        dev = tree.device
        self.dev = dev
        self.coll_device = torch.device(coll_device) if coll_device else dev
        self.per_step = W * W * n
        maxpath = int(tree.node_path_len.max().item())
        self.data_bytes = min(tree.data_bytes, 128)
        self.j = torch.arange(n, dtype=I64, device=dev)
        self.jw = torch.arange(W * n, dtype=I64, device=dev) % n
        self.rank_of = torch.arange(W * n, dtype=I64, device=dev) // n
        # the sessions' next xid, on the device: a captured step replays
        # with new xids
        self.xid_iota = torch.arange(n, dtype=I64, device=dev)
        self.xid_dev = torch.zeros(1, dtype=I64, device=dev)
        self.ops_get = torch.full((n,), consts.OP_CODES['GET_DATA'],
                                  dtype=I32, device=dev)
        self.ops_set = torch.full((n,), consts.OP_CODES['SET_DATA'],
                                  dtype=I32, device=dev)
        self.one32 = torch.ones(n, dtype=I32, device=dev)
        self.neg32 = torch.full((n,), -1, dtype=I32, device=dev)
        self.zero32 = torch.zeros(n, dtype=I32, device=dev)
        self.zero64 = torch.zeros(n, dtype=I64, device=dev)
        g = torch.Generator(device=dev)
        g.manual_seed(seed + 23)
        self.data_arena = torch.randint(0, 256, (n * self.data_bytes + 16,),
                                        dtype=U8, device=dev, generator=g)
        self.data_off = self.j * self.data_bytes
        self.data_len = torch.full((n,), self.data_bytes, dtype=I32,
                                   device=dev)
        self.acl_off = torch.zeros(1, dtype=I64, device=dev)
        self.acl_len = torch.zeros(1, dtype=I32, device=dev)
        self.acl_arena = torch.zeros(16, dtype=U8, device=dev)
        self.tx = torch.empty(n * (33 + maxpath + self.data_bytes) + 64,
                              dtype=U8, device=dev)
        self.xt = B.XidTable(bits=max(12, (n - 1).bit_length() + 1),
                             device=dev)
        rep_max = 4 + 16 + 4 + max(tree.data_bytes, 128) + 68
        self.server = GpuServer(tree, n, n * rep_max + 64,
                                window=B.frame_window(33 + maxpath +
                                                      self.data_bytes),
                                seq_order=False)
        self.rscan = B.FrameScanner(n, dev, window=B.frame_window(rep_max))
        self.reply = B.alloc_replies(n, dev)
        # R1 slots: one notification stream per rank
        rec = 4 + 16 + 4 + 4 + 4 + maxpath
        self.rec_max = rec
        self.slot = (16 + n * rec + 15) & ~15
        from ..parallel.fanout import FrameFanout
        self.fan = FrameFanout(group, device=dev,
                               coll_device=self.coll_device)
        self.pstats = None
        self.nscan = B.FrameScanner(W * n, dev, window=B.frame_window(rec))
        self.nreply = B.alloc_replies(W * n, dev)
        self.nxt = B.XidTable(bits=10, device=dev)
        self.sid_w = (2 << 56) | (self.rank + 1)
        self.sid_wr = (3 << 56) | (self.rank + 1)
        self.seed = seed
        self.step_no = 0
        self.last = None
        self.stats = {'armed': 0, 'written': 0, 'notified': 0}

    def _affine(self, rank, step):
        """(a, b) of the distinct nodes rank ``rank`` watches and writes at
        ``step``: node leaf0 + (a * j + b) % n_leaves, a coprime with
        n_leaves (a permutation, so the batch's nodes are distinct)."""
        import math
        nl = self.tree.n_leaves
        h = (rank + 1) * 0x9E3779B97F4A7C15 + (step + 1) * 0xBF58476D1CE4E5B9 \
            + self.seed * 0x94D049BB133111EB
        h &= (1 << 62) - 1
        a = (h % max(nl - 1, 1)) + 1
        while math.gcd(a, nl) != 1:
            a += 1
        b = (h >> 20) % nl
        return a, b

    def _batch(self, ops, arg, idx, xid, data):
        t = self.tree
        poff = t.node_path_off[idx]
        plen = t.node_path_len[idx]
        if data:
            doff, dlen = self.data_off, self.data_len
        else:
            doff, dlen = self.zero64, self.zero32
        return B.RequestBatch(self.n, ops, xid, arg, poff, plen, doff, dlen,
                              self.zero32, t.path_arena, self.data_arena,
                              self.acl_off, self.acl_len, self.acl_arena)

    def _xids(self):
        x = ((self.xid_iota + self.xid_dev) & 0x7fffffff).to(I32)
        self.xid_dev.add_(self.n)
        return x

    @property
    def capturable(self):
        """The R1 all-gather is captured with the step when it runs on this
        GPU (RCCL); a gloo rehearsal's host all-gather is not."""
        return self.world == 1 or self.coll_device == self.dev

    def capture(self, acc, cycle=8):
        """``cycle`` HIP graphs, replayed in turn: a step's watched and
        written nodes are an affine permutation the host picks per step
        (:meth:`_affine`), so each graph holds one step of a cycle of
        ``cycle`` node sets; xids come from a device counter."""
        return _capture_steps(self, acc, cycle, counter='step_no')

    def _roundtrip(self, rb, session, wslot, check=None):
        tx, _, total, _ = B.encode_requests(rb, self.xt, out=self.tx)
        out, rtotal, _, _ = self.server.serve(tx, total, session=session,
                                              wslot=wslot)
        ft = self.rscan.scan(out, rtotal)
        return B.decode_replies(out, ft, self.xt, out=self.reply,
                                check=check)

    def step(self, validate=True, acc=None):
        t = self.tree
        n = self.n
        W = self.world
        L = _lib.lib()
        if acc is None:
            acc = torch.zeros(1, dtype=I64, device=self.dev)
        nl = t.n_leaves
        a, b = self._affine(self.rank, self.step_no)
        idx = t.leaf0 + (self.j * a + b) % nl
        # arm: GET_DATA watch=1 from the watcher session (slot 0)
        xid = self._xids()
        arm = acc.new_zeros(1)
        self._roundtrip(self._batch(self.ops_get, self.one32, idx, xid,
                                    False), self.sid_w, 0,
                        check=(idx, xid, t.data_len, arm))
        # write: SET_DATA of the same nodes from the writer (slot 1)
        rep = self._roundtrip(self._batch(self.ops_set, self.neg32, idx,
                                          self._xids(), True),
                              self.sid_wr, 1)
        wrote = ((rep.status[:n] == 0) & (rep.err[:n] == 0)).sum()
        # R1: every rank's notification stream to every rank (FrameFanout's
        # fixed-slot transport: no host read in the step)
        nbuf, ntotal, _, ncount = self.server.notif
        self.rx, self.nrx, self.src_counts, self.pstats = \
            self.fan.gather_slots(nbuf, self.server.notif_rec_off, ncount,
                                  self.server.ecap, ntotal, self.slot)
        ft = self.nscan.scan(self.rx, self.nrx)
        nrep = B.decode_replies(self.rx, ft, self.nxt, out=self.nreply)
        self.step_no += 1
        self.last = (nrep, ft, idx)
        if not validate:
            return None
        # the nodes every rank's writer set, in write order
        want = torch.empty(W * n, dtype=I64, device=self.dev)
        for r in range(W):
            ar, br = self._affine(r, self.step_no - 1)
            want[r * n:(r + 1) * n] = t.leaf0 + (self.j * ar + br) % nl
        good = torch.zeros(1, dtype=I64, device=self.dev)
        L.bench_check_notif(W * n, n, self.zero64[:1], t.leaf0, nl,
                            t.node_path_off, t.node_path_len, t.path_arena,
                            self.rx, nrep.tensors(), good, want)
        # a step counts only if every arm and write answered OK
        ok = (arm[0] == n) & (wrote == n) & (ft.count[0] == W * n)
        acc[:1] += torch.where(ok, good, torch.zeros_like(good))
        self.stats['armed'] += n
        self.stats['written'] += n
        self.stats['notified'] += W * n
        return acc

    def diagnose(self):
        nrep, ft, idx = self.last
        return {'frames': ft.host_result(),
                'status_bad': int((nrep.status != 0).sum().item()),
                'opcodes': torch.unique(nrep.opcode).cpu().tolist(),
                'events': self.server.ev_total.cpu().tolist(),
                'overflow': self.pstats.cpu().tolist()}
