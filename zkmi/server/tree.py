"""The HBM tree's host side: :class:`GpuTree` builds the znode tables on the
device (a synthetic ``/bench`` fill or a byte image) for csrc/kernels/tree*."""

import time

import numpy as np
import torch

from ..ops import _lib, batch as B

I64, I32, U8 = torch.int64, torch.int32, torch.uint8


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
