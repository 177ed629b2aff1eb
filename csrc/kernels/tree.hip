// The GPU tree's core passes (layout, claims and the ordering contract:
// zk_tree.h): fill / build and the free-ring compaction, the serve kernel,
// the between-batch finish and the session expiry, the digest.  Each group's
// launchers stand below its kernels.  The other passes have a file each:
// tree_order.hip (in-batch ordering and the ordered serve), tree_seq.hip
// (SEQUENTIAL numbering), tree_list.hip (GET_CHILDREN*), tree_watch.hip
// (watch events and the SET_WATCHES catch-up), tree_acl.hip, tree_mix.hip,
// tree_snap.hip (the image: snapshot and load).
#include "zk_tree.h"
#include "zk_frame_rows.h"

namespace zk {

__global__ __launch_bounds__(TR_T) void tree_fill_k(ZkTree t, int64_t n0,
                                                   int64_t n,
                                                   const int32_t* __restrict__ nkids,
                                                   int64_t now_ms) {
  const int64_t v = n0 + (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (v >= n) return;
  const ZkNodeStore& s = t.store;
  uint8_t* slot = s.slab + s.slot_off[v];
  const int32_t dl = s.data_len[v];
  fill_stat(slot, v + 1, v + 1, now_ms, now_ms, 0, nkids[v], 0, 0, dl,
            nkids[v], v + 1);
  st_be32(slot + 68, 0);
  st_be32(slot + ZK_SLOT_LEN, dl > 0 ? dl : -1);
  t.cn[v] = cn_pack(nkids[v], nkids[v]);
  t.pzxid[v] = v + 1;
  t.eph[v] = 0;
  t.dirty[v] = 0;
}

// Free-ring compaction between batches: the ring's pending entries rebuilt
// as every free node in ascending order.  Frees go to the ring in the
// order the workgroups of a batch happened to take their ticket, and
// creates take the ring in ticket order too, so over a few hundred batches
// of create / delete the nodes one workgroup creates scatter over the whole
// node table (each per-node field a random line instead of a shared one):
// the mix step drifted 1.42 -> 1.65 ms and the nest step 6.26 -> 7.78 ms
// over 600 / 200 steps (profiles/r5_free_ring_locality.md).  Sorted, a
// workgroup's creates take nodes from one dense run again.  Two passes and
// a scan over the node high-water mark; at a batch boundary the pending
// entries are exactly the free nodes (the finish published every free).
__global__ __launch_bounds__(TR_T) void free_count_k(ZkTree t,
                                                    int64_t* __restrict__ bsum) {
  __shared__ int32_t c[TR_T / 64];
  const int64_t nn = min(t.counters[TC_NODES], t.store.cap);
  const int64_t v = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const bool f = v < nn && t.node_parent[v] == NODE_FREE;
  const uint64_t m = __ballot(f);
  if ((threadIdx.x & 63) == 0) c[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t s = 0;
    for (int k = 0; k < TR_T / 64; ++k) s += c[k];
    bsum[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(TR_T) void free_scatter_k(
    ZkTree t, const int64_t* __restrict__ bbase,
    const int64_t* __restrict__ total) {
  __shared__ int32_t c[TR_T / 64];
  const int64_t head = t.counters[TC_FREE_HEAD];
  const int64_t nn = min(t.counters[TC_NODES], t.store.cap);
  const int64_t v = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const bool f = v < nn && t.node_parent[v] == NODE_FREE;
  const uint64_t m = __ballot(f);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) c[w] = __popcll(m);
  __syncthreads();
  int64_t r = bbase[blockIdx.x] +
              __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                        __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
  for (int k = 0; k < w; ++k) r += c[k];
  if (f) t.free_list[(head + r) % t.free_cap] = v;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    t.counters[TC_FREE_TAIL] = head + *total;
    t.counters[TC_FREE_PUB] = head + *total;
  }
}

__global__ __launch_bounds__(TR_T) void tree_build_k(ZkTree t, int64_t n0,
                                                    int64_t n) {
  const int64_t v = n0 + (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (v >= n || t.node_parent[v] == NODE_FREE) return;
  tree_insert(t, v, t.path_arena + t.node_path_off[v], t.node_path_len[v],
              t.store.data_len[v]);
}

}  // namespace zk

extern "C" {

int zk_tree_fill(const ZkTree* t, int64_t n0, int64_t n, const int32_t* nkids,
                 int64_t now_ms, hipStream_t st) {
  if (n <= n0) return 0;
  const int64_t m = n - n0;
  zk::tree_fill_k<<<(unsigned)((m + zk::TR_T - 1) / zk::TR_T), zk::TR_T, 0,
                    st>>>(*t, n0, n, nkids, now_ms);
  ZK_LAUNCH_CHECK();
  return 0;
}

// Workspace (int64) of zk_tree_free_compact for a node capacity.
int64_t zk_tree_free_workspace(int64_t cap) {
  const int64_t nb = (cap + zk::TR_T - 1) / zk::TR_T;
  return 2 * nb + 8 + zk_scan_workspace(nb);
}

// The free ring's pending entries rebuilt in node order (free_count_k).
int zk_tree_free_compact(const ZkTree* t, int64_t* ws, hipStream_t st) {
  const int64_t nb = (t->store.cap + zk::TR_T - 1) / zk::TR_T;
  if (nb <= 0) return 0;
  int64_t* bsum = ws;
  int64_t* bbase = ws + nb;
  int64_t* total = ws + 2 * nb;
  zk::free_count_k<<<(unsigned)nb, zk::TR_T, 0, st>>>(*t, bsum);
  ZK_LAUNCH_CHECK();
  int rc = zk_scan_excl_i64(bsum, bbase, nb, total, ws + 2 * nb + 8, st);
  if (rc) return rc;
  zk::free_scatter_k<<<(unsigned)nb, zk::TR_T, 0, st>>>(*t, bbase, total);
  ZK_LAUNCH_CHECK();
  return 0;
}

// Every hash entry back to empty: all zero bytes (val_pack), one memset.
// (Round 5's first reset wrote {0, -3, 0...} entries from a kernel: 2.2 ms
// for the storm's 4 GB table.)
int zk_tree_ht_reset(const ZkTree* t, hipStream_t st) {
  return hipMemsetAsync(t->ht, 0, (size_t)(t->mask + 1) * zk::HT_W * 8, st);
}

int zk_tree_build(const ZkTree* t, int64_t n0, int64_t n, hipStream_t st) {
  if (n <= n0) return 0;
  const int64_t m = n - n0;
  zk::tree_build_k<<<(unsigned)((m + zk::TR_T - 1) / zk::TR_T), zk::TR_T, 0,
                     st>>>(*t, n0, n);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

namespace zk {

// Write "%010d" of a non-negative sequence number (ZooKeeper's sequential
// suffix; the counter is the parent's cversion).
ZK_DEV void put_seq10(uint8_t* d, int32_t x) {
  uint32_t u = (uint32_t)x;
#pragma unroll
  for (int k = 9; k >= 0; --k) { d[k] = (uint8_t)('0' + u % 10); u /= 10; }
}

// Per-lane state of one request through the three phases of tree_serve_k.
struct Lane {
  int32_t op, err, pl, dl, flags, dlen;
  int64_t node, zx, par, slot;
  const uint8_t* path;
};

// Reply frame size (length word included) of a served request, as
// encode.hip's resp_body_size computes it from the reply descriptors.
ZK_DEV int64_t served_reply_size(int32_t op, int32_t err, int32_t dl,
                                 int32_t rpl) {
  const int64_t sz = 4 + 16;                    // length, xid, zxid, err
  if (err != ERR_OK) return sz;
  switch (op) {
    case OP_GET_DATA: return sz + 4 + max(dl, 0) + STAT_BYTES;
    case OP_EXISTS: case OP_SET_DATA: return sz + STAT_BYTES;
    case OP_CREATE: return sz + 4 + max(rpl, 0);
    default: return sz;
  }
}

// The ordering pass's word for request i (zk_tree_seq_order): parent node
// << 32 | its SEQUENTIAL number, -1 when it has none.
ZK_DEV int32_t seq_num(const ZkTree& t, int64_t i) {
  if (t.seqno == nullptr) return -1;
  const int64_t x = t.seqno[i];
  return x < 0 ? -1 : (int32_t)(uint32_t)x;
}
ZK_DEV int64_t seq_par(const ZkTree& t, int64_t i) {
  return t.seqno == nullptr || t.seqno[i] < 0 ? -1 : t.seqno[i] >> 32;
}

// CREATE (lib/zk-buffer.js:97-136 request shape; semantics of the server the
// reference talks to): parent must exist and not be ephemeral, ACL must be
// non-empty, SEQUENTIAL appends the parent's cversion, EPHEMERAL records the
// owning session in the Stat.  `v` (with storage `po` / `so`) was claimed
// for this lane in phase A; on failure the caller frees it.
ZK_DEV int32_t do_create(const ZkTree& t, Lane& L, const uint8_t* data,
                         int32_t nacl, int64_t session, int64_t now_ms,
                         int64_t v, int64_t i) {
  const ZkNodeStore& s = t.store;
  const bool eph = L.flags & CF_EPHEMERAL, seq = L.flags & CF_SEQUENTIAL;
  // a create the ordering pass numbered: the pass also counted it as its
  // parent's child (one atomic per parent a batch, not one per create); if
  // it fails, tree_serve_k takes the count back (seq_par)
  const int32_t pre = seq ? seq_num(t, i) : -1;
  if (nacl <= 0) return ERR_INVALID_ACL;
  if (v < 0) return ERR_SYSTEM;                       // tree full
  // node v's path and slot offsets, loaded before the parent lookup: their
  // round trip rides under it (a create is a chain of dependent trips)
  const int64_t vpo = t.node_path_off[v];
  const int64_t vso = s.slot_off[v];
  const uint8_t* path = L.path;
  const int32_t pl = L.pl;
  int32_t cut = pl - 1;
  while (cut > 0 && path[cut] != '/') --cut;
  const int64_t par = cut > 0 ? tree_find(t, path, cut) : -1;
  if (cut > 0 && par < 0) return ERR_NO_NODE;
  if (par >= 0 && t.eph[par] != 0)
    return ERR_NO_CHILDREN_FOR_EPHEMERALS;
  // (an existing path is found by tree_insert itself — it probes the same
  // chain and answers NODE_EXISTS before publishing anything — so the
  // usual, successful create walks the chain once, not twice; what this
  // lane wrote to its own node v before is freed by the caller)
  const int32_t npl = pl + (seq ? 10 : 0);
  // a SEQUENTIAL name: the number zk_tree_seq_order assigned it in stream
  // order (the parent's cversion at the batch's start + the request's rank
  // among the batch's sequential creates under that parent; the parent was
  // bumped once for all of them, and a failed create leaves a gap, never a
  // number handed back).  Without one (no ordering pass, or a parent the
  // pass did not find) the parent's cversion is taken here, bumped in the
  // same atomic as its child count — unique, but in arrival order.
  const bool taken = seq && par >= 0 && pre < 0;
  const int32_t seqno = !seq || par < 0 ? 0
                        : pre >= 0      ? pre
                                        : cn_cver(cn_add(t, par, 1, 1));
  uint8_t* pd = t.path_arena + vpo;
  copy_bytes(pd, path, pl);
  if (seq) put_seq10(pd + pl, seqno);
  const int32_t dl = L.dl;
  uint8_t* slot = s.slab + vso;
  fill_stat(slot, L.zx, L.zx, now_ms, now_ms, 0, 0, 0, eph ? session : 0, dl,
            0, L.zx);
  st_be32(slot + ZK_SLOT_LEN, dl > 0 ? dl : -1);
  copy_bytes(slot + ZK_SLOT_DATA, data, dl);
  t.node_path_len[v] = npl;
  s.data_len[v] = dl;
  t.cn[v] = 0;
  t.pzxid[v] = L.zx;
  t.node_parent[v] = par;
  t.node_pw[v] = pw_pack(pd - t.path_arena, npl);
  // No fence before publishing v in the hash: only a same-batch reader of
  // this very path could observe the half-written node (unordered by the
  // batch contract; every field it could read is in bounds), and the next
  // launch sees everything.  A __threadfence here is an XCD-L2 writeback
  // per wave (MI355X_MICROARCH.md: ~3.5 us each) and cost milliseconds.
  const int64_t ins = pre >= 0 ? tree_insert<true>(t, v, pd, npl, dl, vso)
                               : tree_insert(t, v, pd, npl, dl, vso);
  if (ins != v) {
    // the child was not made (the cversion it took stays: a gap)
    if (taken) cn_add(t, par, 0, -1);
    // (-1: the probe met no empty entry and no tombstone of this key — an
    // index full of other names' tombstones, cured by a rebuild; the name
    // itself does not exist)
    return ins < 0 ? ERR_SYSTEM : ERR_NODE_EXISTS;  // (or the timeout)
  }
  t.eph[v] = eph ? session : 0;
  if (par >= 0) {
    if (seq) {
      // (cversion and child count: taken above, or by the ordering pass)
      atomicMax((unsigned long long*)&t.pzxid[par], (unsigned long long)L.zx);
    } else {
      parent_touch(t, par, 1, true, L.zx);
    }
  }
  L.par = par;
  L.node = v;
  L.slot = s.slot_off[v];
  return ERR_OK;
}

// Apply one batch of decoded requests; produce reply descriptors for K13.
// r_path_off/len (may be null) receive the created node's path in the tree's
// path arena (SEQUENTIAL names differ from the requested one).  r_slot,
// r_sizes and r_bsum (may be null) receive each reply's slot offset, its
// frame size and the block's size sum, so the reply encoder needs neither
// its sizes pass nor a lookup of the node's slot (zk_encode_responses
// presized).
// PARSE: the requests come as K1 frames (foff / flen) and each lane parses
// its own in registers (zk_wire.h parse_request) instead of reading K12's SoA back —
// one launch and a 30 MB write + read less per 512K-request batch.
// RO: a batch of reads only (GET_DATA / EXISTS; the GET pipeline's): no
// node / storage claims, frees or dirty parents, so none of their five
// block-wide ticket barriers per workgroup; any other op is answered
// UNIMPLEMENTED.  (A run-time vote of the block for the same skip cost the
// create storm 10 %; a template costs the write batches nothing.)
// TILES (with PARSE): after a rows-deferred K1 scan of the request stream.
// The frame's row comes from the scan's tile lists T (zk_frame_rows.h)
// instead of the table; the workgroup also writes its rows to the table
// (rows_off / rows_len, what fs_rows would have written) and clears its
// share of the scan's flags.
// MS: a session batch (tree_sess.hip): the frames of several connections in
// one stream.  A live frame takes its session and watcher slot from its
// segment's row of the table M instead of the launch's scalars; when the
// table is unsound (*M.bad != 0) every request is answered SYSTEMERROR, and
// a request of a segment whose session is not alive SESSION_EXPIRED — both
// as the ordered passes refuse a request: nothing is looked up, claimed,
// written, armed or fired.
// (the kernels' own name for the launchers' ZkSegs, zk_abi.h)
struct ServeSegs : ZkSegs {};
// DEFER (MS only): the ordered serve with deferral (tree_order.hip
// ord_clip_mark_k).  A deferred frame comes with no segment and the rank byte
// ORD_RANK: it is refused like any frame of no segment, but the batch is not
// refused as a whole, so the numbers of its other SEQUENTIAL creates are in
// use and a deferred one leaves its gap in the parent's cversion.
static_assert(TR_T == FR_T, "a workgroup per block of FR_T frames");
// the read-only TILES instance's frame image: 64 requests of the benchmark
// (41 B bodies) are 2.9 KiB; a wave over 4 KiB reads global memory as ever
constexpr int SRV_STAGE = 4096;
template <bool PARSE, bool RO, bool TILES, bool MS = false, bool DEFER = false>
ZK_DEV void tree_serve_body(
    const ZkTree& t, const uint8_t* __restrict__ rx, const ZkReqOut& q,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap, int32_t* __restrict__ r_op,
    int32_t* __restrict__ r_xid, int32_t* __restrict__ r_err,
    int64_t* __restrict__ r_node, int64_t* __restrict__ r_zxid,
    int64_t* __restrict__ r_path_off, int32_t* __restrict__ r_path_len,
    int64_t* __restrict__ r_slot, int64_t* __restrict__ r_sizes,
    int64_t* __restrict__ r_bsum, int64_t session, int64_t now_ms,
    const uint8_t* __restrict__ rank, int32_t pass, int32_t last_pass,
    int64_t snap_base, int64_t snap_cap, int64_t* __restrict__ snap_top,
    int32_t wslot, int64_t* __restrict__ fired, const ZkFrameTiles* T,
    int64_t* __restrict__ rows_off, int32_t* __restrict__ rows_len,
    const ServeSegs* M = nullptr) {
  session = sess_of(t, session);
  const uint32_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t i = (int64_t)blk * TR_T + threadIdx.x;
  const bool in_batch = i < ncap && i < *n_dev;
  int64_t fo = 0;                    // the frame's row (TILES)
  int32_t fl = 0;
  // where this lane reads its frame's bytes: rxs + (a stream offset inside
  // the frame).  The read-only TILES instance (the GET pipeline's) stages the
  // wave's frames in LDS first (zk_frame_rows.h FrSpan) and parses, hashes
  // and compares the path there; offsets stay stream offsets.
  const uint8_t* rxs = rx;
  if (TILES) {
    __shared__ FrLds rows;
    const int64_t nf = *n_dev;
    const bool has = fr_row(*T, blk, nf < ncap ? nf : ncap, rows, fo, fl);
    if (has) {
      rows_off[i] = fo;
      rows_len[i] = fl;
    }
    fr_housekeep(*T);
    if constexpr (RO && TILES) {
      __shared__ __attribute__((aligned(16)))
          uint8_t img[TR_T / 64][fr_image_bytes<SRV_STAGE>()];
      uint8_t* im = img[threadIdx.x >> 6];
      const int lane = threadIdx.x & 63;
      const int64_t n = stream_len(T->n_dev, T->n_cap);
      FrSpan<SRV_STAGE> F;
      fr_span_load(rx, n, has, fo, fl, lane, F);
      int32_t rel;
      if (fr_span_store(rx, n, F, im, lane, fo, rel))
        rxs = (const uint8_t*)((uintptr_t)(const uint8_t*)im + rel - fo);
    }
  }
  // ordered passes: this launch serves the requests of rank `pass`; the
  // last pass also answers any of a higher rank, refused (SYSTEMERROR: more
  // same-path requests than passes).  rank bit 7: a later request of the
  // batch writes this path, so the reply's slot is snapshotted.
  const int32_t rb = rank != nullptr && in_batch ? (int32_t)rank[i] : 0;
  const int32_t rk = rb & ORD_RANK;
  const bool live = in_batch && (rk == pass || (last_pass && rk > pass));
  int32_t ms_err = ERR_OK;           // MS: the segment's refusal
  if (MS && live) {
    const int64_t sg = M->f_seg[i];
    if (*M->bad != 0 || sg < 0 || sg >= M->S) {
      ms_err = ERR_SYSTEM;
    } else {
      session = sess_of(t, M->sessions[sg]);
      wslot = M->wslots[sg];
      if (M->seg_state[sg] == 1) ms_err = ERR_SESSION_EXPIRED;
    }
  }
  const bool refused = live && (rk > pass || (MS && ms_err != ERR_OK));
  ReqFields rq{ST_BAD_DECODE, 0, OP_PING, 0, 0, 0, 0, -1, -1, -1, 0};
  if (live) {
    if (PARSE) {
      rq = TILES ? parse_request(rxs, fo, fl)
                 : parse_request(rx, foff[i], flen[i]);
    } else {
      rq.status = q.status[i];
      rq.xid = q.xid[i];
      rq.op = q.opcode[i];
      rq.arg = q.arg[i];
      rq.pl = q.path_len[i];
      rq.dl = q.data_len[i];
      rq.vc = q.vec_count[i];
      rq.poff = q.path_off[i];
      rq.doff = q.data_off[i];
    }
  }
  const bool ok_req = live && !refused && rq.status == ST_OK;
  const ZkNodeStore& s = t.store;
  Lane L;
  L.op = live ? rq.op : OP_PING;
  L.err = refused ? (MS && ms_err != ERR_OK ? ms_err : ERR_SYSTEM)
                  : (live && !ok_req ? ERR_BAD_ARGUMENTS : ERR_OK);
  L.node = -1;
  L.slot = -1;
  L.dlen = 0;
  L.par = -1;
  L.flags = 0;
  L.path = nullptr;
  L.pl = L.dl = 0;
  if (ok_req) {
    L.path = rxs + rq.poff;
    L.pl = rq.pl;
    L.dl = max(rq.dl, 0);
    L.flags = rq.arg;
  }
  // ---- phase A: wave-aggregated claims -----------------------------------
  // zxids without atomics: write i of the batch is txn base + i + 1, reads
  // see base; tree_publish_k advances the counter by the batch size.
  const bool write = ok_req && (L.op == OP_CREATE || L.op == OP_SET_DATA ||
                                L.op == OP_DELETE);
  const int64_t zbase = t.counters[TC_ZXID];
  L.zx = write ? zbase + i + 1 : zbase;
  const bool create = !RO && ok_req && L.op == OP_CREATE;
  int64_t v = -1;
  int32_t npl = 0, cap = 0;
  if (create) {
    npl = L.pl + ((L.flags & CF_SEQUENTIAL) ? 10 : 0);
    cap = max(L.dl, 128);
  }
  if (RO && ok_req && L.op != OP_GET_DATA && L.op != OP_EXISTS)
    L.err = ERR_UNIMPLEMENTED;
  if (!RO) {
    const int64_t pub = t.counters[TC_FREE_PUB];
    const int64_t h = block_ticket(&t.counters[TC_FREE_HEAD], create);
    if (create && h < pub) v = t.free_list[h % t.free_cap];
    const bool fresh = create && v < 0;
    const int64_t nv = block_ticket(&t.counters[TC_NODES], fresh);
    if (fresh && nv < s.cap) v = nv;
    // storage: reuse the recycled node's when it fits (path storage comes
    // in 16-byte multiples and keeps its capacity, so nodes recycled across
    // paths of a few lengths stop allocating: the arena is bounded by the
    // node count, not by the number of creates)
    const bool new_path = v >= 0 && (fresh || npl > t.node_path_cap[v]);
    const bool new_slot = v >= 0 && (fresh || cap > s.slot_cap[v]);
    const int32_t pcap = (npl + 15) & ~15;
    const int64_t po = wave_bytes(&t.counters[TC_PATH_TOP],
                                  new_path ? pcap : 0);
    const int64_t sb = new_slot ? slot_bytes(cap) : 0;
    const int64_t so = wave_bytes(&t.counters[TC_SLAB_TOP], sb);
    if (new_path) {
      if (po + pcap <= t.path_cap) {
        t.node_path_off[v] = po;
        t.node_path_len[v] = npl;
        t.node_path_cap[v] = pcap;
      } else {
        t.node_path_len[v] = 0;                     // storage-less free node
        t.node_path_cap[v] = 0;
      }
    }
    if (new_slot) {
      if (so + sb <= t.slab_cap) {
        s.slot_off[v] = so;
        s.slot_cap[v] = cap;
      } else {
        s.slot_cap[v] = -1;
      }
    }
    if (v >= 0 && ((new_path && po + pcap > t.path_cap) ||
                   (new_slot && so + sb > t.slab_cap))) {
      L.err = ERR_SYSTEM;                           // arena full
    }
  }
  // ---- phase B: the operation -------------------------------------------
  int64_t freed = -1;
  // a SEQUENTIAL create the ordering pass numbered (and counted as its
  // parent's child) that never reaches do_create — refused by the ordered
  // passes, or out of arena — takes that child back below
  // (the pass reads a frame's op, path and flags only: a frame it numbered
  // that the full parse refuses is taken back here too)
  bool numbered = !RO && live && seq_num(t, i) >= 0;
  if (ok_req && L.err == ERR_OK) {
    switch (L.op) {
      case OP_GET_DATA: case OP_EXISTS:
        {
          const Found f = tree_lookup<true>(t, L.path, L.pl);
          L.node = f.node;
          L.slot = f.slot;
          L.dlen = f.dlen;
        }
        if (L.node < 0) L.err = ERR_NO_NODE;
        break;
      case OP_SET_DATA: {
        const Found f = tree_lookup(t, L.path, L.pl);
        const int64_t node = f.node;
        if (node < 0) { L.err = ERR_NO_NODE; break; }
        L.slot = f.slot;
        if (L.dl > s.slot_cap[node]) { L.err = ERR_BAD_ARGUMENTS; break; }
        uint8_t* slot = s.slab + L.slot;
        unsigned int* ver = (unsigned int*)(slot + 32);
        const int32_t want = L.flags;
        unsigned int old = *ver, cmp;
        do {                                          // version CAS
          cmp = old;
          if (want != -1 && cmp != bswap32((uint32_t)want)) break;
          old = atomicCAS(ver, cmp, bswap32(bswap32(cmp) + 1));
        } while (old != cmp);
        if (old != cmp || (want != -1 && cmp != bswap32((uint32_t)want))) {
          L.err = ERR_BAD_VERSION;
          break;
        }
        copy_bytes(slot + ZK_SLOT_DATA, rx + rq.doff, L.dl);
        st_be32(slot + ZK_SLOT_LEN, L.dl > 0 ? L.dl : -1);
        s.data_len[node] = L.dl;
        ent_set_dlen(t, f.ent, L.dl);
        st_be64(slot + 8, L.zx);                      // mzxid
        st_be64(slot + 24, now_ms);                   // mtime
        st_be32(slot + 52, L.dl);                     // dataLength
        L.node = node;
        break;
      }
      case OP_CREATE:
        L.err = do_create(t, L, rx + rq.doff, rq.vc, session,
                          now_ms, v, i);
        if (L.err == ERR_OK) numbered = false;      // the child is made
        if (L.err == ERR_OK && r_path_off != nullptr) {
          r_path_off[i] = t.node_path_off[v];
          r_path_len[i] = t.node_path_len[v];
        }
        break;
      case OP_DELETE: {
        const Found f = tree_lookup(t, L.path, L.pl);
        const int64_t node = f.node, so = f.slot;
        if (node < 0) { L.err = ERR_NO_NODE; break; }
        // the version before the children, as ZooKeeper checks them (a
        // stale delete of a parent with children is BAD_VERSION)
        const int32_t nkids = cn_nchild(__hip_atomic_load(
            &t.cn[node], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const int32_t want = L.flags;
        if (want != -1 && ld_be32(s.slab + so + 32) != want) {
          L.err = ERR_BAD_VERSION;
          break;
        }
        if (nkids > 0) {
          L.err = ERR_NOT_EMPTY;
          break;
        }
        if (!tree_erase_at(t, f.ent, node)) { L.err = ERR_NO_NODE; break; }
        L.par = t.node_parent[node];
        if (L.par >= 0) parent_touch(t, L.par, -1, true, L.zx);
        t.eph[node] = 0;
        freed = node;
        break;
      }
      case OP_SYNC: case OP_PING:
        break;
      case OP_SET_WATCHES:
        // header-only reply; the catch-up (notifications for what changed
        // after relZxid, re-registration of the rest) is zk_watch_resume
        break;
      default:
        L.err = ERR_UNIMPLEMENTED;
    }
  }
  // (MS, the whole batch refused: no number of the ordering pass's bump was
  // used, so the parent's cversion goes back with the child)
  if (numbered)
    cn_add(t, seq_par(t, i),
           MS && ms_err == ERR_SYSTEM && !(DEFER && rk == ORD_RANK) ? -1 : 0,
           -1);
  // ---- watches: reads with watch=1 arm (this session's slot), successful
  // writes fire (lib/zk-session.js:558-574 is the client side of the
  // trigger table; the server rules are SURVEY Appendix D)
  if (t.wt_key != nullptr && ok_req) {
    const bool wflag = rq.arg == 1;
    if (L.op == OP_GET_DATA && wflag && L.err == ERR_OK) {
      wt_arm(t, L.path, L.pl, WK_DATA, wslot);
    } else if (L.op == OP_EXISTS && wflag &&
               (L.err == ERR_OK || L.err == ERR_NO_NODE)) {
      wt_arm(t, L.path, L.pl, WK_DATA, wslot);
    } else if (L.err == ERR_OK && (L.op == OP_SET_DATA ||
                                   L.op == OP_CREATE ||
                                   L.op == OP_DELETE)) {
      const int64_t node = L.op == OP_DELETE ? freed : L.node;
      const int64_t pw = t.node_pw[node];
      const int64_t ppw = L.par >= 0 ? t.node_pw[L.par] : 0;
      const uint8_t* np = node_path(t, pw);
      const int32_t nl = pw_len(pw);
      uint64_t m0 = wt_fire(t, np, nl, WK_DATA), m1 = 0, m2 = 0;
      if (L.op == OP_DELETE) m1 = wt_fire(t, np, nl, WK_CHILD) & ~m0;
      if (L.op != OP_SET_DATA && L.par >= 0)
        m2 = wt_fire(t, node_path(t, ppw), pw_len(ppw), WK_CHILD);
      if (fired != nullptr) {
        int64_t* f = fired + (int64_t)WT_REC * i;
        f[0] = (int64_t)m0;
        f[1] = (int64_t)m1;
        f[2] = (int64_t)m2;
        f[3] = pw;
        f[4] = ppw;
      }
    }
  }
  // ---- ordered snapshot: a reply that reads the node's slot (stat, data)
  // while a later pass of this batch writes the node reads a private copy
  // in the slab's scratch tail, taken now (wave-aggregated claim)
  if (rank != nullptr) {
    const bool snap = (rb & ORD_SNAP) && live && L.err == ERR_OK &&
                      (L.op == OP_GET_DATA || L.op == OP_EXISTS ||
                       L.op == OP_SET_DATA);
    const int64_t dl = snap && L.op == OP_GET_DATA ? L.dlen : 0;
    const int64_t sb = snap ? slot_bytes((int32_t)dl) : 0;
    const int64_t so = wave_bytes(snap_top, sb);
    if (snap) {
      if (so + sb <= snap_cap) {
        copy_bytes(s.slab + snap_base + so, s.slab + L.slot,
                   (int32_t)(ZK_SLOT_DATA + dl));
        L.slot = snap_base + so;
      } else {
        L.err = ERR_SYSTEM;              // scratch full (counted by caller)
      }
    }
  }
  // ---- phase C: wave-aggregated frees and dirty parents -----------------
  if (create && L.err != ERR_OK && v >= 0) freed = v;  // return the claim
  // (A read-only block could skip these claims, but guarding them with a
  // block vote cost the create storm 10% in measurement; they stay, except
  // in the RO instance.)
  if (!RO) {
    wave_free(t, freed);
    // (DEFER: a numbered create that was not made has moved its parent's
    // child count in a pass of its own — the last, for a deferred frame — so
    // the parent's Stat is written again behind it)
    wave_mark_dirty(t, L.err == ERR_OK ? L.par
                       : DEFER && numbered ? seq_par(t, i) : -1);
  }
  if (r_sizes != nullptr) {                       // block-uniform
    __shared__ int64_t sm[TR_T / 64 + 1];
    int64_t sz = 0;
    if (live) {
      const bool get = L.err == ERR_OK && L.op == OP_GET_DATA;
      const bool mk = L.err == ERR_OK && L.op == OP_CREATE;
      sz = served_reply_size(L.op, L.err, get ? L.dlen : 0,
                             mk ? t.node_path_len[L.node] : 0);
      r_sizes[i] = sz;
    } else if (in_batch && rk < pass) {
      sz = r_sizes[i];                  // served by an earlier pass
    } else if (!in_batch && i < ncap) {
      r_sizes[i] = 0;
    }
    int64_t tot;
    block_excl_scan(sz, sm, &tot);
    if (threadIdx.x == 0) r_bsum[blk] = tot;
  }
  if (!live) return;
  r_op[i] = L.op;
  r_xid[i] = rq.xid;
  r_err[i] = L.err;
  r_node[i] = L.op == OP_DELETE ? -1 : L.node;
  r_zxid[i] = L.zx;
  if (r_slot != nullptr) r_slot[i] = L.op == OP_DELETE ? -1 : L.slot;
}

template <bool PARSE, bool RO = false>
__global__ __launch_bounds__(TR_T) void tree_serve_k(
    ZkTree t, const uint8_t* __restrict__ rx, ZkReqOut q,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap, int32_t* __restrict__ r_op,
    int32_t* __restrict__ r_xid, int32_t* __restrict__ r_err,
    int64_t* __restrict__ r_node, int64_t* __restrict__ r_zxid,
    int64_t* __restrict__ r_path_off, int32_t* __restrict__ r_path_len,
    int64_t* __restrict__ r_slot, int64_t* __restrict__ r_sizes,
    int64_t* __restrict__ r_bsum, int64_t session, int64_t now_ms,
    const uint8_t* __restrict__ rank, int32_t pass, int32_t last_pass,
    int64_t snap_base, int64_t snap_cap, int64_t* __restrict__ snap_top,
    int32_t wslot, int64_t* __restrict__ fired) {
  tree_serve_body<PARSE, RO, false>(
      t, rx, q, foff, flen, n_dev, ncap, r_op, r_xid, r_err, r_node, r_zxid,
      r_path_off, r_path_len, r_slot, r_sizes, r_bsum, session, now_ms, rank,
      pass, last_pass, snap_base, snap_cap, snap_top, wslot, fired, nullptr,
      nullptr, nullptr);
}

// The parsing serve over a rows-deferred scan's tile lists (one pass: no
// ranks, no snapshots).
template <bool RO>
__global__ __launch_bounds__(TR_T) void tree_serve_tiles_k(
    ZkTree t, ZkFrameTiles T, int64_t* __restrict__ rows_off,
    int32_t* __restrict__ rows_len, const int64_t* __restrict__ n_dev,
    int64_t ncap, ZkServeOut o, int64_t session, int64_t now_ms,
    int32_t wslot, int64_t* __restrict__ fired) {
  tree_serve_body<true, RO, true>(
      t, T.buf, ZkReqOut{}, nullptr, nullptr, n_dev, ncap, o.opcode, o.xid,
      o.err, o.node, o.zxid, o.path_off, o.path_len, o.slot, o.sizes,
      o.block_sums, session, now_ms, nullptr, 0, 1, 0, 0, nullptr, wslot,
      fired, &T, rows_off, rows_len);
}

// The serve of a session batch (MS; the plain and the ordered passes' form).
template <bool PARSE>
__global__ __launch_bounds__(TR_T) void tree_serve_sess_k(
    ZkTree t, const uint8_t* __restrict__ rx, ZkReqOut q,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap, ZkServeOut o,
    int64_t now_ms, const uint8_t* __restrict__ rank, int32_t pass,
    int32_t last_pass, int64_t snap_base, int64_t snap_cap,
    int64_t* __restrict__ snap_top, int64_t* __restrict__ fired,
    ServeSegs M) {
  tree_serve_body<PARSE, false, false, true>(
      t, rx, q, foff, flen, n_dev, ncap, o.opcode, o.xid, o.err, o.node,
      o.zxid, o.path_off, o.path_len, o.slot, o.sizes, o.block_sums, 0,
      now_ms, rank, pass, last_pass, snap_base, snap_cap, snap_top, -1, fired,
      nullptr, nullptr, nullptr, &M);
}

// The ordered passes of a session batch served with deferral (DEFER; K12's
// table only).
__global__ __launch_bounds__(TR_T) void tree_serve_sess_defer_k(
    ZkTree t, const uint8_t* __restrict__ rx, ZkReqOut q,
    const int64_t* __restrict__ n_dev, int64_t ncap, ZkServeOut o,
    int64_t now_ms, const uint8_t* __restrict__ rank, int32_t pass,
    int32_t last_pass, int64_t snap_base, int64_t snap_cap,
    int64_t* __restrict__ snap_top, int64_t* __restrict__ fired,
    ServeSegs M) {
  tree_serve_body<false, false, false, true, true>(
      t, rx, q, nullptr, nullptr, n_dev, ncap, o.opcode, o.xid, o.err, o.node,
      o.zxid, o.path_off, o.path_len, o.slot, o.sizes, o.block_sums, 0,
      now_ms, rank, pass, last_pass, snap_base, snap_cap, snap_top, -1, fired,
      nullptr, nullptr, nullptr, &M);
}

// The one launch site of tree_serve_k (zk_tree.h ServeLaunch): its
// <false, false>, <true, false> and <true, true> instances, and the two of
// tree_serve_tiles_k.
int serve_launch(const ServeLaunch& s, hipStream_t st) {
  if (s.ncap <= 0) return 0;
  const ZkServeOut& o = *s.out;
  if ((o.sizes == nullptr) != (o.block_sums == nullptr)) return -1;
  if (s.tiles != nullptr) {
    // after a rows-deferred scan: the frame table receives the rows
    if (s.q != nullptr || s.rank != nullptr || s.segs != nullptr) return -1;
    const auto kt = s.read_only ? tree_serve_tiles_k<true>
                                : tree_serve_tiles_k<false>;
    kt<<<(unsigned)((s.ncap + TR_T - 1) / TR_T), TR_T, 0, st>>>(
        *s.tree, *s.tiles, s.rows_off, s.rows_len, s.n_dev, s.ncap, o,
        s.session, s.now_ms, s.wslot, s.fired);
    ZK_LAUNCH_CHECK();
    return 0;
  }
  const bool parse = s.q == nullptr;
  if (s.segs != nullptr) {
    // a session batch: the MS instances (none read-only, none over tiles)
    const ServeSegs M{*s.segs};
    if (s.read_only || M.f_seg == nullptr || M.sessions == nullptr ||
        M.wslots == nullptr || M.seg_state == nullptr || M.bad == nullptr ||
        M.S < 1)
      return -1;
    if (s.defer) {
      if (parse || s.rank == nullptr) return -1;
      tree_serve_sess_defer_k<<<(unsigned)((s.ncap + TR_T - 1) / TR_T), TR_T,
                                0, st>>>(
          *s.tree, s.rx, *s.q, s.n_dev, s.ncap, o, s.now_ms, s.rank, s.pass,
          s.last_pass, s.snap_base, s.snap_cap, s.snap_top, s.fired, M);
      ZK_LAUNCH_CHECK();
      return 0;
    }
    const auto km = parse ? tree_serve_sess_k<true> : tree_serve_sess_k<false>;
    km<<<(unsigned)((s.ncap + TR_T - 1) / TR_T), TR_T, 0, st>>>(
        *s.tree, s.rx, parse ? ZkReqOut{} : *s.q, s.foff, s.flen, s.n_dev,
        s.ncap, o, s.now_ms, s.rank, s.pass, s.last_pass, s.snap_base,
        s.snap_cap, s.snap_top, s.fired, M);
    ZK_LAUNCH_CHECK();
    return 0;
  }
  const auto k = !parse        ? tree_serve_k<false>
                 : s.read_only ? tree_serve_k<true, true>
                               : tree_serve_k<true>;
  k<<<(unsigned)((s.ncap + TR_T - 1) / TR_T), TR_T, 0, st>>>(
      *s.tree, s.rx, parse ? ZkReqOut{} : *s.q, s.foff, s.flen, s.n_dev,
      s.ncap, o.opcode, o.xid, o.err, o.node, o.zxid, o.path_off, o.path_len,
      o.slot, o.sizes, o.block_sums, s.session, s.now_ms, s.rank, s.pass,
      s.last_pass, s.snap_base, s.snap_cap, s.snap_top, s.wslot, s.fired);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // namespace zk

extern "C" {

// The unordered serve of K12's decoded requests + its finish.
int zk_tree_serve(const ZkTree* t, const uint8_t* rx, const ZkReqOut* q,
                  const int64_t* n_dev, int64_t ncap, const ZkServeOut* out,
                  int64_t session, int64_t now_ms, hipStream_t st) {
  if (ncap <= 0) return 0;
  zk::ServeLaunch s;
  s.tree = t, s.rx = rx, s.q = q, s.n_dev = n_dev, s.ncap = ncap;
  s.out = out, s.session = session, s.now_ms = now_ms;
  const int rc = zk::serve_launch(s, st);
  // at most one dirty parent per request
  return rc ? rc : zk::finish_launch(t, n_dev, 0, 1, st);
}

// zk_tree_serve straight from K1's frame table (foff / flen, *n_dev
// frames): every lane parses its request in registers (no K12 pass).
// wslot: this session's watcher slot (-1: its reads arm no watch); fired
// (may be null; [ncap * 5]): per successful write, the watcher masks it
// fired and the paths (zk_watch_events expands them).
// read_only: a batch of GET_DATA / EXISTS only (tree_serve_k's RO instance).
// No finish: the caller launches zk_tree_finish_scan next.
int zk_tree_serve_frames(const ZkTree* t, const uint8_t* rx,
                         const int64_t* foff, const int32_t* flen,
                         const int64_t* n_dev, int64_t ncap,
                         const ZkServeOut* out, int64_t session,
                         int64_t now_ms, int32_t wslot, int64_t* fired,
                         int32_t read_only, hipStream_t st) {
  zk::ServeLaunch s;
  s.tree = t, s.rx = rx, s.foff = foff, s.flen = flen, s.n_dev = n_dev;
  s.ncap = ncap, s.out = out, s.session = session, s.now_ms = now_ms;
  s.wslot = wslot, s.fired = fired, s.read_only = read_only;
  return zk::serve_launch(s, st);
}

// zk_tree_serve_frames for a session batch: session and watcher slot per
// segment (segs: ZkSegs).  No finish, like zk_tree_serve_frames.
int zk_tree_serve_frames_sessions(
    const ZkTree* t, const uint8_t* rx, const int64_t* foff,
    const int32_t* flen, const int64_t* n_dev, int64_t ncap,
    const ZkServeOut* out, int64_t now_ms, int64_t* fired, const ZkSegs* segs,
    hipStream_t st) {
  if (segs == nullptr) return (int)hipErrorInvalidValue;
  zk::ServeLaunch s;
  s.tree = t, s.rx = rx, s.foff = foff, s.flen = flen, s.n_dev = n_dev;
  s.ncap = ncap, s.out = out, s.now_ms = now_ms, s.fired = fired;
  s.segs = segs;
  return zk::serve_launch(s, st);
}

// zk_tree_serve_frames after a rows-deferred scan of the request stream
// (zk_frame_scan flags bit 24): the rows come from the scan's tile lists;
// foff / flen [ncap] receive them and the scan's workspace is left clean.
int zk_tree_serve_tiles(const ZkTree* t, const ZkFrameTiles* tiles,
                        int64_t* foff, int32_t* flen, const int64_t* n_dev,
                        int64_t ncap, const ZkServeOut* out, int64_t session,
                        int64_t now_ms, int32_t wslot, int64_t* fired,
                        int32_t read_only, hipStream_t st) {
  if (ncap <= 0) return (int)hipErrorInvalidValue;  // (the flags stay set)
  zk::ServeLaunch s;
  s.tree = t, s.rx = tiles->buf, s.tiles = tiles, s.rows_off = foff;
  s.rows_len = flen, s.n_dev = n_dev, s.ncap = ncap, s.out = out;
  s.session = session, s.now_ms = now_ms, s.wslot = wslot, s.fired = fired;
  s.read_only = read_only;
  return zk::serve_launch(s, st);
}

}  // extern "C"

namespace zk {

// After a serve / expire launch, one kernel:
//  1. rewrite the wire-format Stat words of every dirty parent from the
//     shadows;
//  2. then (thread 0, after a barrier) publish: make the nodes freed by the
//     launch poppable, clamp a head that overshot the previously published
//     tail, reset the dirty list and consume the launch's zxids (`*n_dev`
//     for a batch of requests, 1 for a session expiry, which is one
//     closeSession txn).
constexpr int FIN_T = 1024;

// One workgroup: the dirty list holds the distinct parents a batch touched
// (a few thousand at most in practice), and a single block needs no
// cross-block sign-off — the grid version's atomic sign-off counter took
// 15-60 us per launch on a read-only GET batch, and two streams finishing
// at once could interleave on it.
// The finish (see above) by the calling workgroup (blockDim.x threads).
// The counters and parent shadows other workgroups updated are read with
// agent-scope loads (this workgroup's L1 may hold older lines).
ZK_DEV void finish_body(const ZkTree& t, const int64_t* n_dev,
                        int64_t bump_zxid, int32_t publish) {
  int64_t* c = t.counters;
  const int64_t nd = __hip_atomic_load(&c[TC_DIRTY], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  for (int64_t k = threadIdx.x; k < nd; k += blockDim.x) {
    const int64_t p = __hip_atomic_load(&t.dirty_list[k], __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
    uint8_t* slot = t.store.slab + t.store.slot_off[p];
    const int64_t cn = __hip_atomic_load(&t.cn[p], __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    st_be32(slot + 36, cn_cver(cn));
    st_be32(slot + 56, cn_nchild(cn));
    st_be64(slot + 60, __hip_atomic_load(&t.pzxid[p], __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT));
    t.dirty[p] = 0;
  }
  __syncthreads();                 // every thread has read TC_DIRTY
  if (threadIdx.x != 0) return;
  auto ld = [&](int k) {
    return __hip_atomic_load(&c[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  if (publish) {
    if (ld(TC_FREE_HEAD) > ld(TC_FREE_PUB)) c[TC_FREE_HEAD] = ld(TC_FREE_PUB);
    c[TC_FREE_PUB] = ld(TC_FREE_TAIL);
  }
  c[TC_DIRTY] = 0;
  c[TC_ZXID] = ld(TC_ZXID) + (n_dev != nullptr ? *n_dev : bump_zxid);
}

template <int NT = FIN_T>
__global__ __launch_bounds__(NT) void tree_finish_k(ZkTree t,
                                                   const int64_t* n_dev,
                                                   int64_t bump_zxid,
                                                   int32_t publish) {
  finish_body(t, n_dev, bump_zxid, publish);
}

// The between-batch finish and the reply encoder's block-sum scan in ONE
// launch of two workgroups: they are independent one-workgroup jobs that
// ran back to back on the connection's stream (tree_finish_k, then K13's
// scan_one_block), each waiting for a CU behind the other connection's
// kernels.  Workgroup 1 scans the serve's per-256-reply size sums (bsum,
// nb of them) into the encoder's block bases and writes the stream total
// (zk_encode_responses `presized` 2).
template <int NT>
__global__ __launch_bounds__(NT) void tree_finish_scan_k(
    ZkTree t, const int64_t* n_dev, int64_t bump_zxid, int32_t publish,
    const int64_t* __restrict__ bsum, int64_t nb, int64_t* __restrict__ bbase,
    int64_t* __restrict__ total) {
  if (blockIdx.x == 0) {
    finish_body(t, n_dev, bump_zxid, publish);
    return;
  }
  // a thread owns FS_V consecutive sums, so a 512K-reply connection's 2048
  // are one block scan (one value a thread per chunk took eight: 9.9 us
  // against scan_one_block's 4.2, profiles/r6_get_pmc.md)
  constexpr int FS_V = 8;
  __shared__ int64_t sm[NT / 64 + 1];
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < nb; c0 += (int64_t)NT * FS_V) {   // (uniform)
    const int64_t b = c0 + (int64_t)threadIdx.x * FS_V;
    int64_t v[FS_V];
    int64_t s = 0;
#pragma unroll
    for (int j = 0; j < FS_V; ++j) {
      v[j] = b + j < nb ? bsum[b + j] : 0;
      s += v[j];
    }
    int64_t tot;
    int64_t p = carry + block_excl_scan(s, sm, &tot);
#pragma unroll
    for (int j = 0; j < FS_V; ++j) {
      if (b + j < nb) bbase[b + j] = p;
      p += v[j];
    }
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

// Session expiry: remove every ephemeral node owned by `session`
// (lib/zk-session.js expiry; the server side deletes the session's
// ephemerals as ONE closeSession txn: all removals share zxid + 1).  One
// pass over the node table; `removed` counts deletions.
// DBG: phase clocks into dbg (zk_tree_expire_debug), 100 MHz ticks — an
// instance of its own: the clock reads in the plain kernel, even behind a
// null test, took the expiry from ~0.45 to ~1 ms.
//
// WT: the instance for a tree with a watch table (chosen on the host by
// wt_key != nullptr).  Every removed node fires what a DELETE fires — its
// data mask, its child mask (a watcher in both is told once) and its
// parent's child mask — and a removal that fired anything appends one
// compact record (WT_REC words, the serve's `fired` layout) at rec + 8;
// rec[0] counts the records wanted, rec_cap is the room (records past it
// are dropped: the caller compares the two).  zk_watch_events expands them as
// it does a batch's.  The plain instance is a kernel of its own and comes
// out as before (same registers, LDS and code size).  The same fire behind
// a run-time null test of wt_key took the plain kernel from 40 to 46 VGPRs,
// 76 to 88 SGPRs and 4708 to 6880 bytes of code (occupancy 8 either way;
// the resource table, not timed — the phase clocks above are why a test
// that costs nothing on paper is not trusted in this kernel).
template <bool DBG, bool WT>
ZK_DEV void tree_expire_body(
    const ZkTree& t, int64_t session, int64_t ncap,
    unsigned long long* __restrict__ removed, int32_t* __restrict__ dbg,
    int64_t* __restrict__ rec, int64_t rec_cap) {
  session = sess_of(t, session);
  const int64_t v = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const int64_t c0 = DBG ? (int64_t)wall_clock64() : 0;
  int64_t c1 = 0, c2 = 0;
  // the owner from the contiguous shadow (a node's slab line per node was
  // 256 MB of random reads over a 4M-node tree, 335 us an expiry); a
  // freed node's shadow is 0.  The slab's ephemeralOwner of a freed node is
  // left as it was: nothing reads a freed slot, and the create that reuses
  // it writes the whole Stat (fill_stat) — zeroing it was one random slab
  // line written back per removal (256 MB an expiry of 2M nodes)
  bool hit = v < ncap && v < t.counters[TC_NODES] && t.eph[v] == session;
  const int64_t zx = t.counters[TC_ZXID] + 1;
  int64_t par = -1;
  int32_t dflag = 1;
  if (hit) {
    // what the removal reads of node v, at once: its path, its parent and
    // the parent's dirty flag (their round trips ride under the probe's:
    // the thread is a chain of dependent trips to memory; pairing the
    // probe's loads took the storm step 1.298 -> 1.262 ms, these measured
    // within noise)
    const int64_t poff = t.node_path_off[v];
    const int32_t plen = t.node_path_len[v];
    const int64_t p0 = t.node_parent[v];
    if (p0 >= 0)
      dflag = __hip_atomic_load(&t.dirty[p0], __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
    const int64_t tag = tomb_tag(zx);
    const int64_t es = tree_erase_slot(t, v, t.path_arena + poff, plen, tag);
    hit = es >= 0;
    if (DBG) c1 = (int64_t)wall_clock64();
    if (hit) {
      ht_shift(t, es, session, tag);
      if (DBG) c2 = (int64_t)wall_clock64();
      par = p0;
      if (par >= 0) parent_touch(t, par, -1, true, zx);
      t.eph[v] = 0;
      if (WT) {
        const int64_t ws = wt_find(t, t.path_arena + poff, plen);
        const uint64_t m0 = wt_fire_at(t, ws, WK_DATA);
        const uint64_t m1 = wt_fire_at(t, ws, WK_CHILD) & ~m0;
        const int64_t ppw = par >= 0 ? t.node_pw[par] : 0;
        const uint64_t m2 =
            par >= 0 ? wt_fire(t, node_path(t, ppw), pw_len(ppw), WK_CHILD)
                     : 0;
        if ((m0 | m1 | m2) != 0 && rec != nullptr) {
          const int64_t k = (int64_t)atomicAdd((unsigned long long*)&rec[0],
                                               1ull);
          if (k < rec_cap) {
            int64_t* f = rec + 8 + (int64_t)WT_REC * k;
            f[0] = (int64_t)m0;
            f[1] = (int64_t)m1;
            f[2] = (int64_t)m2;
            f[3] = pw_pack(poff, plen);
            f[4] = ppw;
          }
        }
      }
    }
  }
  // the frees' ticket also counts `removed` (no second block round)
  wave_free(t, hit ? v : -1, removed);
  wave_mark_dirty_at(t, par, dflag);
  if (DBG && hit) {
    // start (low word), lookup + tombstone, backward shift, whole thread
    const int64_t c3 = (int64_t)wall_clock64();
    dbg[4 * v] = (int32_t)c0;
    dbg[4 * v + 1] = (int32_t)(c1 - c0);
    dbg[4 * v + 2] = (int32_t)(c2 - c1);
    dbg[4 * v + 3] = (int32_t)(c3 - c0);
  }
}

template <bool DBG>
__global__ __launch_bounds__(TR_T) void tree_expire_k(
    ZkTree t, int64_t session, int64_t ncap,
    unsigned long long* __restrict__ removed, int32_t* __restrict__ dbg) {
  tree_expire_body<DBG, false>(t, session, ncap, removed, dbg, nullptr, 0);
}

__global__ __launch_bounds__(TR_T) void tree_expire_wt_k(
    ZkTree t, int64_t session, int64_t ncap,
    unsigned long long* __restrict__ removed, int64_t* __restrict__ rec,
    int64_t rec_cap) {
  tree_expire_body<false, true>(t, session, ncap, removed, nullptr, rec,
                                rec_cap);
}

int finish_launch(const ZkTree* t, const int64_t* n_dev, int64_t bump,
                  int32_t publish, hipStream_t st) {
  // (256 threads: the workgroup finds a CU sooner behind another stream's
  // kernel than 1024 did, and the dirty list is a few thousand entries)
  tree_finish_k<256><<<1, 256, 0, st>>>(*t, n_dev, bump, publish);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // namespace zk

extern "C" {

// The between-batch finish of a serve (parent Stat fix-up, free-ring
// publish, zxid += *n_dev or bump), the partner of zk_tree_serve_frames, +
// the presized reply encode's block-sum scan (the serve's r_bsum for ncap
// replies, in scan_ws[0, nb)) -> scan_ws[nb, 2 nb) and *total, in one launch
// (tree_finish_scan_k).
int zk_tree_finish_scan(const ZkTree* t, const int64_t* n_dev, int64_t bump,
                        int32_t publish, int64_t ncap, int64_t* scan_ws,
                        int64_t* total, hipStream_t st) {
  const int64_t nb = ncap > 0 ? (ncap + 255) / 256 : 0;
  zk::tree_finish_scan_k<256><<<2, 256, 0, st>>>(
      *t, n_dev, bump, publish, scan_ws, nb, scan_ws + nb, total);
  ZK_LAUNCH_CHECK();
  return 0;
}

static int32_t* g_exp_dbg = nullptr;
void zk_tree_expire_debug(int32_t* buf) { g_exp_dbg = buf; }

// rec (a tree with a watch table; may be null: the fired masks are then
// consumed without a record): [0] records wanted (zeroed by the caller),
// [8 + WT_REC * k) record k < rec_cap.
int zk_tree_expire(const ZkTree* t, int64_t session, int64_t ncap,
                   unsigned long long* removed, int64_t* rec, int64_t rec_cap,
                   hipStream_t st) {
  if (ncap <= 0) return 0;
  const unsigned nb = (unsigned)((ncap + zk::TR_T - 1) / zk::TR_T);
  if (t->wt_key != nullptr)
    zk::tree_expire_wt_k<<<nb, zk::TR_T, 0, st>>>(*t, session, ncap, removed,
                                                  rec, rec_cap);
  else if (g_exp_dbg != nullptr)
    zk::tree_expire_k<true><<<nb, zk::TR_T, 0, st>>>(*t, session, ncap, removed,
                                                     g_exp_dbg);
  else
    zk::tree_expire_k<false><<<nb, zk::TR_T, 0, st>>>(*t, session, ncap,
                                                      removed, nullptr);
  ZK_LAUNCH_CHECK();
  return zk::finish_launch(t, nullptr, 1, 1, st);
}

}  // extern "C"

namespace zk {

// ---- tree digest (tests / replica checks) ----------------------------------
// Sum over live nodes of a hash of (path, czxid, mzxid, version, cversion |
// numChildren, pzxid, ephemeralOwner, data): equal on two trees that hold
// the same znodes with the same Stat (times aside) and data, whatever node
// slots and hash entries they sit in.
ZK_DEV uint64_t wave_sum_u64(uint64_t x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

__global__ __launch_bounds__(TR_T) void tree_digest_k(
    ZkTree t, unsigned long long* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const int64_t nn = min(t.counters[TC_NODES], t.store.cap);
  uint64_t h = 0, live = 0;
  if (v < nn && t.node_parent[v] != NODE_FREE) {
    const int64_t pw = t.node_pw[v];
    const uint8_t* slot = t.store.slab + t.store.slot_off[v];
    const int32_t dl = t.store.data_len[v];
    h = path_hash(node_path(t, pw), pw_len(pw));
    auto mix = [&](uint64_t x) {
      h = (h ^ x) * 0x9E3779B97F4A7C15ull;
      h ^= h >> 29;
    };
    mix((uint64_t)ld_be64(slot));                  // czxid
    mix((uint64_t)ld_be64(slot + 8));              // mzxid
    mix((uint32_t)ld_be32(slot + 32));             // version
    mix((uint64_t)t.cn[v]);
    mix((uint64_t)t.pzxid[v]);
    mix((uint64_t)t.eph[v]);
    mix((uint64_t)(uint32_t)dl);
    mix(path_hash(slot + ZK_SLOT_DATA, max(dl, 0)));
    live = 1;
  }
  h = wave_sum_u64(h);
  live = wave_sum_u64(live);
  if ((threadIdx.x & 63) == 0 && live) {
    atomicAdd(&out[0], (unsigned long long)h);
    atomicAdd(&out[1], (unsigned long long)live);
  }
}

__global__ __launch_bounds__(TR_T) void ht_census_k(
    ZkTree t, unsigned long long* __restrict__ out) {
  uint64_t used = 0, tomb = 0;
  for (int64_t s = (int64_t)blockIdx.x * TR_T + threadIdx.x; s <= t.mask;
       s += (int64_t)gridDim.x * TR_T) {
    if (*ht_key(t, s) != 0) {
      ++used;
      if (val_tomb(*ht_val(t, s))) ++tomb;
    }
  }
  used = wave_sum_u64(used);
  tomb = wave_sum_u64(tomb);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&out[2], (unsigned long long)used);
    atomicAdd(&out[3], (unsigned long long)tomb);
  }
}

int digest_launch(const ZkTree* t, unsigned long long* out, hipStream_t st) {
  const int64_t nb = (t->store.cap + TR_T - 1) / TR_T;
  if (nb <= 0) return 0;
  tree_digest_k<<<(unsigned)nb, TR_T, 0, st>>>(*t, out);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // namespace zk

extern "C" {

// out[4] (zeroed here): node digest sum, live nodes, hash entries in use,
// tombstones (zk_abi.h).
int zk_tree_digest(const ZkTree* t, unsigned long long* out, hipStream_t st) {
  if (hipMemsetAsync(out, 0, 32, st) != hipSuccess) return -4;
  const int64_t nb = (t->store.cap + zk::TR_T - 1) / zk::TR_T;
  if (nb > 0) {
    zk::tree_digest_k<<<(unsigned)nb, zk::TR_T, 0, st>>>(*t, out);
    ZK_LAUNCH_CHECK();
  }
  zk::ht_census_k<<<2048, zk::TR_T, 0, st>>>(*t, out);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
