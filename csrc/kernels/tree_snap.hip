// The GPU tree's image: snapshot of the live znodes into one compact,
// position-independent byte image, and the load of such an image into a
// fresh, empty tree of any capacity (the layout and its checks: zk_snap.h;
// the tree: zk_tree.h).  Snapshot followed by load is the tree's compaction
// and its regrow, and the image is what a replica would be sent.  Watches
// and the session table are not part of an image.
//
// Both run between batches on the caller's stream as plain launches: a
// kernel boundary is the only cross-workgroup synchronisation, offsets come
// from the device-wide scan (zk_scan_excl_i64), no lane waits for another
// lane's store (the index build's tree_insert aside, which is the serve's).
#include "zk_acl.h"
#include "zk_snap.h"

namespace zk {

// ZooKeeper's open ACL in wire format: what a tree without an ACL table
// writes for every node (count 1; perms 31, "world", "anyone")
__device__ const uint8_t SNAP_OPEN_ACL[SNAP_OPEN_ACL_BYTES] = {
    0, 0, 0, 1, 0, 0, 0, 31, 0, 0, 0, 5, 'w', 'o', 'r', 'l', 'd',
    0, 0, 0, 6, 'a', 'n', 'y', 'o', 'n', 'e'};

// The writer's tiers by padded record bytes: up to SNAP_SMALL a group of
// SNAP_GROUP lanes per record (a wave stores one contiguous span of 8
// records), above it a wave per record.
constexpr int SNAP_GROUP = 8;
constexpr int64_t SNAP_SMALL = 512;
// the Stat's bytes before cversion (czxid .. version): the slot's, as they are
constexpr int32_t SNAP_STAT_HEAD = 36;

// scalars of a snapshot (int64 words at the workspace's start)
enum : int { SW_DIGEST = 0, SW_LIVE = 1, SW_PATH16 = 4, SW_MAX_DATA = 5,
             SW_N = 6, SW_BODY = 7, SW_OVER = 8, SW_WORDS = 16 };

struct SnapWs {
  int64_t* sc;                  // [SW_WORDS]
  int64_t* cnt;                 // [cap] 1: a live node
  int64_t* sz;                  // [cap] its record's padded bytes
  int64_t* idx;                 // [cap] record index (scan of cnt)
  int64_t* off;                 // [cap] record offset in the body (of sz)
  int64_t* scan;                // zk_scan_workspace(cap)
};

ZK_DEV void st_le64(uint8_t* p, int64_t v) { __builtin_memcpy(p, &v, 8); }

// ---- snapshot ----------------------------------------------------------------
// The sources of node v's record.
struct RecSrc {
  const uint8_t *path, *slot, *acl;     // acl null: a lost binding
  int32_t pl, dl, al;
  uint32_t aver;                        // the slot's aversion
  int64_t cn, pz, eph;
};

ZK_DEV RecSrc rec_src(const ZkTree& t, const ZkAclTable& a, bool has_acl,
                      int64_t v) {
  RecSrc s;
  const int64_t pw = t.node_pw[v];
  s.path = node_path(t, pw);
  s.pl = pw_len(pw);
  s.slot = t.store.slab + t.store.slot_off[v];
  s.dl = max(t.store.data_len[v], 0);
  s.aver = (uint32_t)ld_be32(s.slot + 40);
  s.cn = t.cn[v];
  s.pz = t.pzxid[v];
  s.eph = t.eph[v];
  s.acl = SNAP_OPEN_ACL;
  s.al = SNAP_OPEN_ACL_BYTES;
  if (has_acl) {
    const int64_t w = v < a.cap ? a.node_acl[v] : ACL_LOST;
    if (acl_word_ok(a, w)) {
      s.acl = a.arena + acl_off(w);
      s.al = acl_len(w);
    } else {
      s.acl = nullptr;
      s.al = 4;
    }
  }
  return s;
}

ZK_DEV int64_t rec_bytes(const RecSrc& s) {
  return snap_pad8(4 + (int64_t)s.pl + SNAP_STAT + 4 + s.dl + s.al);
}

// Byte q of the record: the length words, the path, the Stat (the slot's,
// with cversion / numChildren / pzxid / ephemeralOwner from their shadows:
// what a read of the node answers), the data, the ACL, zero padding.
ZK_DEV uint32_t rec_byte(const RecSrc& s, int64_t q) {
  auto be = [](uint32_t x, int64_t k) { return (x >> (8 * (3 - k))) & 0xffu; };
  if (q < 4) return be((uint32_t)s.pl, q);
  q -= 4;
  if (q < s.pl) return s.path[q];
  q -= s.pl;
  if (q < SNAP_STAT_HEAD) return s.slot[q];
  if (q < SNAP_STAT) {
    // (past the version every word is a register: no load)
    const int w = (int)(q >> 2);
    const uint32_t x =
        w == 9 ? (uint32_t)cn_cver(s.cn) : w == 10 ? s.aver
        : w == 11 ? (uint32_t)((uint64_t)s.eph >> 32)
        : w == 12 ? (uint32_t)s.eph : w == 13 ? (uint32_t)s.dl
        : w == 14 ? (uint32_t)cn_nchild(s.cn)
        : w == 15 ? (uint32_t)((uint64_t)s.pz >> 32) : (uint32_t)s.pz;
    return be(x, q & 3);
  }
  q -= SNAP_STAT;
  if (q < 4) return be((uint32_t)s.dl, q);
  q -= 4;
  if (q < s.dl) return s.slot[ZK_SLOT_DATA + q];
  q -= s.dl;
  if (q < s.al) return s.acl != nullptr ? s.acl[q] : 0xffu;
  return 0;
}

// Pass 1, a thread per node slot: is it live, and how long is its record;
// the header's path16 and max_data over the same nodes (one atomic each per
// workgroup).
__global__ __launch_bounds__(TR_T) void snap_size_k(ZkTree t, ZkAclTable a,
                                                   int32_t has_acl, SnapWs w) {
  __shared__ int64_t sm[TR_T / 64 + 1];
  __shared__ int32_t mx[TR_T / 64];
  const int64_t v = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const int64_t nn = min(t.counters[TC_NODES], t.store.cap);
  const bool live = v < nn && t.node_parent[v] != NODE_FREE;
  int64_t sz = 0, p16 = 0;
  int32_t dl = 0;
  if (live) {
    const RecSrc s = rec_src(t, a, has_acl != 0, v);
    sz = rec_bytes(s);
    p16 = snap_pad16(s.pl);
    dl = s.dl;
  }
  if (v < t.store.cap) {
    w.cnt[v] = live ? 1 : 0;
    w.sz[v] = sz;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) dl = max(dl, __shfl_xor(dl, d, 64));
  if ((threadIdx.x & 63) == 0) mx[threadIdx.x >> 6] = dl;
  int64_t tot;
  block_excl_scan(p16, sm, &tot);             // (its barriers cover mx[])
  if (threadIdx.x == 0) {
    int32_t m = 0;
    for (int k = 0; k < TR_T / 64; ++k) m = max(m, mx[k]);
    if (tot) atomicAdd((unsigned long long*)&w.sc[SW_PATH16],
                       (unsigned long long)tot);
    if (m) atomicMax((unsigned long long*)&w.sc[SW_MAX_DATA],
                     (unsigned long long)m);
  }
}

// After the scans: the image's size.  total[0] = bytes, total[1] = records.
__global__ void snap_total_k(SnapWs w, int64_t* __restrict__ total) {
  total[0] = SNAP_HEAD + 8 * (w.sc[SW_N] + 1) + w.sc[SW_BODY];
  total[1] = w.sc[SW_N];
}

// The header and the table's last word, or SNAP_NO_ROOM and nothing at all
// when the image does not fit out_cap.
__global__ void snap_head_k(ZkTree t, SnapWs w, uint8_t* __restrict__ out,
                            int64_t out_cap, int64_t* __restrict__ status) {
  const int64_t n = w.sc[SW_N], body = w.sc[SW_BODY];
  const bool over = SNAP_HEAD + 8 * (n + 1) + body > out_cap;
  w.sc[SW_OVER] = over ? 1 : 0;
  status[0] = over ? SNAP_NO_ROOM : SNAP_OK;
  status[1] = -1;
  if (over) return;
  st_le64(out + SH_MAGIC, (int64_t)SNAP_MAGIC);
  st_le64(out + SH_VERSION, (int64_t)SNAP_VERSION);     // (+ reserved 0)
  st_le64(out + SH_N, n);
  st_le64(out + SH_BODY, body);
  st_le64(out + SH_ZXID, t.counters[TC_ZXID]);
  st_le64(out + SH_DIGEST, w.sc[SW_DIGEST]);
  st_le64(out + SH_PATH16, w.sc[SW_PATH16]);
  st_le64(out + SH_MAX_DATA, w.sc[SW_MAX_DATA]);
  st_le64(out + SNAP_HEAD + 8 * n, body);
}

// Pass 2.  The records of up to SNAP_SMALL bytes are written by
// snap_write_k, SNAP_GROUP lanes per node slot, the longer ones by
// snap_write_wave_k, a wave per record.  The record is cut into the 16-byte
// pieces of the DESTINATION's alignment (records start on 8 bytes, so the
// first and the last piece may be halves); lane l moves pieces l, l + G, ...:
// a group's stores cover one record, a wave's one contiguous span.  A piece
// inside the path, the data or the ACL is one 16-byte load and one 16-byte
// store.  Any other piece goes as two 8-byte halves: a half inside one of
// those or inside the Stat's first 36 bytes is one 8-byte load, a half over
// a seam, the length words and the Stat's tail (four of its fields come from
// the shadows) is put together from bytes.  Each lane loads a trip's piece
// before it stores it, and trips do not depend on one another.
template <int G>
ZK_DEV void write_record(const ZkTree& t, const ZkAclTable& a, bool has_acl,
                         const SnapWs& w, uint8_t* __restrict__ out,
                         int64_t v, int l) {
  const int64_t R = w.sz[v];
  const int64_t n = w.sc[SW_N], off = w.off[v];
  if (l == 0) st_le64(out + SNAP_HEAD + 8 * w.idx[v], off);
  uint8_t* o = out + SNAP_HEAD + 8 * (n + 1) + off;
  const RecSrc s = rec_src(t, a, has_acl, v);
  // region bounds inside the record
  const int64_t p0 = 4, p1 = p0 + s.pl;               // path
  const int64_t s1 = p1 + SNAP_STAT_HEAD;             // the Stat's head
  const int64_t d0 = p1 + SNAP_STAT + 4, d1 = d0 + s.dl;   // data
  const int64_t a0 = d1, a1 = s.acl != nullptr ? a0 + s.al : a0;   // ACL
  // the source of [p, p + len) when one region holds it, else null
  auto whole = [&](int64_t p, int64_t len) -> const uint8_t* {
    if (p >= p0 && p + len <= p1) return s.path + (p - p0);
    if (p >= d0 && p + len <= d1) return s.slot + ZK_SLOT_DATA + (p - d0);
    if (p >= a0 && p + len <= a1) return s.acl + (p - a0);
    if (len == 8 && p >= p1 && p + len <= s1) return s.slot + (p - p1);
    return nullptr;
  };
  const int64_t vs = -(int64_t)((uintptr_t)o & 15);   // 0 or -8
  for (int64_t p = vs + (int64_t)l * 16; p < R; p += (int64_t)G * 16) {
    const uint8_t* src = whole(p, 16);
    if (src != nullptr) {
      uint4 x;
      __builtin_memcpy(&x, src, 16);
      *(uint4*)(o + p) = x;
      continue;
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int64_t q = p + 8 * hf;
      if (q < 0 || q >= R) continue;                  // (R is 8-aligned)
      uint64_t x = 0;
      const uint8_t* h = whole(q, 8);
      if (h != nullptr) {
        __builtin_memcpy(&x, h, 8);
      } else {
#pragma unroll
        for (int b = 0; b < 8; ++b)
          x |= (uint64_t)rec_byte(s, q + b) << (8 * b);
      }
      *(uint64_t*)(o + q) = x;
    }
  }
}

__global__ __launch_bounds__(TR_T) void snap_write_k(
    ZkTree t, ZkAclTable a, int32_t has_acl, SnapWs w,
    uint8_t* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const int64_t v = g / SNAP_GROUP;
  if (v >= t.store.cap || w.sc[SW_OVER] != 0 || w.cnt[v] == 0 ||
      w.sz[v] > SNAP_SMALL)
    return;
  write_record<SNAP_GROUP>(t, a, has_acl != 0, w, out, v,
                           (int)(g % SNAP_GROUP));
}

// The long records: every wave looks at 64 node slots a trip, a lane each,
// and writes the long ones among them one after the other, all 64 lanes on
// one record.  (A launch of a wave per node slot spent 128 us on a 1.1M-slot
// tree without one long record.)
__global__ __launch_bounds__(TR_T) void snap_write_wave_k(
    ZkTree t, ZkAclTable a, int32_t has_acl, SnapWs w,
    uint8_t* __restrict__ out) {
  if (w.sc[SW_OVER] != 0) return;
  const int lane = lane_id();
  const int64_t wave = ((int64_t)blockIdx.x * TR_T + threadIdx.x) >> 6;
  const int64_t step = (int64_t)gridDim.x * TR_T;     // node slots a trip
  for (int64_t base = wave * 64; base < t.store.cap; base += step) {
    const int64_t v = base + lane;
    const bool big = v < t.store.cap && w.cnt[v] != 0 &&
                     w.sz[v] > SNAP_SMALL;
    uint64_t m = __ballot(big);
    while (m != 0) {
      const int j = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      write_record<64>(t, a, has_acl != 0, w, out, base + j, lane);
    }
  }
}

// ---- load --------------------------------------------------------------------
// The outcome of a load is ONE word, the smallest over every failure seen:
// code << 40 | record index + 1 (all ones: no failure), so the earliest
// failing phase and its smallest record index win whatever order the lanes
// report in.  Every kernel after the first returns at once when the word
// holds a failure of an EARLIER launch (a kernel boundary orders them:
// load_ok / load_go).
struct LoadWs {
  unsigned long long* key;      // [1] the outcome word
  int64_t* tot;                 // [2] path bytes, slab bytes used
  unsigned long long* dig;      // [4] zk_tree_digest's words
  int64_t* p16;                 // [n] path storage of record i
  int64_t* sb;                  // [n] slot bytes of record i
  int64_t* poff;                // [n]
  int64_t* soff;                // [n]
  int32_t* aslot;               // [n] ACL index slot / AS_*
  int64_t* scan;                // zk_scan_workspace(n)
};
constexpr unsigned long long LOAD_CLEAN = ~0ull;

ZK_DEV void load_fail(const LoadWs& w, int32_t code, int64_t index) {
  atomicMin(w.key, (unsigned long long)code << 40 |
                       (unsigned long long)(index + 1));
}
ZK_DEV bool load_ok(const LoadWs& w) { return *w.key == LOAD_CLEAN; }
// For the lanes of a launch that reports `code` itself: a failure another
// lane of the same launch has just reported does not stop this one (the
// smallest index would be missed), one of an earlier launch does.
ZK_DEV bool load_go(const LoadWs& w, int32_t code) {
  const unsigned long long k = *w.key;
  return k == LOAD_CLEAN || (int64_t)(k >> 40) >= code;
}

struct Image {
  const uint8_t* p;
  int64_t len, n;               // n: the record count the launches are sized by
};
ZK_DEV const uint8_t* img_tab(const Image& m) { return m.p + SNAP_HEAD; }
ZK_DEV const uint8_t* img_body(const Image& m) {
  return m.p + SNAP_HEAD + 8 * (m.n + 1);
}

// 1. the header (one thread): everything the later kernels take from it is
// checked against the image's length here; the record count the host sized
// the launches by must be the header's.
__global__ void load_head_k(Image m, LoadWs w) {
  SnapHead h;
  int32_t rc = snap_check_header(m.p, m.len, &h);
  if (rc == SNAP_OK && h.n != m.n) rc = SNAP_BAD_HEADER;
  if (rc != SNAP_OK) load_fail(w, rc, rc == SNAP_BAD_TABLE ? 0 : -1);
}

// 2. a thread per record: its table entry, then the record against its span,
// and its storage needs.
__global__ __launch_bounds__(TR_T) void load_check_k(Image m, int32_t data_cap,
                                                    LoadWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= m.n || !load_go(w, SNAP_BAD_TABLE)) return;
  const int64_t body = ld_le64(m.p + SH_BODY);
  int64_t p16 = 0, sb = 0;
  if (!snap_check_table(img_tab(m), m.n, body, i)) {
    load_fail(w, SNAP_BAD_TABLE, i);
  } else {
    const int64_t a = ld_le64(img_tab(m) + 8 * i);
    const int64_t b = ld_le64(img_tab(m) + 8 * (i + 1));
    SnapRec r;
    if (!snap_check_record(img_body(m) + a, b - a, &r)) {
      load_fail(w, SNAP_BAD_RECORD, i);
    } else {
      p16 = snap_pad16(r.pl);
      sb = slot_bytes(max(data_cap, r.dl));
    }
  }
  w.p16[i] = p16;
  w.sb[i] = sb;
}

// 3. after the scans (one thread): do nodes, path arena and slab all fit.
__global__ void load_room_k(ZkTree t, Image m, LoadWs w) {
  if (!load_ok(w)) return;
  // (the index at most half full; a hash val holds slot offsets below 2^35)
  if (m.n > t.store.cap || m.n > t.free_cap || 2 * m.n > t.mask + 1 ||
      w.tot[0] > t.path_cap || w.tot[1] > t.slab_cap ||
      w.tot[1] >= (1ll << 35))
    load_fail(w, SNAP_NO_ROOM, -1);
}

// 4. place record i at node i: path, slot, shadows; a provisional root parent.
__global__ __launch_bounds__(TR_T) void load_place_k(ZkTree t, Image m,
                                                    int32_t data_cap,
                                                    LoadWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= m.n || !load_ok(w)) return;
  const uint8_t* rec = img_body(m) + ld_le64(img_tab(m) + 8 * i);
  const int64_t span = ld_le64(img_tab(m) + 8 * (i + 1)) -
                       ld_le64(img_tab(m) + 8 * i);
  SnapRec r;
  if (!snap_check_record(rec, span, &r)) return;      // (checked: cannot be)
  const ZkNodeStore& s = t.store;
  const int64_t po = w.poff[i], so = w.soff[i];
  copy_bytes(t.path_arena + po, rec + r.path, r.pl);
  t.node_path_off[i] = po;
  t.node_path_len[i] = r.pl;
  t.node_path_cap[i] = (int32_t)snap_pad16(r.pl);
  t.node_pw[i] = pw_pack(po, r.pl);
  uint8_t* slot = s.slab + so;
  const uint8_t* st = rec + r.stat;
  copy_bytes(slot, st, SNAP_STAT);
  st_be32(slot + 68, 0);
  st_be32(slot + ZK_SLOT_LEN, r.dl > 0 ? r.dl : -1);
  copy_bytes(slot + ZK_SLOT_DATA, rec + r.data, r.dl);
  s.slot_off[i] = so;
  s.data_len[i] = r.dl;
  s.slot_cap[i] = max(data_cap, r.dl);
  t.cn[i] = cn_pack(ld_be32(st + 36), ld_be32(st + 56));
  t.eph[i] = ld_be64(st + 44);
  t.pzxid[i] = ld_be64(st + 60);
  t.dirty[i] = 0;
  t.node_parent[i] = -1;
}

// 5. the index: the serve's own insert; a path already there is a duplicate.
// Two launches.  tree_insert waits (bounded) for the claimer of its key to
// publish; a claimer in the waiting lane's own wave cannot run meanwhile, so
// records of one 64-bit key (a duplicate, or paths made up to collide) that
// share a wave end in TREE_INSERT_TIMEOUT for all but the first.  Such a
// record is flagged (w.p16, free since the scans) and inserted again by the
// second launch, in which the flagged lanes of a wave insert ONE AT A TIME
// (a ballot loop): no claimer of the key is ever in the inserting lane's own
// wave, so however many records of one key a wave holds, a true duplicate
// finds the published entry and a colliding path takes the next one.
template <bool RETRY>
__global__ __launch_bounds__(TR_T) void load_index_k(ZkTree t, Image m,
                                                    LoadWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  bool need = i < m.n && load_go(w, SNAP_DUP_PATH);
  if (RETRY) need = need && w.p16[i] != 0;
  int64_t pw = 0, so = 0;
  int32_t dl = 0;
  if (need) {
    pw = t.node_pw[i];
    so = t.store.slot_off[i];
    dl = t.store.data_len[i];
  }
  int64_t ins = i;
  if (!RETRY) {
    if (need) ins = tree_insert(t, i, node_path(t, pw), pw_len(pw), dl, so);
    if (need) w.p16[i] = ins == TREE_INSERT_TIMEOUT ? 1 : 0;
    if (ins == TREE_INSERT_TIMEOUT) ins = i;        // (the second launch's)
  } else {
    const int lane = lane_id();
    uint64_t todo = __ballot(need);
    while (todo != 0) {                             // (wave-uniform)
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      if (lane == j)
        ins = tree_insert(t, i, node_path(t, pw), pw_len(pw), dl, so);
    }
  }
  if (need && ins != i) load_fail(w, SNAP_DUP_PATH, i);
}

// 6. parents, in a launch of their own (every path is indexed by now): a
// path with one '/' is a root, any other looks its parent's path up.
__global__ __launch_bounds__(TR_T) void load_parent_k(ZkTree t, Image m,
                                                     LoadWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= m.n || !load_go(w, SNAP_ORPHAN)) return;
  const int64_t pw = t.node_pw[i];
  const uint8_t* p = node_path(t, pw);
  int32_t cut = pw_len(pw) - 1;
  while (cut > 0 && p[cut] != '/') --cut;
  if (cut == 0) return;                               // (-1, from the place)
  const int64_t par = tree_find(t, p, cut);
  if (par < 0) load_fail(w, SNAP_ORPHAN, i);
  else t.node_parent[i] = par;
}

// 7. ACLs, on a tree with a table: two launches, as the record pass of a
// CREATE batch has them (tree_acl.hip), so that no lane waits for another's
// store.  load_acl_intern_k: a thread per record finds or claims its
// vector's key in the intern index; an entry from before the load (the
// open ACL the table starts with: its bytes end below AC_OLD_TOP) is
// compared byte for byte, an entry of this launch is taken on its hash.
// The wave's claimers take entry numbers and arena bytes with one atomic
// each and publish the arena word, or ACL_LOST when the store is full.
// load_acl_bind_k: the published word, its bytes against the record's (two
// new vectors with one hash: the loser is lost), node_acl[i]; a record
// with count -1 is bound lost.  AC_OLD_TOP moves up, so the record pass of
// a later CREATE compares against the loaded vectors.
__global__ __launch_bounds__(TR_T) void load_acl_intern_k(ZkAclTable a,
                                                         Image m, LoadWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const int lane = lane_id();
  const bool run = load_ok(w);                        // (uniform)
  int32_t slot = AS_NONE, len = 0;
  const uint8_t* vec = nullptr;
  if (run && i < m.n && i < a.cap) {
    const int64_t o = ld_le64(img_tab(m) + 8 * i);
    SnapRec r;
    if (snap_check_record(img_body(m) + o,
                          ld_le64(img_tab(m) + 8 * (i + 1)) - o, &r) &&
        r.acl_count > 0) {
      vec = img_body(m) + o + r.acl;
      len = (int32_t)r.acl_len;
      slot = AS_LOST;
    }
  }
  bool claimed = false;
  if (vec != nullptr) {
    const int64_t h = (int64_t)(path_hash(vec, len) | 1ull);
    const int64_t old_top = a.ctr[AC_OLD_TOP];
    int64_t s = (int64_t)((uint64_t)h >> 8) & a.hmask;
    for (int64_t probe = 0; probe <= a.hmask; ++probe) {
      int64_t k = ld_relaxed(&a.key[s]);
      if (k == 0) {
        k = (int64_t)atomicCAS((unsigned long long*)&a.key[s], 0ull,
                               (unsigned long long)h);
        if (k == 0) {
          claimed = true;
          slot = (int32_t)s;
          break;
        }
      }
      if (k == h) {
        const int64_t v = ld_relaxed(&a.val[s]);
        bool other = false;
        if (acl_word_ok(a, v) && acl_off(v) + acl_len(v) <= old_top)
          other = acl_len(v) != len ||
                  !bytes_eq(a.arena + acl_off(v), vec, len);
        if (!other) {
          slot = (int32_t)s;
          break;
        }
      }
      s = (s + 1) & a.hmask;
    }
  }
  const uint64_t cm = __ballot(claimed);
  if (cm != 0) {                                   // (wave-uniform)
    const int lead = __ffsll((unsigned long long)cm) - 1;
    long long base = 0;
    if (lane == lead)
      base = (long long)atomicAdd((unsigned long long*)&a.ctr[AC_ENT],
                                  (unsigned long long)__popcll(cm));
    base = __shfl(base, lead, 64);
    const int rank = __popcll(cm & ((1ull << lane) - 1ull));
    bool ok = claimed && base + rank < a.ctr[AC_LIMIT];
    const int64_t o = wave_bytes(&a.ctr[AC_TOP], ok ? (int64_t)len : 0);
    if (ok && (o < 0 || o + len > a.arena_cap)) ok = false;
    if (claimed) {
      int64_t word = ACL_LOST;
      if (ok) {
        copy_bytes(a.arena + o, vec, len);
        word = (o << 24) | (int64_t)len;
      }
      __hip_atomic_store(&a.val[slot], word, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint64_t fail = __ballot(claimed && !ok);
    if (fail != 0 && lane == lead)
      atomicAdd((unsigned long long*)&a.ctr[AC_ENT],
                (unsigned long long)(-(long long)__popcll(fail)));
  }
  if (run && i < m.n) w.aslot[i] = slot;
}

__global__ __launch_bounds__(TR_T) void load_acl_bind_k(ZkAclTable a, Image m,
                                                       LoadWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const bool run = load_ok(w);
  // (nothing claims arena bytes in this launch: the top is the load's)
  if (run && i == 0) a.ctr[AC_OLD_TOP] = a.ctr[AC_TOP];
  bool lost = false;
  if (run && i < m.n && i < a.cap) {
    const int32_t slot = w.aslot[i];
    int64_t word = ACL_LOST;
    if (slot >= 0 && (int64_t)slot <= a.hmask) {
      const int64_t o = ld_le64(img_tab(m) + 8 * i);
      SnapRec r;
      const int64_t v = a.val[slot];
      if (snap_check_record(img_body(m) + o,
                            ld_le64(img_tab(m) + 8 * (i + 1)) - o, &r) &&
          acl_word_ok(a, v) && acl_len(v) == (int32_t)r.acl_len &&
          bytes_eq(a.arena + acl_off(v), img_body(m) + o + r.acl,
                   (int32_t)r.acl_len))
        word = v;
    }
    a.node_acl[i] = word;
    lost = word == ACL_LOST;
  }
  const uint64_t lm = __ballot(lost);
  if (lm != 0 && lane_id() == __ffsll((unsigned long long)lm) - 1)
    atomicAdd((unsigned long long*)&a.ctr[AC_LOST],
              (unsigned long long)__popcll(lm));
}

// 8. the counters (one thread): the loaded tree is dense, its ring empty.
__global__ void load_counters_k(ZkTree t, Image m, LoadWs w) {
  if (!load_ok(w)) return;
  int64_t* c = t.counters;
  c[TC_NODES] = m.n;
  c[TC_ZXID] = ld_le64(m.p + SH_ZXID);
  c[TC_PATH_TOP] = w.tot[0];
  c[TC_SLAB_TOP] = w.tot[1];
  c[TC_FREE_HEAD] = c[TC_FREE_TAIL] = c[TC_FREE_PUB] = 0;
  c[TC_DIRTY] = 0;
}

// 9. the verdict (one thread): the loaded tree's digest against the
// header's, and the outcome word as (code, record index).
__global__ void load_verdict_k(Image m, LoadWs w, int64_t* __restrict__ status) {
  if (load_ok(w) &&
      (w.dig[0] != (unsigned long long)ld_le64(m.p + SH_DIGEST) ||
       w.dig[1] != (unsigned long long)m.n))
    load_fail(w, SNAP_DIGEST, -1);
  const unsigned long long k = *w.key;
  status[0] = k == LOAD_CLEAN ? SNAP_OK : (int64_t)(k >> 40);
  status[1] = k == LOAD_CLEAN ? -1 : (int64_t)(k & ((1ull << 40) - 1)) - 1;
}

static int64_t a16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// Workspace layouts (bytes; 16-aligned parts).
static int64_t snap_layout(int64_t cap, uint8_t* ws, SnapWs* w) {
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    uint8_t* p = ws != nullptr ? ws + o : nullptr;
    o += a16(bytes);
    return (int64_t*)p;
  };
  int64_t* sc = take(SW_WORDS * 8);
  int64_t* part[4];
  for (auto& p : part) p = take(cap * 8);
  int64_t* scan = take(zk_scan_workspace(cap > 0 ? cap : 1) * 8);
  if (w != nullptr) *w = SnapWs{sc, part[0], part[1], part[2], part[3], scan};
  return o;
}

static int64_t load_layout(int64_t n, uint8_t* ws, LoadWs* w) {
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    uint8_t* p = ws != nullptr ? ws + o : nullptr;
    o += a16(bytes);
    return p;
  };
  uint8_t* head = take(64);
  uint8_t* part[4];
  for (auto& p : part) p = take(n * 8);
  uint8_t* aslot = take(n * 4);
  uint8_t* scan = take(zk_scan_workspace(n > 0 ? n : 1) * 8);
  if (w != nullptr)
    *w = LoadWs{(unsigned long long*)head, (int64_t*)(head + 8),
                (unsigned long long*)(head + 32), (int64_t*)part[0],
                (int64_t*)part[1], (int64_t*)part[2], (int64_t*)part[3],
                (int32_t*)aslot, (int64_t*)scan};
  return o;
}

static bool acl_table_ok(const ZkAclTable* a) {
  return a->cap > 0 && a->arena_cap > 0 && a->hmask >= 0 &&
         (a->hmask & (a->hmask + 1)) == 0;
}

}  // namespace zk

extern "C" {

int64_t zk_tree_snap_workspace(int64_t cap) {
  return zk::snap_layout(cap > 0 ? cap : 0, nullptr, nullptr);
}

int64_t zk_tree_load_workspace(int64_t n) {
  return zk::load_layout(n > 0 ? n : 0, nullptr, nullptr);
}

// Size the image of tree t (a: its ACL table, or null): the live nodes'
// record sizes, offsets and indices into ws (zk_tree_snap_write reads them:
// the tree must not change in between), the digest of the same nodes, and
// total[0] = image bytes, total[1] = records.  No host read.
int zk_tree_snap_size(const ZkTree* t, const ZkAclTable* a, uint8_t* ws,
                      int64_t ws_bytes, int64_t* total, hipStream_t st) {
  const int64_t cap = t->store.cap;
  if (cap <= 0 || cap >= 0x7fffffff / 64) return -1;
  if (ws_bytes < zk_tree_snap_workspace(cap) || ((uintptr_t)ws & 15))
    return -1;
  if (a != nullptr && !zk::acl_table_ok(a)) return -1;
  zk::SnapWs w;
  zk::snap_layout(cap, ws, &w);
  if (hipMemsetAsync(w.sc, 0, zk::SW_WORDS * 8, st) != hipSuccess) return -4;
  const ZkAclTable none{};
  const unsigned nb = (unsigned)((cap + zk::TR_T - 1) / zk::TR_T);
  zk::snap_size_k<<<nb, zk::TR_T, 0, st>>>(*t, a != nullptr ? *a : none,
                                           a != nullptr, w);
  ZK_LAUNCH_CHECK();
  int rc = zk_scan_excl_i64(w.cnt, w.idx, cap, &w.sc[zk::SW_N], w.scan, st);
  if (rc) return rc;
  rc = zk_scan_excl_i64(w.sz, w.off, cap, &w.sc[zk::SW_BODY], w.scan, st);
  if (rc) return rc;
  // (the digest's two words: SW_DIGEST, SW_LIVE)
  rc = zk::digest_launch(t, (unsigned long long*)w.sc, st);
  if (rc) return rc;
  zk::snap_total_k<<<1, 1, 0, st>>>(w, total);
  ZK_LAUNCH_CHECK();
  return 0;
}

// Write the image zk_tree_snap_size sized on ws into out[0, out_cap) (16-byte
// aligned).  status[0] = SNAP_OK, or SNAP_NO_ROOM when it does not fit: then
// nothing is written.  status[1] = -1.  No host read.
int zk_tree_snap_write(const ZkTree* t, const ZkAclTable* a, uint8_t* ws,
                       int64_t ws_bytes, uint8_t* out, int64_t out_cap,
                       int64_t* status, hipStream_t st) {
  const int64_t cap = t->store.cap;
  if (cap <= 0 || cap >= 0x7fffffff / 64 || out_cap < 0) return -1;
  if (ws_bytes < zk_tree_snap_workspace(cap) || ((uintptr_t)ws & 15) ||
      ((uintptr_t)out & 15))
    return -1;
  if (a != nullptr && !zk::acl_table_ok(a)) return -1;
  zk::SnapWs w;
  zk::snap_layout(cap, ws, &w);
  const ZkAclTable none{};
  const ZkAclTable& at = a != nullptr ? *a : none;
  zk::snap_head_k<<<1, 1, 0, st>>>(*t, w, out, out_cap, status);
  ZK_LAUNCH_CHECK();
  const unsigned nb8 =
      (unsigned)((cap * zk::SNAP_GROUP + zk::TR_T - 1) / zk::TR_T);
  zk::snap_write_k<<<nb8, zk::TR_T, 0, st>>>(*t, at, a != nullptr, w, out);
  ZK_LAUNCH_CHECK();
  const int64_t nbw = (cap + zk::TR_T - 1) / zk::TR_T;
  zk::snap_write_wave_k<<<(unsigned)(nbw < 2048 ? nbw : 2048), zk::TR_T, 0,
                          st>>>(*t, at, a != nullptr, w, out);
  ZK_LAUNCH_CHECK();
  return 0;
}

// Load image img[0, img_len) of n records (the host's reading of the
// header; the device checks it) into the fresh, empty tree t (all-zero hash
// table and counters; a: its ACL table as GpuTree makes it, or null), with
// data capacity max(data_cap, data length) per node.  status[0] = SNAP_*,
// status[1] = the record index (-1: none).  A refused image leaves the tree
// in no usable state.  No host read.
int zk_tree_load(const ZkTree* t, const ZkAclTable* a, const uint8_t* img,
                 int64_t img_len, int64_t n, int32_t data_cap, uint8_t* ws,
                 int64_t ws_bytes, int64_t* status, hipStream_t st) {
  if (img_len < 0 || n < 0 || n >= 0x7fffffff || data_cap < 0) return -1;
  if (ws_bytes < zk_tree_load_workspace(n) || ((uintptr_t)ws & 15)) return -1;
  if (a != nullptr && !zk::acl_table_ok(a)) return -1;
  zk::LoadWs w;
  zk::load_layout(n, ws, &w);
  if (hipMemsetAsync(w.key, 0xFF, 8, st) != hipSuccess) return -4;
  if (hipMemsetAsync(w.tot, 0, 16, st) != hipSuccess) return -4;
  if (hipMemsetAsync(w.dig, 0, 32, st) != hipSuccess) return -4;
  const zk::Image m{img, img_len, n};
  const unsigned nb = (unsigned)((n + zk::TR_T - 1) / zk::TR_T);
  zk::load_head_k<<<1, 1, 0, st>>>(m, w);
  ZK_LAUNCH_CHECK();
  if (n > 0) {
    zk::load_check_k<<<nb, zk::TR_T, 0, st>>>(m, data_cap, w);
    ZK_LAUNCH_CHECK();
    int rc = zk_scan_excl_i64(w.p16, w.poff, n, &w.tot[0], w.scan, st);
    if (rc) return rc;
    rc = zk_scan_excl_i64(w.sb, w.soff, n, &w.tot[1], w.scan, st);
    if (rc) return rc;
  }
  zk::load_room_k<<<1, 1, 0, st>>>(*t, m, w);
  ZK_LAUNCH_CHECK();
  if (n > 0) {
    zk::load_place_k<<<nb, zk::TR_T, 0, st>>>(*t, m, data_cap, w);
    ZK_LAUNCH_CHECK();
    zk::load_index_k<false><<<nb, zk::TR_T, 0, st>>>(*t, m, w);
    ZK_LAUNCH_CHECK();
    zk::load_index_k<true><<<nb, zk::TR_T, 0, st>>>(*t, m, w);
    ZK_LAUNCH_CHECK();
    zk::load_parent_k<<<nb, zk::TR_T, 0, st>>>(*t, m, w);
    ZK_LAUNCH_CHECK();
    if (a != nullptr) {
      zk::load_acl_intern_k<<<nb, zk::TR_T, 0, st>>>(*a, m, w);
      ZK_LAUNCH_CHECK();
      zk::load_acl_bind_k<<<nb, zk::TR_T, 0, st>>>(*a, m, w);
      ZK_LAUNCH_CHECK();
    }
  }
  zk::load_counters_k<<<1, 1, 0, st>>>(*t, m, w);
  ZK_LAUNCH_CHECK();
  const int rc = zk::digest_launch(t, w.dig, st);
  if (rc) return rc;
  zk::load_verdict_k<<<1, 1, 0, st>>>(m, w, status);
  ZK_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
