// GPU-resident synthetic ZooKeeper tree (the server side of the 1M-znode
// benchmark, the create/set/delete mix and the ephemeral create storm).  Not
// part of the reference — it stands in for the JVM server the reference's
// tests talk to, so that the whole request -> reply path runs at HBM speed.
//
// Layout (HBM, sized by the caller for 288 GB parts):
//   * open-addressing hash table of 64-byte entries {key, val, path head,
//     data length} (one line per probe): key = word-wise multiply-xorshift
//     hash of the path | 1, val = node and slot + 1 (-2 = tombstone, 0 =
//     empty or being published), linear probing, pow2 capacity;
//   * node slots in wire format (zk_batch.h ZkNodeStore), so replies are
//     contiguous copies;
//   * a path arena holding each node's path for exact-match verification;
//   * counters (TC_*): node high-water mark, zxid, path-arena top, slab top,
//     the free-node ring (head / tail / published tail) and the dirty count;
//   * a free-node ring: DELETE (and session expiry) push the node index,
//     CREATE pops one published by an EARLIER launch (tree_publish_k runs
//     between batches), reusing its slot and path storage when they fit;
//   * host-endian shadows of each node's cversion / numChildren (one packed
//     word, cn_*) and pzxid.
//     Children come and go with plain atomicAdd / atomicMax on these (a
//     big-endian Stat word would need a CAS retry loop, and ~1000 parents
//     shared by a million writes contend); every parent touched in a launch
//     is put on a dirty list once, and tree_fixup_k rewrites the wire-format
//     Stat words of exactly those parents before replies are encoded.
//
// Single-address counters (free ring, node bump, dirty list) are claimed
// once per BLOCK (ballot/mbcnt ranks + an LDS prefix, one atomic), the rare
// byte claims of the arena bump allocators once per wave (64-lane shuffle
// scan); zxids need no atomic at all (base + request index).  For that the
// serve and expire kernels keep every thread alive to the end (out-of-range
// threads carry a no-op).
//
// Requests are applied concurrently within a batch, except that requests
// on ONE path are applied in batch (xid) order when any of them writes:
// tree_order.hip ranks every request by the number of earlier same-path
// requests of the batch and the serve kernel runs in passes of equal rank
// (ZooKeeper applies a session's requests in order; requests on different
// paths commute).  Version CAS is an atomicCAS on the slot's big-endian
// version word, so exactly one of several same-version SET_DATAs wins (the
// others get BAD_VERSION), matching ZooKeeper's conditional set.  Every
// write request is assigned a zxid, failed ones included (ZooKeeper logs an
// error txn for them).
//
// This header holds what every pass over the tree shares: the constants,
// the claims, the hash index, the watch table and the parent bookkeeping
// (all __forceinline__ device code), and at its end the few host functions
// through which one file launches another's kernel.  The kernels and their
// launchers: tree.hip, tree_order.hip, tree_seq.hip, tree_list.hip,
// tree_watch.hip, tree_acl.hip, tree_mix.hip, tree_snap.hip.
#pragma once
#include "zk_common.h"

namespace zk {

constexpr int TR_T = 256;
enum : int {
  TC_NODES = 0, TC_ZXID = 1, TC_PATH_TOP = 2, TC_SLAB_TOP = 3,
  TC_FREE_HEAD = 4, TC_FREE_TAIL = 5, TC_FREE_PUB = 6, TC_DIRTY = 7,
  TC_SESS = 8, TC_N = 9
};
// `session` argument value meaning "the session in counters[TC_SESS]": a
// captured step whose session changes from replay to replay (the storm's
// born / resumed / expired sessions) keeps it on the device
constexpr int64_t SESS_DEV = -2;
ZK_DEV int64_t sess_of(const ZkTree& t, int64_t session) {
  return session == SESS_DEV ? t.counters[TC_SESS] : session;
}
constexpr int64_t NODE_FREE = -2;

// ordered serve: rank byte = min(rank, ORD_RANK) | ORD_SNAP (the contract
// between the ordering pass, tree_order.hip, which writes the byte, and
// tree_serve_k, which reads it)
constexpr int32_t ORD_RANK = 0x7f, ORD_SNAP = 0x80;

ZK_DEV int64_t slot_bytes(int32_t data_cap) {
  return ZK_SLOT_DATA + (((int64_t)data_cap + 15) & ~(int64_t)15) + 4;
}

// ---- aggregated claims (all threads of the block must be active) ---------
ZK_DEV int lane_id() {
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0));
}

// One ticket per thread with `want`: returns base + rank, or -1.  Ranks come
// from ballot/mbcnt within a wave and an LDS prefix over the block's waves;
// ONE atomic per block of NT threads (a single word sustains only ~88
// returning atomics/us, MI355X_MICROARCH.md "dequeue").  Every thread of the
// block must call it.
template <int NT = TR_T>
ZK_DEV int64_t block_ticket(int64_t* ctr, bool want,
                            unsigned long long* also = nullptr) {
  constexpr int TR_T = NT;
  __shared__ int64_t part[TR_T / 64 + 1];
  const int w = threadIdx.x >> 6;
  const uint64_t m = __ballot(want);
  const int rank = __builtin_amdgcn_mbcnt_hi(
      (uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
  if (lane_id() == 0) part[w] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t tot = 0;
    for (int k = 0; k < TR_T / 64; ++k) {
      const int64_t c = part[k];
      part[k] = tot;
      tot += c;
    }
    part[TR_T / 64] = tot ? (int64_t)atomicAdd((unsigned long long*)ctr,
                                               (unsigned long long)tot)
                          : 0;
    // (a second count of the same threads: its result unused, no wait)
    if (also != nullptr && tot) atomicAdd(also, (unsigned long long)tot);
  }
  __syncthreads();
  const int64_t r = want ? part[TR_T / 64] + part[w] + rank : -1;
  __syncthreads();                                 // part[] reusable
  return r;
}

// Claim `amount` (>= 0) bytes per lane; returns this lane's offset or -1.
ZK_DEV int64_t wave_bytes(int64_t* ctr, int64_t amount) {
  const int lane = lane_id();
  int64_t incl = amount;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t y = __shfl_up(incl, d, 64);
    if (lane >= d) incl += y;
  }
  const int64_t tot = __shfl(incl, 63, 64);
  if (tot == 0) return -1;
  int64_t base = 0;
  if (lane == 63)
    base = (int64_t)atomicAdd((unsigned long long*)ctr,
                              (unsigned long long)tot);
  base = __shfl(base, 63, 64);
  return amount > 0 ? base + incl - amount : -1;
}

// ---- hash index -----------------------------------------------------------
// Path hash: 8 bytes per step (unaligned loads), a multiply-xorshift per
// word and a final avalanche — 4 multiplies for a 25-byte path where a
// byte-serial FNV-1a needs 25.
ZK_DEV uint64_t path_hash(const uint8_t* p, int32_t n) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
  int32_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w; __builtin_memcpy(&w, p + i, 8);
    h = (h ^ w) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
  }
  if (i < n) {
    uint64_t w = 0;
    for (int32_t k = 0; i + k < n; ++k) w |= (uint64_t)p[i + k] << (8 * k);
    h = (h ^ w) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
  }
  h ^= h >> 33;
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  return h;
}

ZK_DEV bool bytes_eq(const uint8_t* a, const uint8_t* b, int32_t n) {
  int32_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t x, y; __builtin_memcpy(&x, a + i, 8); __builtin_memcpy(&y, b + i, 8);
    if (x != y) return false;
  }
  for (; i < n; ++i) if (a[i] != b[i]) return false;
  return true;
}

// One 64-byte entry per slot (a cache line; open addressing, linear
// probing): int64 words [0] key = path hash | 1 (0 empty), [1] val (node |
// slot offset, below; -2 tombstone, 0 empty or being published), [2] path
// length | data length << 32, [3, 8) the path's first EN_PATH bytes.  A
// lookup loads the entry in one burst and verifies the path and gets a GET
// reply's data length from it: ONE random line per lookup (rounds 2-4 read
// the 16-byte {key, val} entry and then the node's 64-byte lookup line, a
// second dependent random read).  Longer paths compare their tail in the
// arena.  (The per-node 64-byte lookup lines of round 4 are gone.)
constexpr int HT_W = 8;                    // int64 words per entry
constexpr int EN_PATH = 40;                // path bytes held in the entry

ZK_DEV int64_t* ht_ent(const ZkTree& t, int64_t s) { return &t.ht[HT_W * s]; }
ZK_DEV int64_t* ht_key(const ZkTree& t, int64_t s) { return &t.ht[HT_W * s]; }
ZK_DEV int64_t* ht_val(const ZkTree& t, int64_t s) { return &t.ht[HT_W * s + 1]; }

// Node v's path as one word (offset << 24 | length; paths < 16 MiB like
// the frames that carry them): the arena tail of a long path.
ZK_DEV int64_t pw_pack(int64_t off, int32_t len) {
  return (off << 24) | (int64_t)(uint32_t)len;
}

// The entry's path / data length words (everything but key and val); plain
// stores before the val is published.
ZK_DEV void ent_fill(const ZkTree& t, int64_t s, const uint8_t* p, int32_t n,
                     int32_t dl) {
  int64_t* e = ht_ent(t, s);
  e[2] = (int64_t)(uint32_t)n | ((int64_t)dl << 32);
  uint8_t* pb = (uint8_t*)&e[3];
  const int32_t h = n < EN_PATH ? n : EN_PATH;
  copy_bytes(pb, p, h);
}

ZK_DEV void ent_set_dlen(const ZkTree& t, int64_t s, int32_t dl) {
  __builtin_memcpy((uint8_t*)ht_ent(t, s) + 20, &dl, 4);
}

// 8 bytes of p at o (up to n: a shorter tail is zero-filled)
ZK_DEV uint64_t path_word(const uint8_t* p, int32_t o, int32_t n) {
  uint64_t w = 0;
  if (o + 8 <= n) {
    __builtin_memcpy(&w, p + o, 8);
  } else {
    for (int32_t k = 0; o + k < n; ++k) w |= (uint64_t)p[o + k] << (8 * k);
  }
  return w;
}

// Does entry e (its words loaded) name path p[0, n) of node v?
ZK_DEV bool ent_is(const ZkTree& t, const int64_t (&e)[HT_W], int64_t v,
                   const uint8_t* p, int32_t n) {
  if ((int32_t)(uint32_t)e[2] != n) return false;
  const int32_t h = n < EN_PATH ? n : EN_PATH;
#pragma unroll
  for (int w = 0; w < EN_PATH / 8; ++w) {
    if (8 * w >= h) break;
    uint64_t x = (uint64_t)e[3 + w];
    const int32_t left = h - 8 * w;
    if (left < 8) x &= (1ull << (8 * left)) - 1;   // (copy_bytes left the
                                                   // rest of the word as is)
    if (x != path_word(p, 8 * w, h)) return false;
  }
  if (n <= EN_PATH) return true;
  const int64_t pw = t.node_pw[v];
  return bytes_eq(t.path_arena + (pw >> 24) + EN_PATH, p + EN_PATH,
                  n - EN_PATH);
}

ZK_DEV void ent_load(const ZkTree& t, int64_t s, int64_t (&e)[HT_W]) {
  const uint4* q = (const uint4*)ht_ent(t, s);
#pragma unroll
  for (int k = 0; k < HT_W / 2; ++k) {
    const uint4 v = q[k];
    e[2 * k] = (int64_t)((uint64_t)v.x | (uint64_t)v.y << 32);
    e[2 * k + 1] = (int64_t)((uint64_t)v.z | (uint64_t)v.w << 32);
  }
}

// A hash val holds the node index (low 32 bits) and its slot offset / 16
// (high 32; slots are 16-byte aligned), plus one, so a hit needs no
// slot_off[v] read.  Live vals are > 0, the tombstone is -2, and 0 is an
// empty or being-published entry: an empty table is all zero bytes (a
// plain memset resets it; the -3 "empty" of before took a strided second
// pass).
ZK_DEV int64_t val_pack(int64_t v, int64_t slot) {
  return ((int64_t)(((uint64_t)slot >> 4) << 32) | v) + 1;
}
ZK_DEV int64_t val_node(int64_t x) { return (x - 1) & 0xFFFFFFFFll; }
// Order this thread's earlier global accesses before its later ones
// without a cache writeback or invalidate: a workgroup-scope fence is a
// wait for the outstanding accesses (the agent-scope atomics around it are
// served at L2, where the order then holds for other CUs too).  An
// agent-scope release / acquire writes back / invalidates caches, ~us each
// (MI355X_MICROARCH.md): in round 6's first expiry with them, 3.9 ms.
ZK_DEV void order_wait() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
}

// Tombstones: any val <= -2.  -2 is the plain one (DELETE, an insert's
// claim); a session expiry tags its own with its txn's zxid (ht_shift
// tells the holes of the launch it runs in from older tombstones).
// -1: an entry being moved (ht_shift).
constexpr int64_t VAL_TOMB = -2;
constexpr int64_t VAL_MOVING = -1;
ZK_DEV bool val_tomb(int64_t x) { return x <= VAL_TOMB; }
ZK_DEV int64_t tomb_tag(int64_t zx) {
  return VAL_TOMB - 1 - (zx & 0x3FFFFFFFFFFFll);
}
ZK_DEV int64_t val_slot(int64_t x) {
  return (int64_t)((uint64_t)(x - 1) >> 32) << 4;
}

// Node of path p (node -1 if absent), its slot offset and data length, and
// the hash entry (for a SET_DATA's data length update).
struct Found {
  int64_t node, slot;
  int32_t dlen;
  int64_t ent;
};

template <bool DLEN = false>
ZK_DEV Found tree_lookup(const ZkTree& t, const uint8_t* p, int32_t n) {
  (void)DLEN;
  const int64_t key = (int64_t)(path_hash(p, n) | 1ull);
  int64_t s = key & t.mask;
  for (int64_t probe = 0; probe <= t.mask; ++probe) {
    // one 64-byte entry per probe, loaded in one burst; entries being
    // written concurrently in this launch may read torn (val 0): not
    // found, as the batch contract allows for same-batch conflicts on one
    // path
    int64_t e[HT_W];
    ent_load(t, s, e);
    if (e[0] == 0) break;
    if (e[0] == key && e[1] > 0) {
      const int64_t node = val_node(e[1]);
      if (ent_is(t, e, node, p, n))
        return Found{node, val_slot(e[1]), (int32_t)(e[2] >> 32), s};
    }
    s = (s + 1) & t.mask;
  }
  return Found{-1, -1, 0, -1};
}

ZK_DEV int64_t tree_find(const ZkTree& t, const uint8_t* p, int32_t n) {
  return tree_lookup(t, p, n).node;
}

// Insert node `v` (path already in the arena).  Returns the existing node if
// the path is present (NODE_EXISTS), else v; TREE_INSERT_TIMEOUT when a
// concurrent claimer of the same key never published its value (the caller
// answers SYSTEMERROR rather than probing on and indexing the path twice).
constexpr int64_t TREE_INSERT_TIMEOUT = -4;
// REUSE: the caller knows no other request of the launch inserts this path
// (a SEQUENTIAL name numbered by zk_tree_seq_order: unique in its batch and
// above every number its parent gave before).  The probe still walks to the
// first empty slot (an existing node of that name answers NODE_EXISTS), but
// then the first tombstone passed on the way — of any key — is taken
// instead: entries of dead names are recycled by the next batch's names.
template <bool REUSE = false>
ZK_DEV int64_t tree_insert(const ZkTree& t, int64_t v, const uint8_t* p,
                           int32_t n, int32_t dl, int64_t so = -1) {
  const int64_t key = (int64_t)(path_hash(p, n) | 1ull);
  const int64_t pv = val_pack(v, so >= 0 ? so : t.store.slot_off[v]);
  int64_t s = key & t.mask;
  int64_t tomb = -1, tv = 0;
  for (int64_t probe = 0; probe <= t.mask; ++probe) {
    int64_t k0 = -1;                   // REUSE: the key loaded below
    if (REUSE) {
      // key and val in one round trip (the val only matters as a
      // tombstone to take, and the CAS on it decides)
      int64_t k = __hip_atomic_load(ht_key(t, s), __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
      const int64_t vv = __hip_atomic_load(ht_val(t, s), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
      if (k != 0 && k != key) {
        if (tomb < 0 && val_tomb(vv)) {
          tomb = s;
          tv = vv;
        }
        s = (s + 1) & t.mask;
        continue;
      }
      k0 = k;
      if (k == 0 && tomb >= 0) {
        // the name is absent: take the tombstone (val -2 -> 0 claims it;
        // a lookup in between sees a key with val 0 and probes on)
        if (atomicCAS((unsigned long long*)ht_val(t, tomb),
                      (unsigned long long)tv, 0ull) ==
            (unsigned long long)tv) {
          ent_fill(t, tomb, p, n, dl);
          __hip_atomic_store(ht_key(t, tomb), key, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(ht_val(t, tomb), pv, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          return v;
        }
        tomb = -1;                     // taken by another name: the empty
      }
    }
    // a plain load first: an occupied slot of another key (the usual probe
    // past a tombstone or a collision) costs a load, not an L2 atomic on
    // another line each (keys only ever go 0 -> key within a launch, so a
    // stale 0 just means the CAS below answers); REUSE has just loaded it
    int64_t k = REUSE ? k0 : *ht_key(t, s);
    if (!REUSE && k == 0 && tomb >= 0) {
      // the chain ends without the path: take the tombstone of its key
      // passed on the way (below)
      if (atomicCAS((unsigned long long*)ht_val(t, tomb),
                    (unsigned long long)tv, 0ull) == (unsigned long long)tv) {
        ent_fill(t, tomb, p, n, dl);
        __hip_atomic_store(ht_val(t, tomb), pv, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        return v;
      }
      tomb = -1;                       // taken meanwhile: the empty slot
    }
    if (k == 0)
      k = atomicCAS((unsigned long long*)ht_key(t, s), 0ull,
                    (unsigned long long)key);
    if (k == 0) {                         // claimed an empty slot
      ent_fill(t, s, p, n, dl);
      __hip_atomic_store(ht_val(t, s), pv, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      return v;
    }
    if (k == key) {
      int64_t w = 0;
      // The claimer may not have published the val yet: bounded wait.
      for (int spin = 0; spin < 1000000 && w == 0; ++spin)
        w = __hip_atomic_load(ht_val(t, s), __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT);
      if (w == 0) return TREE_INSERT_TIMEOUT;
      // the entry's path against this one: of a live entry, and of a
      // tombstone whose words hold a whole path (below)
      const bool live = w > 0;
      bool same = false;
      if (live || (!REUSE && n <= EN_PATH)) {
        int64_t e[HT_W];
        ent_load(t, s, e);
        same = ent_is(t, e, live ? val_node(w) : 0, p, n);
      }
      if (live && same) return val_node(w);
      // a tombstone of the same key.  The path may still live further down
      // the chain — another path of the same key went first, and this
      // tombstone is that one's (two paths of one 64-bit key are rare, but
      // a client can make them up) — so the first such tombstone is only
      // remembered and taken where the chain ends.  Claimed at once (0
      // while its words are rewritten, then published): REUSE, where the
      // caller vouches that the name is new, and a tombstone that still
      // holds this very path — a DELETE writes only the val, and a path of
      // up to EN_PATH bytes is whole in the entry — which is the path's
      // own: a path is indexed once and a moved entry's copy lies before
      // the tombstone it leaves, so the path lives nowhere after it (the
      // usual re-create of a deleted name: no probe to the chain's end)
      if (val_tomb(w)) {
        if (!REUSE && !same) {
          if (tomb < 0) {
            tomb = s;
            tv = w;
          }
        } else if (atomicCAS((unsigned long long*)ht_val(t, s),
                             (unsigned long long)w, 0ull) ==
                   (unsigned long long)w) {
          ent_fill(t, s, p, n, dl);
          __hip_atomic_store(ht_val(t, s), pv, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          return v;
        }
      }
    }
    s = (s + 1) & t.mask;
  }
  // no empty entry: the tombstone of this key, if the probe passed one
  if (!REUSE && tomb >= 0 &&
      atomicCAS((unsigned long long*)ht_val(t, tomb), (unsigned long long)tv,
                0ull) == (unsigned long long)tv) {
    ent_fill(t, tomb, p, n, dl);
    __hip_atomic_store(ht_val(t, tomb), pv, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    return v;
  }
  return -1;
}

// Tombstone node `v`'s hash entry.  Returns its slot for exactly one caller
// when several erase the same node concurrently (the CAS winner owns the
// free), else -1.
ZK_DEV int64_t tree_erase_slot(const ZkTree& t, int64_t v, const uint8_t* p,
                               int32_t n, int64_t tag = VAL_TOMB) {
  const int64_t key = (int64_t)(path_hash(p, n) | 1ull);
  int64_t s = key & t.mask;
  for (int64_t probe = 0; probe <= t.mask; ++probe) {
    // key and val in one round trip: a live val names its node alone (one
    // slot holds it at a time: a move parks the old slot at VAL_MOVING
    // first), and the CAS decides; the key only ends the probe
    const int64_t k = __hip_atomic_load(ht_key(t, s), __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
    const int64_t cur = __hip_atomic_load(ht_val(t, s), __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0) return -1;
    if (k == key && cur > 0 && val_node(cur) == v &&
        atomicCAS((unsigned long long*)ht_val(t, s), (unsigned long long)cur,
                  (unsigned long long)tag) == (unsigned long long)cur)
      return s;
    s = (s + 1) & t.mask;
  }
  return -1;
}

ZK_DEV bool tree_erase(const ZkTree& t, int64_t v, const uint8_t* p,
                       int32_t n) {
  return tree_erase_slot(t, v, p, n) >= 0;
}

// Tombstone reclaim, in a launch where nothing INSERTS (session expiry): a
// tombstone whose next slot is empty lies on no probe chain that reaches a
// live entry (linear probing: an entry's chain from its home slot is
// contiguous non-empty slots), so it can be emptied, and then so can the
// tombstones before it.  Concurrent erasers stay correct: a slot before a
// live entry of its chain never has an empty successor, and the only
// writer of a live entry's val is its own eraser.  Emptiness only grows in
// such a launch, so racing reclaims agree; a missed one is just a tombstone
// left for later.  Without it the storm's never-reused SEQUENTIAL names
// left 1M tombstones a step and the index was rebuilt every few hundred
// steps (round 5: 1.29 ms timed, 1.40 ms sustained).
ZK_DEV int64_t ht_reclaim(const ZkTree& t, int64_t s, bool succ_empty = false);

// Backward shift from the hole s (a tombstone this thread just made), in a
// launch where nothing inserts and the only erasers are those of `session`
// (session expiry): the first live entry after s whose probe chain covers s
// moves into it, its old slot becomes the hole, and so on; the last hole is
// then reclaimed.  Without it, a tombstone right before a live entry (a
// static node, another session's) could only go when an insert passed it,
// and at ~2/3 of the expired names the index filled up anyway (40 create /
// expire rounds: 0 -> 21 % of a 32K-entry table, still growing).  Entries
// of `session` are never moved (their erasers may be probing for them);
// every other live entry has no eraser in the launch, and its val is
// claimed (-3: no lookup matches it) while it moves, so one thread moves it
// and it is found at one slot or the other by any later launch.
//
// ht_shift_if is the shift with "this live entry has no eraser in the launch"
// as a functor over the entry's node (one load on the removal's dependent
// path, whatever decides it); ht_shift below is the one-session form.  The
// many-session close (tree_close.hip) marks the closing sessions' nodes in an
// array before its removal launch and asks that.
template <class Movable>
ZK_DEV void ht_shift_if(const ZkTree& t, int64_t s, int64_t tag,
                        Movable movable) {
  for (int moves = 0; moves < 16; ++moves) {
    // the first entry after the hole whose chain covers it: movable (any
    // live entry but `session`'s), or blocking (`session`'s, one moving or
    // being written); none before the run's end: no chain passes the hole
    int64_t j = (s + 1) & t.mask, cand = -1, cv = 0;
    bool blocked = true, tombs = false;
    for (int k = 0; k < 64; ++k, j = (j + 1) & t.mask) {
      // an empty key ends the run whatever the val: the usual first slot
      // (a sparse index) costs one round trip
      if (__hip_atomic_load(ht_key(t, j), __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT) == 0) {
        blocked = tombs;
        break;
      }
      // val, key, val: a hole another thread fills between the loads
      // would pair its old key with the new val (the key decides whether
      // the entry covers s), so a val that changed blocks
      const int64_t v1 = __hip_atomic_load(ht_val(t, j), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
      order_wait();
      const int64_t key = __hip_atomic_load(ht_key(t, j), __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
      if (key == 0) {
        // (a tombstone on the way may be another thread's hole that an
        // entry covering s is moving into right now — seen here as the
        // tombstone before, and at its old slot as the tombstone after:
        // then s is not emptied)
        blocked = tombs;
        break;
      }
      order_wait();
      const int64_t val = __hip_atomic_load(ht_val(t, j), __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
      if (val != v1) break;                         // (blocking)
      if (val_tomb(val)) {                          // tombstone
        if (val == tag) tombs = true;               // (of this launch)
        continue;
      }
      if (val > 0 &&
          ((j - (key & t.mask)) & t.mask) < ((j - s) & t.mask))
        continue;                                   // home after the hole
      if (val > 0 && movable(val_node(val))) {
        cand = j;
        cv = val;
      }
      break;                                        // (else: blocking)
    }
    if (cand < 0) {
      if (!blocked) {
        // nothing reaches past the hole: empty it, then the tombstones
        // before it (their successor is now empty)
        __hip_atomic_store(ht_val(t, s), (int64_t)0, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        order_wait();
        __hip_atomic_store(ht_key(t, s), (int64_t)0, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        // (s's key is this thread's 0 — an empty slot stays empty in the
        // launch — so the reclaim's first step reads only the val before;
        // it is read after the run's end was seen empty, as it must be)
        ht_reclaim(t, (s - 1) & t.mask, true);
      }
      return;
    }
    if (atomicCAS((unsigned long long*)ht_val(t, cand), (unsigned long long)cv,
                  (unsigned long long)VAL_MOVING) != (unsigned long long)cv)
      return;
    if (atomicCAS((unsigned long long*)ht_val(t, s), (unsigned long long)tag,
                  0ull) != (unsigned long long)tag) {
      __hip_atomic_store(ht_val(t, cand), cv, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    int64_t e[HT_W];
    ent_load(t, cand, e);
    int64_t* d = ht_ent(t, s);
#pragma unroll
    for (int w = 2; w < HT_W; ++w) d[w] = e[w];
    __hip_atomic_store(ht_key(t, s), e[0], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    order_wait();                       // the key before the val ...
    __hip_atomic_store(ht_val(t, s), cv, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    order_wait();                       // ... and the copy before the vacate
    __hip_atomic_store(ht_val(t, cand), tag, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    s = cand;                                       // the new hole
  }
  ht_reclaim(t, s);
}

ZK_DEV void ht_shift(const ZkTree& t, int64_t s, int64_t session,
                     int64_t tag) {
  ht_shift_if(t, s, tag,
              [&](int64_t node) { return t.eph[node] != session; });
}

ZK_DEV int64_t ht_reclaim(const ZkTree& t, int64_t s, bool succ_empty) {
  int64_t n = 0;
  for (int k = 0; k < 64; ++k) {
    const int64_t nx = (s + 1) & t.mask;
    if (succ_empty && k == 0) {
      if (!val_tomb(__hip_atomic_load(ht_val(t, s), __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT)))
        break;
      __hip_atomic_store(ht_val(t, s), (int64_t)0, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      order_wait();
      __hip_atomic_store(ht_key(t, s), (int64_t)0, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      ++n;
      s = (s - 1) & t.mask;
      continue;
    }
    // the successor's key first, the val after it: a val read before an
    // entry moved into s (from past nx, which was emptied after) paired
    // with the emptied key would drop the live entry — both loads in one
    // round trip lost a storm node in a 400-step run
    if (__hip_atomic_load(ht_key(t, nx), __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT) != 0)
      break;
    if (!val_tomb(__hip_atomic_load(ht_val(t, s), __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT)))
      break;
    // val first: a reader between the two stores sees a key with val 0
    // (no match, probe on), then the empty key (end of chain)
    __hip_atomic_store(ht_val(t, s), (int64_t)0, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    order_wait();
    __hip_atomic_store(ht_key(t, s), (int64_t)0, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    ++n;
    s = (s - 1) & t.mask;
  }
  return n;
}

// tree_erase at the entry a lookup just found (slot s): no second probe.
// The CAS against the live val the lookup saw keeps one winner among
// concurrent erasers of the node; a lost race answers like tree_erase.
ZK_DEV bool tree_erase_at(const ZkTree& t, int64_t s, int64_t v) {
  if (s < 0) return false;
  const int64_t cur = __hip_atomic_load(ht_val(t, s), __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
  return cur > 0 && val_node(cur) == v &&
         atomicCAS((unsigned long long*)ht_val(t, s), (unsigned long long)cur,
                   (unsigned long long)VAL_TOMB) == (unsigned long long)cur;
}

// ---- watches (one-shot, per watcher slot) ---------------------------------
// A path-keyed table beside the tree (lib/zk-session.js:482-526 describes
// the server semantics the client relies on): key = path
// hash | 1 (0 = empty, linear probing, entries are removed only by the
// rebuild, zk_watch_rebuild), two 64-bit masks per entry — the data watches
// (GET_DATA / EXISTS with watch=1; an EXISTS on a missing path is
// ZooKeeper's "exist" watch, kept in the same set like the server's
// dataWatches) and the child watches — one bit per watcher slot (<= 64
// sessions of the server).  Firing is an atomic exchange with 0: one-shot,
// and each watcher of a path is notified exactly once even when several
// writes of a batch hit the path (the first takes the mask).  Paths are
// keyed, not nodes, so a watch on a missing path waits for its creation.
//
// Two paths of one key (hash twins) are told apart by a second word per
// entry, tag = an independent 64-bit hash of the path | 1, folded in the
// same pass over the bytes (path_hash2).  The claimer of a key publishes
// its tag with atomicCAS(0 -> mine); nobody waits: an armer that reads 0
// tries the same CAS (result 0 or mine: the entry is this path's, anything
// else: a twin's, probe on), a fire that reads 0 treats the entry as an
// insert of the launch it runs in and misses it, as the batch contract
// allows.  Residual: two paths equal in BOTH 64-bit hashes (and in length,
// which both fold) still alias; no path bytes are kept or compared.
enum : int { WK_DATA = 0, WK_CHILD = 1 };
// counters behind the masks (wt_mask[2 * (wt_hmask + 1) + WS_*])
enum : int { WS_LOST = 0, WT_STATS = 8 };
// notification types (lib/zk-consts.js NOTIFICATION_TYPE)
enum : int32_t { NT_CREATED = 1, NT_DELETED = 2, NT_DATA_CHANGED = 3,
                 NT_CHILDREN_CHANGED = 4 };
constexpr int WT_REC = 5;    // per request: m_path, m_path_child, m_parent,
                             // path word of the node, of its parent

// path_hash and the tag of the same bytes in one pass (other multipliers,
// another seed: a pair built to collide in one does not in the other)
ZK_DEV uint64_t path_hash2(const uint8_t* p, int32_t n, uint64_t* tag) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
  uint64_t g = 0xD6E8FEB86659FD93ull + (uint64_t)n;
  int32_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w; __builtin_memcpy(&w, p + i, 8);
    h = (h ^ w) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
    g = (g + w) * 0x9FB21C651E98DF25ull;
    g ^= g >> 29;
  }
  if (i < n) {
    uint64_t w = 0;
    for (int32_t k = 0; i + k < n; ++k) w |= (uint64_t)p[i + k] << (8 * k);
    h = (h ^ w) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
    g = (g + w) * 0x9FB21C651E98DF25ull;
    g ^= g >> 29;
  }
  h ^= h >> 33;
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  g ^= g >> 31;
  g *= 0xBF58476D1CE4E5B9ull;
  g ^= g >> 30;
  *tag = g | 1ull;
  return h;
}

// (key and tag side by side: the second word of a probe is in the line the
// first one fetched)
ZK_DEV int64_t* wt_tag(const ZkTree& t, int64_t s) {
  return &t.wt_key[2 * s + 1];
}

ZK_DEV int64_t wt_slot(const ZkTree& t, uint64_t key, uint64_t tag,
                       bool insert) {
  int64_t s = (int64_t)key & t.wt_hmask;
  for (int64_t probe = 0; probe <= t.wt_hmask; ++probe) {
    int64_t k = __hip_atomic_load(&t.wt_key[2 * s], __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0) {
      if (!insert) return -1;
      k = (int64_t)atomicCAS((unsigned long long*)&t.wt_key[2 * s], 0ull,
                             (unsigned long long)key);
      if (k == 0) k = (int64_t)key;
    }
    if (k == (int64_t)key) {
      int64_t g = __hip_atomic_load(wt_tag(t, s), __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
      if (g == 0 && insert) {
        g = (int64_t)atomicCAS((unsigned long long*)wt_tag(t, s), 0ull,
                               (unsigned long long)tag);
        if (g == 0) g = (int64_t)tag;
      }
      if (g == (int64_t)tag) return s;
    }
    s = (s + 1) & t.wt_hmask;
  }
  return -1;                                      // table full
}

ZK_DEV void wt_arm(const ZkTree& t, const uint8_t* p, int32_t n, int kind,
                   int32_t wslot) {
  if (t.wt_key == nullptr || wslot < 0 || wslot > 63) return;
  uint64_t tag;
  const uint64_t key = path_hash2(p, n, &tag) | 1ull;
  const int64_t s = wt_slot(t, key, tag, true);
  if (s >= 0) atomicOr(&t.wt_mask[2 * s + kind], 1ull << wslot);
  else atomicAdd(&t.wt_mask[2 * (t.wt_hmask + 1) + WS_LOST], 1ull);
}

// The entry of a path for wt_fire_at (-1: none): one probe for a write that
// fires both of a path's masks.
ZK_DEV int64_t wt_find(const ZkTree& t, const uint8_t* p, int32_t n) {
  if (t.wt_key == nullptr) return -1;
  uint64_t tag;
  const uint64_t key = path_hash2(p, n, &tag) | 1ull;
  return wt_slot(t, key, tag, false);
}

ZK_DEV uint64_t wt_fire_at(const ZkTree& t, int64_t s, int kind) {
  if (s < 0) return 0;
  unsigned long long* m = &t.wt_mask[2 * s + kind];
  if (__hip_atomic_load(m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
    return 0;
  return atomicExch(m, 0ull);
}

ZK_DEV uint64_t wt_fire(const ZkTree& t, const uint8_t* p, int32_t n,
                        int kind) {
  return wt_fire_at(t, wt_find(t, p, n), kind);
}

// Node v's path from its path word.
ZK_DEV const uint8_t* node_path(const ZkTree& t, int64_t pw) {
  return t.path_arena + (pw >> 24);
}
ZK_DEV int32_t pw_len(int64_t pw) { return (int32_t)(pw & 0xFFFFFF); }

ZK_DEV void fill_stat(uint8_t* st, int64_t cz, int64_t mz, int64_t ct,
                      int64_t mt, int32_t ver, int32_t cver, int32_t aver,
                      int64_t owner, int32_t dlen, int32_t nkids, int64_t pz) {
  st_be64(st + 0, cz); st_be64(st + 8, mz); st_be64(st + 16, ct);
  st_be64(st + 24, mt); st_be32(st + 32, ver); st_be32(st + 36, cver);
  st_be32(st + 40, aver); st_be64(st + 44, owner); st_be32(st + 52, dlen);
  st_be32(st + 56, nkids); st_be64(st + 60, pz);
}

// The parent counters (cversion << 32 | numChildren in one word, so a
// child's create or delete moves both with one device-scope atomic: on the
// multi-XCD part each is a trip to the coherence point).  numChildren never
// goes negative, so a signed add of (dc << 32) + dk never borrows across.
ZK_DEV int64_t cn_pack(int32_t cver, int32_t nchild) {
  return (int64_t)((uint64_t)(uint32_t)cver << 32 | (uint32_t)nchild);
}
ZK_DEV int32_t cn_cver(int64_t x) { return (int32_t)((uint64_t)x >> 32); }
ZK_DEV int32_t cn_nchild(int64_t x) { return (int32_t)(uint32_t)x; }
ZK_DEV int64_t cn_add(const ZkTree& t, int64_t v, int32_t dc, int32_t dk) {
  return (int64_t)atomicAdd((unsigned long long*)&t.cn[v],
                            (unsigned long long)(((int64_t)dc << 32) + dk));
}

// ---- parent bookkeeping ----------------------------------------------------
// Child added (dkids = 1) / removed (-1) under `par` by the txn `zx`;
// `bump_cver` is false when a SEQUENTIAL create already took the cversion.
ZK_DEV void parent_touch(const ZkTree& t, int64_t par, int32_t dkids,
                         bool bump_cver, int64_t zx) {
  cn_add(t, par, bump_cver ? 1 : 0, dkids);
  atomicMax((unsigned long long*)&t.pzxid[par], (unsigned long long)zx);
}

// Put every distinct parent this block touched on the dirty list once
// (block-uniform call).
ZK_DEV void wave_mark_dirty(const ZkTree& t, int64_t par) {
  bool first = false;
  if (par >= 0 && __hip_atomic_load(&t.dirty[par], __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT) == 0)
    first = atomicExch(&t.dirty[par], 1) == 0;
  const int64_t k = block_ticket(&t.counters[TC_DIRTY], first);
  if (first) t.dirty_list[k] = par;
}

// Free `v` (block-uniform call; `v < 0` = nothing to free).
ZK_DEV void wave_free(const ZkTree& t, int64_t v,
                      unsigned long long* count = nullptr) {
  if (v >= 0) t.node_parent[v] = NODE_FREE;
  const int64_t k = block_ticket(&t.counters[TC_FREE_TAIL], v >= 0, count);
  if (v >= 0) t.free_list[k % t.free_cap] = v;
}

// wave_mark_dirty with the parent's flag already loaded (flag: its value;
// nonzero: on the list, or no parent)
ZK_DEV void wave_mark_dirty_at(const ZkTree& t, int64_t par, int32_t flag) {
  const bool first = par >= 0 && flag == 0 && atomicExch(&t.dirty[par], 1) == 0;
  const int64_t k = block_ticket(&t.counters[TC_DIRTY], first);
  if (first) t.dirty_list[k] = par;
}

// ---- host side: launches shared by the tree's files -------------------------
// A kernel is launched from the file that defines it (the build has no
// relocatable device code); the other tree files reach these four through
// plain host functions.

// One tree_serve_k launch (tree.hip).  The requests are K12's table (q), or,
// with q null, K1's frames (foff / flen), parsed in the kernel — read_only
// then picks the RO instance.  rank .. snap_top default to the unordered
// serve's values.
struct ServeLaunch {
  const ZkTree* tree = nullptr;
  const uint8_t* rx = nullptr;
  const ZkReqOut* q = nullptr;
  const int64_t* foff = nullptr;
  const int32_t* flen = nullptr;
  const int64_t* n_dev = nullptr;
  int64_t ncap = 0;
  const ZkServeOut* out = nullptr;
  int64_t session = 0, now_ms = 0;
  const uint8_t* rank = nullptr;
  int32_t pass = 0, last_pass = 1;
  int64_t snap_base = 0, snap_cap = 0;
  int64_t* snap_top = nullptr;
  int32_t wslot = -1;
  int64_t* fired = nullptr;
  int32_t read_only = 0;
  // after a rows-deferred K1 scan: its tile lists, and the frame table the
  // serve writes the rows to (foff / flen unused)
  const ZkFrameTiles* tiles = nullptr;
  int64_t* rows_off = nullptr;
  int32_t* rows_len = nullptr;
  // a session batch (tree_sess.hip; set, it picks the serve's MS instances):
  // the segment table.  session / wslot above are then unused
  const ZkSegs* segs = nullptr;
  // the ordered passes of a session batch served with deferral (q and rank
  // set): the MS instance that keeps a deferred SEQUENTIAL create's number
  int32_t defer = 0;
};
int serve_launch(const ServeLaunch& s, hipStream_t st);

// tree_finish_k after a serve / expire launch (tree.hip): zxid += *n_dev, or
// bump when n_dev is null.
int finish_launch(const ZkTree* t, const int64_t* n_dev, int64_t bump,
                  int32_t publish, hipStream_t st);

// tree_digest_k alone (tree.hip): out[0] += the digest sum of the live nodes,
// out[1] += their number (the caller zeroes them); no census of the index.
int digest_launch(const ZkTree* t, unsigned long long* out, hipStream_t st);

// ord_bscan_k (tree_order.hip): bsum[0, nb) -> its exclusive prefix, in place.
int bscan_launch(int64_t* bsum, int64_t nb, hipStream_t st);

}  // namespace zk
