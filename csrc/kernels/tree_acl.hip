// The GPU tree's ACL path: the ACL store beside the tree (ZkAclTable,
// zk_abi.h), the pass that records a batch's CREATE ACLs and the GET_ACL
// serve (the tree: zk_tree.h).
#include "zk_acl.h"
#include "zk_sess.h"
#include "zk_setacl_dev.h"

namespace zk {

// ---- the store ---------------------------------------------------------------
// node_acl[v] names node v's ACL vector in the arena: offset << 24 | bytes,
// the vector in WIRE format (be32 count + entries, the very bytes of the
// CREATE request), so a GET_ACL reply copies it.  Every vector is stored
// once: an open-addressing index (key = 64-bit content hash | 1, val = the
// arena word) interns them at create time; the read path never touches it.
// The words and counters: zk_acl.h.

// One workspace for both passes (they run one after the other on a stream).
struct AclWs {
  int64_t* ctr;                 // [8] 0: the GET_ACL stream overflowed
  int32_t* xid;                 // [ncap] get
  int32_t* err;                 // [ncap] get
  int32_t* slot;                // [ncap] record: index slot / AS_*
  int32_t* alen;                // [ncap] record: bytes of the request's ACL
  int64_t* aoff;                // [ncap] record: its offset in rx
  int64_t* word;                // [ncap] get: the node's ACL word
  int64_t* nslot;               // [ncap] get: the node's slot offset
  int64_t* sizes;               // [ncap] get: frame bytes
  int64_t* scan;                // zk_scan_workspace(ncap)
};

// ---- recording a batch's CREATE ACLs -----------------------------------------
// Two launches after the serve, so that no lane ever waits inside a kernel
// for another lane's store:
//  1. acl_intern_k, a thread per request: a successful CREATE re-parses its
//     frame and hashes its ACL bytes; the wave then claims or finds the key
//     with ONE probe, walked by the whole wave, per distinct hash (a ballot
//     loop over equal hashes, as list_sweep_k does per parent: a storm batch
//     is one ACL a million times).  The probe loop has one exit and takes
//     the slot from its cursor after it (an earlier form, a leader-only loop
//     with a `continue` past an inlined compare, came out of the compiler
//     with the found slot lost on exactly the compared path).  An entry of
//     an EARLIER batch (its bytes end below the arena top that batch left)
//     is compared byte for byte while probing, and a
//     mismatch probes on; an entry of this batch is taken on its hash alone
//     (its bytes may still be on their way).  The claimers of a wave take
//     their entry numbers and arena bytes with one atomic each (wave_bytes),
//     copy the vector and publish the arena word, or ACL_LOST when the store
//     has no room.  Every lane records the slot it landed on.
//  2. acl_bind_k: the now-published word of that slot, the stored bytes
//     compared with the request's (two new vectors of one batch with one
//     hash: the loser is lost), node_acl[node].  A node index is created at
//     most once per batch (freed nodes are published by the finish and
//     popped from the next batch on), so node_acl[v] has one writer.
__global__ __launch_bounds__(TR_T) void acl_intern_k(
    ZkAclTable a, const uint8_t* __restrict__ rx,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap,
    const int32_t* __restrict__ r_op, const int32_t* __restrict__ r_err,
    const int64_t* __restrict__ r_node, AclWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const int lane = lane_id();
  int32_t slot = AS_NONE, len = 0;
  int64_t off = -1;
  uint64_t h = 0;
  if (i < ncap && i < *n_dev && r_op[i] == OP_CREATE && r_err[i] == ERR_OK) {
    const int64_t node = r_node[i];
    if (node >= 0 && node < a.cap) {
      slot = AS_LOST;
      const int64_t base = foff[i], L = flen[i];
      const ReqFields rq = parse_request(rx, base, L);
      if (rq.status == ST_OK && rq.op == OP_CREATE && rq.vc > 0) {
        const int64_t s = skip_acl(rx + rq.voff, base + L - rq.voff, rq.vc);
        if (s >= 0 && 4 + s < ACL_LEN_MAX) {
          off = rq.voff - 4;
          len = (int32_t)(4 + s);
          h = path_hash(rx + off, len) | 1ull;
        }
      }
    }
  }
  const bool need = off >= 0;
  const int64_t old_top = a.ctr[AC_OLD_TOP];
  bool claimed = false;
  int64_t cslot = -1;
  uint64_t todo = __ballot(need);
  while (todo != 0) {
    const int first = __ffsll((unsigned long long)todo) - 1;
    const uint64_t h0 = __shfl(h, first, 64);
    const bool mine = need && h == h0;
    const uint64_t m = __ballot(mine);
    // The whole wave walks the leader's probe chain (wave-uniform control
    // flow: every value that decides a branch is the leader's, broadcast);
    // the leader alone claims, and the lanes share a byte comparison.
    const int64_t loff = __shfl(off, first, 64);
    const int32_t llen = __shfl(len, first, 64);
    int64_t s = (int64_t)(h0 >> 8) & a.hmask;
    bool hit = false;
    for (int64_t probe = 0; probe <= a.hmask; ++probe) {
      // a plain (cached) load first: the usual hit is an earlier batch's
      // entry, and a million creates with one ACL would all go to one L2
      // line with atomic loads (keys only go 0 -> key, words 0 -> word, so a
      // stale 0 just sends the lane to the atomic)
      int64_t k = a.key[s];
      if (k == 0) k = ld_relaxed(&a.key[s]);
      k = __shfl(k, first, 64);
      bool take = false, fresh = false;
      if (k == 0) {
        if (lane == first)
          k = (int64_t)atomicCAS((unsigned long long*)&a.key[s], 0ull,
                                 (unsigned long long)h0);
        k = __shfl(k, first, 64);
        fresh = take = k == 0;                     // claimed an empty slot
      }
      if (!take && k == (int64_t)h0) {
        int64_t v = a.val[s];
        if (v == 0) v = ld_relaxed(&a.val[s]);
        v = __shfl(v, first, 64);
        bool other = false;
        if (acl_word_ok(a, v) && acl_off(v) + acl_len(v) <= old_top) {
          // an earlier batch's entry: its bytes against the leader's
          other = acl_len(v) != llen;
          if (!other) {
            const uint8_t* x = a.arena + acl_off(v);
            const uint8_t* y = rx + loff;
            bool d = false;
            for (int32_t b = lane; b < llen; b += 64) d |= x[b] != y[b];
            other = __ballot(d) != 0;
          }
        }
        take = !other;                             // (another vector: on)
      }
      if (take) {
        if (fresh && lane == first) {
          claimed = true;
          cslot = s;
        }
        hit = true;
        break;
      }
      s = (s + 1) & a.hmask;
    }
    const int32_t found = hit ? (int32_t)s : AS_LOST;   // (a full index)
    if (mine) slot = found;
    todo &= ~m;
  }
  // the wave's claimers: entry numbers, arena bytes, the copy, the word
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
        copy_bytes(a.arena + o, rx + off, len);
        word = (o << 24) | (int64_t)len;
      }
      __hip_atomic_store(&a.val[cslot], word, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    // (entries count the stored vectors: the refused claims go back)
    const uint64_t fail = __ballot(claimed && !ok);
    if (fail != 0 && lane == lead)
      atomicAdd((unsigned long long*)&a.ctr[AC_ENT],
                (unsigned long long)(-(long long)__popcll(fail)));
  }
  if (i < ncap) {
    w.slot[i] = slot;
    w.alen[i] = len;
    w.aoff[i] = off;
  }
}

__global__ __launch_bounds__(TR_T) void acl_bind_k(
    ZkAclTable a, const uint8_t* __restrict__ rx,
    const int64_t* __restrict__ n_dev, int64_t ncap,
    const int64_t* __restrict__ r_node, AclWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  // (nothing claims arena bytes in this launch: the top is this batch's)
  if (i == 0) a.ctr[AC_OLD_TOP] = a.ctr[AC_TOP];
  bool lost = false;
  if (i < ncap && i < *n_dev) {
    const int32_t slot = w.slot[i];
    if (slot != AS_NONE) {
      int64_t word = ACL_LOST;
      if (slot >= 0 && (int64_t)slot <= a.hmask) {
        const int64_t v = a.val[slot];
        const int32_t len = w.alen[i];
        if (acl_word_ok(a, v) && acl_len(v) == len &&
            bytes_eq(a.arena + acl_off(v), rx + w.aoff[i], len))
          word = v;
      }
      const int64_t node = r_node[i];
      if (node >= 0 && node < a.cap) {
        a.node_acl[node] = word;
        lost = word == ACL_LOST;
      }
    }
  }
  const uint64_t lm = __ballot(lost);
  if (lm != 0 && lane_id() == __ffsll((unsigned long long)lm) - 1)
    atomicAdd((unsigned long long*)&a.ctr[AC_LOST],
              (unsigned long long)__popcll(lm));
}

// ---- GET_ACL -------------------------------------------------------------------
// The shape of zk_tree_list without the sweeps:
//  1. acl_size_k, a thread per request: parse, look the path up, read
//     node_acl[node] (the one dependent trip past the lookup) and size the
//     reply: header only for an error, else header + ACL bytes + Stat;
//  2. the device-wide scan and acl_total_k: offsets, the total against the
//     output capacity (K13's convention), the terminator;
//  3. acl_write_k, EIGHT lanes per reply: the reply is header (20 bytes) +
//     ACL vector (27 for the open ACL) + Stat (68) = 115 bytes, three
//     contiguous sources.  A thread per reply (K13's GSink) makes every
//     store instruction of a wave touch 64 lines 115 bytes apart.  Here lane
//     l of a group moves the 16-byte pieces l, l + 8, ... of its reply, so a
//     group's stores cover one reply and a wave's one contiguous span of 8
//     replies (~920 bytes, close to the 1 KiB a wave instruction moves at
//     best), with 16-byte loads from the arena and the slot wherever a piece
//     lies inside one source; only the pieces across a seam and the tail go
//     by dwords and bytes.  Staging the block's span in LDS (K13's LSink)
//     coalesces as well but costs the LDS image, a barrier and the swizzle
//     for records that are plain copies; the part-wave needs none of them,
//     and a long vector (up to 16 MiB) simply takes more trips.
// MS (acl_size_sess_k): the GET_ACL frames of a session batch of any op mix
// (GpuServer.serve_sessions_mixed).  A frame its segment's row of the table M
// refuses (zk_sess.h sess_refusal) is sized header-only with the xid alone
// read: nothing is parsed or looked up.  Refusal is per lane and *M.bad
// grid-uniform; acl_total_k and acl_write_k see an error request.
__global__ __launch_bounds__(TR_T) void acl_size_k(
    ZkTree t, ZkAclTable a, const uint8_t* __restrict__ rx,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap, AclWs w) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= ncap) return;
  int32_t err = ERR_OK, xid = 0;
  int64_t word = 0, nslot = -1, sz = 0;
  if (i < *n_dev) {
    const ReqFields rq = parse_request(rx, foff[i], flen[i]);
    xid = rq.xid;
    if (rq.status != ST_OK) {
      err = ERR_BAD_ARGUMENTS;
    } else if (rq.op != OP_GET_ACL) {
      err = ERR_UNIMPLEMENTED;
    } else {
      const Found f = tree_lookup(t, rx + rq.poff, rq.pl);
      if (f.node < 0 || f.node >= a.cap || f.node >= t.store.cap) {
        err = ERR_NO_NODE;              // ("/" has no node in this tree)
      } else {
        word = a.node_acl[f.node];
        nslot = f.slot;
        if (!acl_word_ok(a, word) || nslot < 0 ||
            nslot + STAT_BYTES > t.slab_cap)
          err = ERR_SYSTEM;             // a lost binding
      }
    }
    sz = 4 + 16 + (err == ERR_OK ? (int64_t)acl_len(word) + STAT_BYTES : 0);
  }
  w.xid[i] = xid;
  w.err[i] = err;
  w.word[i] = word;
  w.nslot[i] = nslot;
  w.sizes[i] = sz;
}

// The MS instance.  (A kernel of its own text: acl_size_k as an instance of a
// shared body, however its parameters were passed, came out of the compiler
// 16 to 32 bytes of code away from what it was; tools/kernel_resources.py
// --diff.)
__global__ __launch_bounds__(TR_T) void acl_size_sess_k(
    ZkTree t, ZkAclTable a, const uint8_t* __restrict__ rx,
    const int64_t* __restrict__ foff, const int32_t* __restrict__ flen,
    const int64_t* __restrict__ n_dev, int64_t ncap, AclWs w, SegTable M) {
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  if (i >= ncap) return;
  int32_t err = ERR_OK, xid = 0;
  int64_t word = 0, nslot = -1, sz = 0;
  if (i < *n_dev) {
    err = sess_refusal(M.bad, M.seg_state, M.S, M.f_seg[i]);
    if (err != ERR_OK) {
      xid = sess_xid(rx, foff[i], flen[i]);
    } else {
      const ReqFields rq = parse_request(rx, foff[i], flen[i]);
      xid = rq.xid;
      if (rq.status != ST_OK) {
        err = ERR_BAD_ARGUMENTS;
      } else if (rq.op != OP_GET_ACL) {
        err = ERR_UNIMPLEMENTED;
      } else {
        const Found f = tree_lookup(t, rx + rq.poff, rq.pl);
        if (f.node < 0 || f.node >= a.cap || f.node >= t.store.cap) {
          err = ERR_NO_NODE;
        } else {
          word = a.node_acl[f.node];
          nslot = f.slot;
          if (!acl_word_ok(a, word) || nslot < 0 ||
              nslot + STAT_BYTES > t.slab_cap)
            err = ERR_SYSTEM;             // a lost binding
        }
      }
    }
    sz = 4 + 16 + (err == ERR_OK ? (int64_t)acl_len(word) + STAT_BYTES : 0);
  }
  w.xid[i] = xid;
  w.err[i] = err;
  w.word[i] = word;
  w.nslot[i] = nslot;
  w.sizes[i] = sz;
}

__global__ void acl_total_k(int64_t* __restrict__ total, int64_t out_cap,
                            int32_t* __restrict__ err, int32_t terminate,
                            uint8_t* __restrict__ out, AclWs w) {
  const int64_t T = *total;
  const bool over = T > out_cap;
  w.ctr[0] = over ? 1 : 0;
  *err = over ? 2 : 0;
  if (over) *total = 0;
  if (!over && terminate && T + 4 <= out_cap) st_be32(out + T, -1);
}

constexpr int ACL_GROUP = 8;                       // lanes per reply
constexpr int64_t ACL_HEAD = 4 + 16;

__global__ __launch_bounds__(TR_T) void acl_write_k(
    ZkTree t, ZkAclTable a, const int64_t* __restrict__ n_dev, int64_t ncap,
    AclWs w, const int64_t* __restrict__ rec_off, uint8_t* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const int64_t i = g / ACL_GROUP;
  const int l = (int)(g % ACL_GROUP);
  if (i >= ncap || i >= *n_dev || w.ctr[0] != 0) return;
  uint8_t* o = out + rec_off[i];
  const int64_t R = w.sizes[i];
  const int32_t err = w.err[i];
  const int64_t word = w.word[i];
  const int64_t A = err == ERR_OK ? (int64_t)acl_len(word) : 0;
  const uint8_t* ap = a.arena + (err == ERR_OK ? acl_off(word) : 0);
  const uint8_t* sp = t.store.slab + (err == ERR_OK ? w.nslot[i] : 0);
  const int64_t zx = t.counters[TC_ZXID];          // reads see the batch's base
  const uint32_t head[5] = {
      bswap32((uint32_t)(R - 4)), bswap32((uint32_t)w.xid[i]),
      bswap32((uint32_t)((uint64_t)zx >> 32)), bswap32((uint32_t)zx),
      bswap32((uint32_t)err)};
  const int64_t seam = ACL_HEAD + A;               // the Stat's first byte
  for (int64_t p = (int64_t)l * 16; p < R; p += ACL_GROUP * 16) {
    if (p >= ACL_HEAD && p + 16 <= seam) {
      uint4 x;
      __builtin_memcpy(&x, ap + (p - ACL_HEAD), 16);
      __builtin_memcpy(o + p, &x, 16);
      continue;
    }
    if (p >= seam && p + 16 <= R) {
      uint4 x;
      __builtin_memcpy(&x, sp + (p - seam), 16);
      __builtin_memcpy(o + p, &x, 16);
      continue;
    }
    const int64_t pe = min(p + 16, R);
    for (int64_t q = p; q < pe; q += 4) {
      uint32_t x;
      if (q < ACL_HEAD) {
        // (a select chain, not an indexed read: head[] stays in registers)
        const int k = (int)(q >> 2);
        x = k == 0 ? head[0] : k == 1 ? head[1] : k == 2 ? head[2]
            : k == 3 ? head[3] : head[4];
        __builtin_memcpy(o + q, &x, 4);
      } else if (q + 4 <= seam) {
        __builtin_memcpy(&x, ap + (q - ACL_HEAD), 4);
        __builtin_memcpy(o + q, &x, 4);
      } else if (q >= seam && q + 4 <= R) {
        __builtin_memcpy(&x, sp + (q - seam), 4);
        __builtin_memcpy(o + q, &x, 4);
      } else {
        const int64_t qe = min(q + 4, R);
        for (int64_t b = q; b < qe; ++b)
          o[b] = b < seam ? ap[b - ACL_HEAD] : sp[b - seam];
      }
    }
  }
}

}  // namespace zk

extern "C" {

// Workspace of zk_tree_acl_record / zk_tree_acl_get for up to ncap requests
// (bytes; 16-aligned parts).  Nothing in it needs zeroing.
static int64_t acl_layout(int64_t ncap, uint8_t* ws, zk::AclWs* w) {
  auto a16 = [](int64_t x) { return (x + 15) & ~(int64_t)15; };
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    uint8_t* p = ws != nullptr ? ws + o : nullptr;
    o += a16(bytes);
    return p;
  };
  uint8_t* ctr = take(64);
  uint8_t* i32s[4];
  for (auto& p : i32s) p = take(ncap * 4);
  uint8_t* i64s[4];
  for (auto& p : i64s) p = take(ncap * 8);
  uint8_t* scan = take(zk_scan_workspace(ncap > 0 ? ncap : 1) * 8);
  if (w != nullptr) {
    w->ctr = (int64_t*)ctr;
    w->xid = (int32_t*)i32s[0];
    w->err = (int32_t*)i32s[1];
    w->slot = (int32_t*)i32s[2];
    w->alen = (int32_t*)i32s[3];
    w->aoff = (int64_t*)i64s[0];
    w->word = (int64_t*)i64s[1];
    w->nslot = (int64_t*)i64s[2];
    w->sizes = (int64_t*)i64s[3];
    w->scan = (int64_t*)scan;
  }
  return o;
}

int64_t zk_tree_acl_workspace(int64_t ncap) {
  return acl_layout(ncap > 0 ? ncap : 0, nullptr, nullptr);
}

static bool acl_table_ok(const ZkAclTable* a) {
  return a->cap > 0 && a->arena_cap > 0 && a->hmask >= 0 &&
         (a->hmask & (a->hmask + 1)) == 0;
}

// Record the ACLs of the batch's successful CREATEs (r_op / r_err / r_node:
// the reply descriptors of the serve that just ran on this stream; foff /
// flen: the batch's request frames).  Two launches, no host read.
int zk_tree_acl_record(const ZkAclTable* a, const uint8_t* rx,
                       const int64_t* foff, const int32_t* flen,
                       const int64_t* n_dev, int64_t ncap,
                       const int32_t* r_op, const int32_t* r_err,
                       const int64_t* r_node, uint8_t* ws, int64_t ws_bytes,
                       hipStream_t st) {
  if (ncap <= 0) return 0;
  if (!acl_table_ok(a) || ncap >= 0x7fffffff) return -1;
  if (ws_bytes < zk_tree_acl_workspace(ncap) || ((uintptr_t)ws & 15))
    return -1;
  zk::AclWs w;
  acl_layout(ncap, ws, &w);
  const unsigned nb = (unsigned)((ncap + zk::TR_T - 1) / zk::TR_T);
  zk::acl_intern_k<<<nb, zk::TR_T, 0, st>>>(*a, rx, foff, flen, n_dev, ncap,
                                            r_op, r_err, r_node, w);
  ZK_LAUNCH_CHECK();
  zk::acl_bind_k<<<nb, zk::TR_T, 0, st>>>(*a, rx, n_dev, ncap, r_node, w);
  ZK_LAUNCH_CHECK();
  return 0;
}

// Answer a batch of GET_ACL frames (foff / flen, *n_dev of them, at most
// ncap) from the tree and its ACL table: the framed replies in request order
// -> out[0, *total), their starts -> rec_off[ncap].  *err = 2 and *total = 0
// when the stream does not fit out_cap.  See acl_size_k above.
static int acl_get_launch(const ZkTree* t, const ZkAclTable* a,
                          const uint8_t* rx, const int64_t* foff,
                          const int32_t* flen, const int64_t* n_dev,
                          int64_t ncap, const zk::SegTable* M, uint8_t* ws,
                          int64_t ws_bytes, uint8_t* out, int64_t out_cap,
                          int64_t* rec_off, int64_t* total, int32_t* err,
                          int32_t terminate, hipStream_t st) {
  if (out_cap < 0) return -1;
  if (ncap <= 0) {
    if (hipMemsetAsync(total, 0, sizeof(int64_t), st) != hipSuccess) return -4;
    if (hipMemsetAsync(err, 0, sizeof(int32_t), st) != hipSuccess) return -4;
    if (terminate && out_cap >= 4 &&
        hipMemsetAsync(out, 0xFF, 4, st) != hipSuccess)
      return -4;
    return 0;
  }
  if (!acl_table_ok(a) || ncap >= (int64_t)0x7fffffff / zk::ACL_GROUP)
    return -1;
  if (ws_bytes < zk_tree_acl_workspace(ncap) || ((uintptr_t)ws & 15))
    return -1;
  zk::AclWs w;
  acl_layout(ncap, ws, &w);
  const unsigned nb = (unsigned)((ncap + zk::TR_T - 1) / zk::TR_T);
  if (M != nullptr)
    zk::acl_size_sess_k<<<nb, zk::TR_T, 0, st>>>(*t, *a, rx, foff, flen, n_dev,
                                                 ncap, w, *M);
  else
    zk::acl_size_k<<<nb, zk::TR_T, 0, st>>>(*t, *a, rx, foff, flen, n_dev,
                                            ncap, w);
  ZK_LAUNCH_CHECK();
  const int rc = zk_scan_excl_i64(w.sizes, rec_off, ncap, total, w.scan, st);
  if (rc) return rc;
  zk::acl_total_k<<<1, 1, 0, st>>>(total, out_cap, err, terminate, out, w);
  ZK_LAUNCH_CHECK();
  const unsigned nbw = (unsigned)((ncap * zk::ACL_GROUP + zk::TR_T - 1) /
                                  zk::TR_T);
  zk::acl_write_k<<<nbw, zk::TR_T, 0, st>>>(*t, *a, n_dev, ncap, w, rec_off,
                                            out);
  ZK_LAUNCH_CHECK();
  return 0;
}

int zk_tree_acl_get(const ZkTree* t, const ZkAclTable* a, const uint8_t* rx,
                    const int64_t* foff, const int32_t* flen,
                    const int64_t* n_dev, int64_t ncap, uint8_t* ws,
                    int64_t ws_bytes, uint8_t* out, int64_t out_cap,
                    int64_t* rec_off, int64_t* total, int32_t* err,
                    int32_t terminate, hipStream_t st) {
  return acl_get_launch(t, a, rx, foff, flen, n_dev, ncap, nullptr, ws,
                        ws_bytes, out, out_cap, rec_off, total, err,
                        terminate, st);
}

// zk_tree_acl_get for the GET_ACL frames of a session batch of any op mix:
// frame i belongs to segment f_seg[i] (zk_sess_split_segments' table of the
// GET_ACL class) and is served, or refused as zk_sess.h sess_refusal says
// (zk_sess_assign's seg_state / bad, S segments), header only.  g: the segment
// table; its sessions and wslots are not read.
int zk_tree_acl_get_sessions(const ZkTree* t, const ZkAclTable* a,
                             const uint8_t* rx, const int64_t* foff,
                             const int32_t* flen, const int64_t* n_dev,
                             int64_t ncap, const ZkSegs* g, uint8_t* ws,
                             int64_t ws_bytes, uint8_t* out, int64_t out_cap,
                             int64_t* rec_off, int64_t* total, int32_t* err,
                             int32_t terminate, hipStream_t st) {
  if (g == nullptr || g->f_seg == nullptr || g->seg_state == nullptr ||
      g->bad == nullptr || g->S < 1)
    return -1;
  const zk::SegTable M{g->f_seg, nullptr, g->seg_state, g->bad, g->S};
  return acl_get_launch(t, a, rx, foff, flen, n_dev, ncap, &M, ws, ws_bytes,
                        out, out_cap, rec_off, total, err, terminate, st);
}

// zk_tree_acl_get_sessions for a caller that serves SET_ACL (opcode 7; the
// split sent those frames here: zk_tree_mix_split_setacl).  The SET_ACL pass
// (tree_setacl.hip) runs over the class's frame table first, so a GET_ACL of
// the batch sees the new ACL; then the class is sized, the pass's frames put
// into their rows, and the one scan and one reply stream carry both ops in
// request order.  addrs (null: no ADMIN check) / au (null: no identities):
// the peers of the S segments; passes: the rounds a node; claim[claim_n]: the
// per-node claim words, all SETACL_IDLE between calls (claim_n >= the node
// capacity); stats[8] += the pass's counters; sws: zk_tree_setacl_workspace.
// A batch of the class without a SET_ACL frame produces the bytes
// zk_tree_acl_get_sessions produces.  No host read.
int zk_tree_acl_setacl_sessions(
    const ZkTree* t, const ZkAclTable* a, const uint8_t* rx, int64_t rx_len,
    const int64_t* foff, const int32_t* flen, const int64_t* n_dev,
    int64_t ncap, const ZkSegs* g, const int32_t* addrs,
    const ZkAuthTable* au, int32_t passes, int32_t* claim, int64_t claim_n,
    int64_t* stats, uint8_t* ws, int64_t ws_bytes, uint8_t* sws,
    int64_t sws_bytes, uint8_t* out, int64_t out_cap, int64_t* rec_off,
    int64_t* total, int32_t* err, int32_t terminate, hipStream_t st) {
  if (g == nullptr || g->f_seg == nullptr || g->seg_state == nullptr ||
      g->bad == nullptr || g->S < 1 || rx_len < 0 || passes < 0 ||
      passes > 64 || claim == nullptr || stats == nullptr)
    return -1;
  if (au != nullptr && (addrs == nullptr || au->recs == nullptr ||
                        au->cnt == nullptr || au->S < g->S))
    return -1;
  const zk::SegTable M{g->f_seg, nullptr, g->seg_state, g->bad, g->S};
  if (ncap <= 0)
    return acl_get_launch(t, a, rx, foff, flen, n_dev, ncap, &M, ws, ws_bytes,
                          out, out_cap, rec_off, total, err, terminate, st);
  if (out_cap < 0 || !acl_table_ok(a) ||
      ncap >= (int64_t)0x7fffffff / zk::ACL_GROUP)
    return -1;
  if (claim_n < a->cap || claim_n < t->store.cap) return -1;
  if (ws_bytes < zk_tree_acl_workspace(ncap) || ((uintptr_t)ws & 15) ||
      sws_bytes < zk::setacl_layout(ncap, nullptr, nullptr) ||
      ((uintptr_t)sws & 15))
    return -1;
  zk::AclWs w;
  acl_layout(ncap, ws, &w);
  zk::SetAclWs sw;
  zk::setacl_layout(ncap, sws, &sw);
  int rc = zk::setacl_pass(*t, *a, rx, rx_len, foff, flen, n_dev, ncap, M,
                           addrs, au, passes, claim, sw, stats, st);
  if (rc) return rc;
  const unsigned nb = (unsigned)((ncap + zk::TR_T - 1) / zk::TR_T);
  zk::acl_size_sess_k<<<nb, zk::TR_T, 0, st>>>(*t, *a, rx, foff, flen, n_dev,
                                               ncap, w, M);
  ZK_LAUNCH_CHECK();
  const zk::SetAclRows rows{w.xid, w.err, w.word, w.nslot, w.sizes, w.ctr};
  rc = zk::setacl_rows(n_dev, ncap, sw, rows, stats, st);
  if (rc) return rc;
  rc = zk_scan_excl_i64(w.sizes, rec_off, ncap, total, w.scan, st);
  if (rc) return rc;
  zk::acl_total_k<<<1, 1, 0, st>>>(total, out_cap, err, terminate, out, w);
  ZK_LAUNCH_CHECK();
  return zk::setacl_write(*t, *a, n_dev, ncap, sw, rows, rec_off, out, st);
}

}  // extern "C"
